"""Reconstruction panels and images end to end (model.log_reconstructions, trainer, imagelog.ImageWriter, evaluate.py
--save_reconstructions) on a small config at image size 64: which files appear, what is in them -- compared bit for bit with the
CPU rule of tests/egress_reference.py applied to the very tensors the step read -- and that switching the logging on changes
nothing that is trained."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import egress_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'
S, B = 64, 4
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC_STD = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
QC_GUMBEL = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='gumbel',
                 params=dict(straight_through=False, temp=1.0, kl_cost=5e-4, kl_warmup_epochs=0.5, temp_decay_epochs=2, temp_final=0.25))
LC_GAN = dict(l1_weight=0.8, l2_weight=0.2, perc_weight=1.0,
              adversarial_params=dict(start_epoch=0, loss_type='non-saturating', g_weight=0.1, use_adaptive=False,
                                      r1_reg_weight=10.0, r1_reg_every=2))


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.set_deterministic(False)


def _batches(count, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(B, 3, S, S, generator=g).to(DEV) for _ in range(count)]


def _model(qc=QC_STD, lc=None, dtype=torch.float32, seed=0):
    torch.manual_seed(seed)
    return model_mod.VQVAE(S, AE, qc, lc, TC, compute_dtype=dtype).to(DEV).train()


def _png(path):
    return torch.from_numpy(np.asarray(Image.open(path).convert('RGB')).copy())


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _rows(path):
    """(top row of cells, bottom row of cells) of a two-row panel of B images with padding 2, each as uint8 [B,S,S,3]; the
    padding must be zero"""
    panel = _png(path)
    assert tuple(panel.shape) == (2 * (S + 2) + 2, B * (S + 2) + 2, 3)
    rows = []
    mask = torch.ones(panel.shape[:2], dtype=torch.bool)
    for r in range(2):
        cells = []
        for c in range(B):
            y0, x0 = 2 + r * (S + 2), 2 + c * (S + 2)
            cells.append(panel[y0:y0 + S, x0:x0 + S])
            mask[y0:y0 + S, x0:x0 + S] = False
        rows.append(torch.stack(cells))
    assert int(panel[mask].max()) == 0
    return rows


def test_eager_fit_writes_exactly_the_due_files(tmp_path):
    """batch 2 of every fifth epoch (vqvae/model.py:241): 2 epochs x 4 batches -> epoch 0 only; 2 batches per epoch -> none"""
    for count, want in ((4, ['train/reconstructions_epoch=0000.png']), (2, [])):
        root = tmp_path / f'log{count}'
        m = _model()
        m.image_log_dir = str(root)
        tr = trainer_mod.MiniTrainer(max_epochs=2)
        tr.fit(m, _batches(count))
        m.close_image_log()
        assert _files(root) == want
    top, bottom = _rows(tmp_path / 'log4' / 'train' / 'reconstructions_epoch=0000.png')
    target = ops.raw_preprocess(_batches(4)[2], torch.float32, want_target=True)[1]
    assert torch.equal(top, R.egress(target, 'sym'))                    # the ground truths fed at batch 2, as the loss read them
    assert int(bottom.max()) > int(bottom.min())                        # (the eager reconstruction is gone: checked under replay)


@pytest.mark.parametrize('form', ['one_graph', 'split_graphs'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_graphed_mse_step_logs_the_fed_batch_and_the_static_reconstruction(tmp_path, monkeypatch, form, dtype):
    if form == 'split_graphs':
        # the data-parallel form of the capture (decoder backward / quantizer + deep encoder / encoder head as three graphs) in one
        # process: the choice of the form is forced, its collectives are no-ops without a process group
        monkeypatch.setenv('VQK_SPLIT_ENCODER_FRACTION', '0.5')
    m = _model(dtype=dtype)
    m.image_log_dir = str(tmp_path)
    tr = trainer_mod.MiniTrainer(max_epochs=1, num_training_batches=3)
    if form == 'split_graphs':
        tr._use_split = lambda model, opt: True
    tr.attach(m)
    m.on_train_start()
    feed = _batches(4, seed=11)
    tr.capture(m, feed[3], warmup=2, preserve_state=True)               # the capture-time batch is NOT one of the fed ones
    if form == 'split_graphs':
        assert tr._graph2 is not None
        print(f'IMAGELOGMEASURE split form: third graph {tr._graph3 is not None}')
    assert _files(tmp_path) == []                                       # neither the settling steps nor the capture logged
    for i in range(3):
        tr.train_batch_graphed(m, feed[i], i)
    m.flush_image_log()
    torch.cuda.synchronize()
    assert _files(tmp_path) == ['train/reconstructions_epoch=0000.png']
    top, bottom = _rows(tmp_path / 'train' / 'reconstructions_epoch=0000.png')
    target = ops.raw_preprocess(feed[2], m.compute_dtype, want_target=True)[1]
    assert torch.equal(top, R.egress(target, 'sym'))
    assert not torch.equal(top, R.egress(ops.raw_preprocess(feed[3], m.compute_dtype, want_target=True)[1], 'sym'))
    static_target, static_recon = tr._static_pair
    assert static_recon.dtype == dtype and static_recon.shape[1] == (8 if dtype == torch.bfloat16 else 4)
    assert torch.equal(bottom, R.egress(static_recon, 'sym'))           # what the replay of step 2 left
    assert torch.equal(top, R.egress(static_target, 'sym'))
    m.close_image_log()


def test_graphed_gumbel_vqgan_step_logs_the_fed_batch_and_the_static_reconstruction(tmp_path):
    m = _model(QC_GUMBEL, LC_GAN)
    m.image_log_dir = str(tmp_path)
    tr = trainer_mod.MiniTrainer(max_epochs=1, num_training_batches=3)
    tr.attach(m)
    m.on_train_start()
    feed = _batches(4, seed=12)
    tr.capture(m, feed[3], warmup=2, preserve_state=True)
    assert _files(tmp_path) == []                                       # the settling steps pass batch index 2: they must not log
    for i in range(3):
        tr.train_batch_graphed(m, feed[i], i)
    m.flush_image_log()
    torch.cuda.synchronize()
    assert _files(tmp_path) == ['train/reconstructions_epoch=0000.png']
    top, bottom = _rows(tmp_path / 'train' / 'reconstructions_epoch=0000.png')
    target = ops.raw_preprocess(feed[2], m.compute_dtype, want_target=True)[1]
    assert torch.equal(top, R.egress(target, 'sym'))
    assert not torch.equal(top, R.egress(ops.raw_preprocess(feed[3], m.compute_dtype, want_target=True)[1], 'sym'))
    assert torch.equal(bottom, R.egress(tr._static_pair[1], 'sym'))
    m.close_image_log()


def test_eager_gumbel_vqgan_step_logs_before_its_state_is_released(tmp_path):
    m = _model(QC_GUMBEL, LC_GAN)
    m.image_log_dir = str(tmp_path)
    tr = trainer_mod.MiniTrainer(max_epochs=1)
    feed = _batches(3, seed=13)
    tr.fit(m, feed)
    assert _files(tmp_path) == ['train/reconstructions_epoch=0000.png']
    top, _ = _rows(tmp_path / 'train' / 'reconstructions_epoch=0000.png')
    assert torch.equal(top, R.egress(ops.raw_preprocess(feed[2], torch.float32, want_target=True)[1], 'sym'))
    m.close_image_log()


def test_validate_writes_the_validation_panel(tmp_path):
    ops.set_deterministic(True)                                         # the forward is run twice and compared bit for bit
    m = _model()
    m.image_log_dir = str(tmp_path)
    m.current_epoch = 7                                                 # validation logs at batch 2 whatever the epoch (model.py:319)
    tr = trainer_mod.MiniTrainer()
    tr.attach(m)
    feed = _batches(3, seed=14)
    out = tr.validate(m, feed)
    assert np.isfinite(out['validation/loss'])
    assert _files(tmp_path) == ['validation/reconstructions_epoch=0007.png']          # flushed by validate itself
    top, bottom = _rows(tmp_path / 'validation' / 'reconstructions_epoch=0007.png')
    assert torch.equal(top, R.egress(ops.raw_preprocess(feed[2], torch.float32, want_target=True)[1], 'sym'))
    with torch.no_grad():
        m.eval()
        m.image_log_dir = None
        m._step_losses(feed[2], training=False, want_pair=True)
    assert torch.equal(bottom, R.egress(m._recon_pair[1], 'sym'))       # eval mode: the same forward again gives the same tensor
    m.close_image_log()


def _train(log_dir, graphed, steps=6):
    m = _model(seed=3)
    m.image_log_dir = log_dir
    tr = trainer_mod.MiniTrainer(max_epochs=2, num_training_batches=3, deterministic=True)
    tr.attach(m)
    m.on_train_start()
    feed = _batches(3, seed=15)
    if graphed:
        tr.capture(m, feed[0], warmup=1, preserve_state=True)
    step = tr.train_batch_graphed if graphed else tr.train_batch
    losses = []
    for k in range(steps):
        m.current_epoch = k // 3
        losses.append(float(step(m, feed[k % 3], k % 3)))
    m.close_image_log()
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    state['optimizer.v'] = tr.optimizers[0].flat_v.detach().cpu().clone()
    return losses, state


@pytest.mark.parametrize('graphed', [False, True])
def test_logging_has_no_effect_on_training(tmp_path, graphed):
    """deterministic fp32 mode, six steps with and without a log directory: every trained tensor and the optimizer's second
    moments are bit-identical.  The loss VALUES are compared to 1e-6 relative, not bit for bit: the value is an fp32 atomic sum
    over blocks in arrival order (vqk_sse; deterministic mode orders the GRADIENT sums, tests/test_gpu_deterministic.py), so two
    runs of the SAME configuration already differ in its last bits -- the bound is the one tests/test_gpu_data_loop.py
    documents for this sum.  The value feeds nothing: the gradient is computed from the tensors, not from it."""
    l_off, s_off = _train(None, graphed)
    l_on, s_on = _train(str(tmp_path), graphed)
    assert _files(tmp_path) == ['train/reconstructions_epoch=0000.png']
    print(f'IMAGELOGMEASURE graphed={graphed} losses off {l_off} on {l_on} bit-equal {l_off == l_on}')
    assert set(s_off) == set(s_on)
    for k in s_off:
        assert torch.equal(s_off[k], s_on[k]), k
    for a, b in zip(l_off, l_on):
        assert abs(a - b) <= 1e-6 * abs(a)


def _conf_and_ckpt(tmp_path):
    m = _model()
    with torch.no_grad():
        m.quantizer.codebook.weight.mul_(32.0)
    tr = trainer_mod.MiniTrainer()
    tr.attach(m)
    ckpt = str(tmp_path / 'model.ckpt')
    tr.save_checkpoint(m, ckpt)
    conf = tmp_path / 'conf.yaml'
    conf.write_text(f'image_size: {S}\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                    'quantizer:\n  num_embeddings: 64\n  embedding_dim: 16\n  type: standard\n  params:\n'
                    '    commitment_cost: 0.25\n  reinit_every_n_epochs:\n')
    return str(conf), ckpt


def _same_metrics(a, b):
    """codebook statistics exactly; mse / psnr / ssim to 1e-6 relative (atomic fp32 sums in arrival order: two runs of the same
    command differ in the last bits, tests/test_gpu_data_loop.py)"""
    assert set(a) == set(b)
    for k in a:
        if k in ('used_codebook', 'perplexity'):
            assert a[k] == b[k], k
        else:
            assert abs(a[k] - b[k]) <= 1e-6 * abs(b[k]), k


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_evaluate_saves_every_reconstruction(tmp_path, capsys, dtype):
    ev = importlib.import_module(PKG + '.evaluate')
    ops.set_deterministic(True)                                         # the forward is run again below and compared bit for bit
    conf, ckpt = _conf_and_ckpt(tmp_path)
    images = torch.rand(10, 3, S, S, generator=torch.Generator().manual_seed(21))
    pt = str(tmp_path / 'images.pt')
    torch.save(images, pt)
    common = ['--params_file', conf, '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', dtype, '--dataset_path', pt]
    plain = ev.main(common)
    out_dir = tmp_path / 'recon'
    capsys.readouterr()
    saved = ev.main(common + ['--save_reconstructions', str(out_dir), '--save_grid_every', '2'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == saved            # still one JSON line
    print('IMAGELOGMEASURE evaluate', dtype, 'plain', plain, 'saving', saved)
    _same_metrics(saved, plain)
    assert _files(out_dir) == sorted([f'{i:06d}.png' for i in range(10)] + ['grids/batch=000000.png', 'grids/batch=000002.png'])
    # the same model, the same batches: model.reconstruct
    cdt = torch.float32 if dtype == 'f32' else torch.bfloat16
    model = model_mod.VQVAE.load_from_checkpoint(ckpt, strict=False, image_size=S, ae_conf=AE, q_conf=QC_STD, l_conf=None, t_conf=None,
                                                 init_cb=False, load_loss=False, compute_dtype=cdt).to(DEV).eval()
    for start in range(0, 10, 4):
        batch = images[start:start + 4].to(DEV)
        want = R.egress(model.reconstruct(batch), 'unit')
        for j in range(batch.shape[0]):
            assert torch.equal(_png(out_dir / f'{start + j:06d}.png'), want[j]), start + j
        if start // 4 % 2 == 0:
            b = batch.shape[0]
            grid = R.image_grid([batch, model.reconstruct(batch)], b, 2, 0, 'unit')
            assert torch.equal(_png(out_dir / 'grids' / f'batch={start // 4:06d}.png'), grid)


def test_evaluate_names_folder_images_by_their_stem(tmp_path):
    ev = importlib.import_module(PKG + '.evaluate')
    conf, ckpt = _conf_and_ckpt(tmp_path)
    rng = np.random.default_rng(0)
    stems = ['b_first', 'a_second', 'zz', 'same', 'same']
    for k, stem in enumerate(stems):
        path = tmp_path / 'data' / 'test' / ('x' if k < 4 else 'y') / f'{stem}.png'
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)).save(path)
    out_dir = tmp_path / 'recon'
    ev.main(['--params_file', conf, '--batch_size', '2', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32', '--workers', '2',
             '--dataset_path', str(tmp_path / 'data'), '--save_reconstructions', str(out_dir)])
    names = _files(out_dir)
    assert len(names) == 5 and {'a_second.png', 'b_first.png', 'zz.png'} <= set(names)
    assert sum(n.startswith('same_') for n in names) == 2               # a stem met twice carries its dataset index
    assert all(tuple(_png(out_dir / n).shape) == (S, S, 3) for n in names)


@pytest.mark.parametrize('extra', [[], ['--no-graph']])
def test_train_py_writes_the_panels_under_the_run_name(tmp_path, capsys, extra):
    """train.py --image_log_dir, graphed and eager, on synthetic batches: DIR/run_name/train/reconstructions_epoch=0000.png"""
    train = importlib.import_module(PKG + '.train')
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'example_confs', 'standard_vqvae.yaml')
    args = ['--params_file', conf, '--seed', '3', '--max_epochs', '2', '--batches_per_epoch', '4', '--dtype', 'bf16',
            '--image_log_dir', str(tmp_path), '--run_name', 'r1', '--set', f'image_size={S}', '--set', 'autoencoder.channels=32',
            '--set', 'autoencoder.num_res_blocks=1', '--set', 'autoencoder.channel_multipliers=[1, 2]',
            '--set', 'quantizer.num_embeddings=64', '--set', 'quantizer.embedding_dim=16', '--set', 'training.cumulative_bs=4'] + extra
    capsys.readouterr()
    loss = train.main(args)
    out = capsys.readouterr().out
    assert np.isfinite(loss) and ('eager launches' in out) == False
    assert _files(tmp_path) == ['r1/train/reconstructions_epoch=0000.png']
    top, bottom = _rows(tmp_path / 'r1' / 'train' / 'reconstructions_epoch=0000.png')
    g = torch.Generator().manual_seed(3)                                # train.py's synthetic batches: the third one
    batch = [torch.rand(4, 3, S, S, generator=g) for _ in range(3)][2].to(DEV)
    assert torch.equal(top, R.egress(ops.raw_preprocess(batch, torch.bfloat16, want_target=True)[1], 'sym'))
    assert int(bottom.max()) > int(bottom.min())
