"""The finite scalar quantizer on the GPU (csrc/fsq.hip, csrc/proj_quant.h, _ops_proj.py, FSQuantizer) against the float64 reference of
tests/fsq_reference.py.

Tokens are integers: the device must return the reference's token on EVERY row -- the generator removed the rows within 1e-3 of a
rounding boundary, a float32 evaluation moves ``bounded`` by < 1e-5.  Real-valued results are compared in the metric max|got - want| /
max|want|.  The bound is measured, not fixed: e32 = the distance of the float32 numpy evaluation of the same formulas to float64 on
the same inputs; the device may be at max(16 * e32, 1e-6) -- sixteen because it sums up to 2051 rows in another order (per-lane
registers, wave order, block slabs) and uses its own tanh; a wrong term, sign or dropped row is off by >= 1e-2 in this metric.  Every
figure is printed (``FSQMEASURE``) before it is asserted.

Measured on an MI355X, largest e32 / largest device distance over the twelve shapes and both dq dtypes: u 5.9e-7 / 3.0e-7, q 1.2e-7 /
1.2e-7, dz 8.2e-6 / 9.1e-7, dW_in 8.2e-6 / 1.6e-6, dW_out 6.0e-7 / 1.6e-7, db_out 1.6e-6 / 1.7e-7, db_in 9.3e-6 / 1.3e-5 -- and 5.3e-4 /
6.5e-4 for db_in at N = 2051, D = 1024, levels [2]: one scalar whose 2051 terms cancel, the float32 evaluation loses the same digits.
Every case is inside its own bound; the closest is a factor 8 below it."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import fsq_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
vqm = importlib.import_module(PKG + '.modules.vector_quantizers')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

L1, L2, L4, L8 = (2,), (3, 3), (8, 5, 5, 5), (2, 3, 4, 5, 6, 7, 8, 9)
# (N, D, levels): D = 256 production / 64 one chunk per lane / 20 a partly idle wave / 512 several chunks per lane, two backward
# slices / 1024 the upper bound (64 KiB of LDS with d = 8); N = 1 / 67 ragged against the 4 rows of a block / 2051 > one pass of the
# backward's fixed grid, with a tail; d = 1, binary, odd and even levels, d = 8 with K = 362,880
CASES = [(2051, 256, L4), (67, 256, L4), (1, 256, L4), (2051, 64, L2), (67, 20, L1), (67, 512, L4), (67, 1024, L8), (2051, 256, L8),
         (1, 20, L2), (67, 64, L8), (2051, 1024, L1), (1, 512, L1)]
_REF: dict = {}


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def reference(case):
    """inputs + float64 and float32 evaluations of one case, computed once and shared (read-only) by the tests that need it"""
    if case not in _REF:
        n, dm, levels = case
        inp = R.make_inputs(1000 + len(_REF), n, dm, levels)
        args = tuple(inp[k] for k in ('z', 'w_in', 'b_in', 'w_out', 'b_out'))
        ent = dict(inp=inp, f64=R.forward(*args, levels), f32=R.forward(*args, levels, dtype=np.float32), b64={}, b32={})
        for dq_name, dq in (('fp32', inp['dq']), ('bf16', bf16_round(inp['dq']))):
            ent['b64'][dq_name] = R.backward(*args, dq, levels)
            ent['b32'][dq_name] = R.backward(*args, dq, levels, dtype=np.float32)
        for part in ent.values():
            for arr in (part.values() if isinstance(part, dict) else ()):
                if isinstance(arr, np.ndarray):
                    arr.setflags(write=False)
        _REF[case] = ent
    return _REF[case]


def dev_inputs(inp, n, dm):
    """device tensors of one case: z as the [1, D, N, 1] NHWC map whose memory is the [N][D] rows, the four parameters as leaves"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    z = t(inp['z']).view(1, n, 1, dm).permute(0, 3, 1, 2).requires_grad_(True)
    return z, [t(inp[k]).requires_grad_(True) for k in ('w_in', 'b_in', 'w_out', 'b_out')]


def bound(e32):
    return max(16.0 * e32, 1e-6)


def check(name, case, got, want64, want32, extra=''):
    e32, dist = R.distance(want32, want64), R.distance(got, want64)
    print(f'FSQMEASURE {name} N={case[0]} D={case[1]} levels={list(case[2])} {extra} e32 {e32:.3e} device {dist:.3e} bound {bound(e32):.3e}')
    assert dist <= bound(e32), (name, case, dist, e32)


def bf16_ulp(x):
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - 8)                     # |x| in [2^(e-1), 2^e): 8 significant bits


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'N{c[0]}-D{c[1]}-d{len(c[2])}')
def test_forward(case):
    n, dm, levels = case
    ref = reference(case)
    f64, f32 = ref['f64'], ref['f32']
    k = int(np.prod(levels))
    z, params = dev_inputs(ref['inp'], n, dm)
    with torch.no_grad():
        q, idx, loss, hist = ops.FSQFn.apply(z, *params, levels, torch.float32)
        qb, idxb, _, histb = ops.FSQFn.apply(z, *params, levels, torch.bfloat16)
        flat = z.permute(0, 2, 3, 1).reshape(n, dm)
        lib, native = importlib.import_module(PKG + '._native').lib(), importlib.import_module(PKG + '._native')
        u = torch.empty(n, len(levels), device=DEV)
        idx_raw = torch.empty(n, dtype=torch.int64, device=DEV)
        native.check(lib.vqk_fsq_forward(flat.data_ptr(), params[0].data_ptr(), params[1].data_ptr(), 0, 0, n, dm, len(levels),
                                         ops._levels_arg(levels)[0], idx_raw.data_ptr(), u.data_ptr(), 0, 0, 0, ops._stream()), 'fsq_forward')
    torch.cuda.synchronize()
    assert q.dtype == torch.float32 and qb.dtype == torch.bfloat16 and tuple(q.shape) == (1, dm, n, 1) and tuple(idx.shape) == (1, n)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss) == 0.0
    want_idx = f64['idx']
    for got in (idx, idxb, idx_raw):
        np.testing.assert_array_equal(got.reshape(-1).cpu().numpy(), want_idx)          # every row
    assert hist.dtype == torch.int32 and hist.numel() == k
    for h in (hist, histb):
        np.testing.assert_array_equal(h.cpu().numpy(), np.bincount(want_idx, minlength=k))
    check('u', case, u.cpu().numpy(), f64['u'], f32['u'])
    qrows = q.permute(0, 2, 3, 1).reshape(n, dm).cpu().numpy()
    check('q', case, qrows, f64['q'], f32['q'])
    # bf16 output: the fp32 value above, rounded -- one bf16 ulp of the (rounded) reference, plus the fp32 error already allowed
    got_b = qb.permute(0, 2, 3, 1).reshape(n, dm).float().cpu().numpy().astype(np.float64)
    want_b = bf16_round(f64['q'])
    allowed = bf16_ulp(np.maximum(np.abs(got_b), np.abs(want_b))) + bound(R.distance(f32['q'], f64['q'])) * np.abs(f64['q']).max()
    worst = float((np.abs(got_b - want_b) / allowed).max())
    print(f'FSQMEASURE q_bf16 N={n} D={dm} levels={list(levels)} worst |diff| / allowed {worst:.3f}')
    assert worst <= 1.0
    np.testing.assert_array_equal(got_b, bf16_round(qrows))                             # and exactly the rounding of the fp32 output


@pytest.mark.parametrize('dq_name', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'N{c[0]}-D{c[1]}-d{len(c[2])}')
def test_backward(case, dq_name):
    n, dm, levels = case
    ref = reference(case)
    b64, b32 = ref['b64'][dq_name], ref['b32'][dq_name]
    dq = torch.tensor(ref['inp']['dq'], dtype=torch.float32, device=DEV).view(1, n, 1, dm).permute(0, 3, 1, 2)
    if dq_name == 'bf16':
        dq = dq.to(torch.bfloat16)
    runs = []
    for _ in range(2):
        z, params = dev_inputs(ref['inp'], n, dm)
        q = ops.FSQFn.apply(z, *params, levels, dq.dtype)[0]
        q.backward(dq)
        torch.cuda.synchronize()
        runs.append([z.grad.permute(0, 2, 3, 1).reshape(n, dm)] + [p.grad for p in params])
    names = ('dz', 'dw_in', 'db_in', 'dw_out', 'db_out')
    for name, a, b in zip(names, *runs):                                                # the same bits, run to run, in every mode
        assert torch.equal(a, b), name
    for name, got in zip(names, runs[0]):
        assert got.dtype == torch.float32 and tuple(got.shape) == b64[name].shape
        check(name, case, got.cpu().numpy(), b64[name], b32[name], extra=f'dq={dq_name}')


@pytest.mark.parametrize('case', [(67, 256, L4), (2051, 64, L2), (67, 1024, L8), (1, 20, L2), (67, 20, L1)],
                         ids=lambda c: f'N{c[0]}-D{c[1]}-d{len(c[2])}')
def test_decode_has_the_forwards_bits(case):
    n, dm, levels = case
    ref = reference(case)
    z, params = dev_inputs(ref['inp'], n, dm)
    k = int(np.prod(levels))
    with torch.no_grad():
        for dtype in (torch.float32, torch.bfloat16):
            q, idx, _, _ = ops.FSQFn.apply(z, *params, levels, dtype)
            dec = ops.fsq_decode(idx, params[2], params[3], levels, dtype)
            assert dec.dtype == dtype and tuple(dec.shape) == (1, n, dm)
            assert torch.equal(dec.reshape(n, dm), q.permute(0, 2, 3, 1).reshape(n, dm))
        # an index outside [0, K) decodes to SOME code's vector (arithmetic on the index, no table)
        wild = torch.tensor([-1, k, 2 ** 40 + 3, -2 ** 62], dtype=torch.int64, device=DEV)
        out = ops.fsq_decode(wild, params[2], params[3], levels)
        assert bool(torch.isfinite(out).all())
        if k > 1000:
            return
        # the module over the same parameters: implicit tokens, decoder-side codebook, vec_to_codes
        quant = vqm.FSQuantizer(k, dm, levels).to(DEV)
        quant.project_in.weight.copy_(params[0].view(len(levels), dm, 1, 1)); quant.project_in.bias.copy_(params[1])
        quant.project_out.weight.copy_(params[2].view(dm, len(levels), 1, 1)); quant.project_out.bias.copy_(params[3])
        q, idx, _ = quant(z)
        rows = q.permute(0, 2, 3, 1).reshape(n, dm)
        np.testing.assert_array_equal(idx.reshape(-1).cpu().numpy(), ref['f64']['idx'])
        assert int(quant.last_hist.sum()) == n
        assert torch.equal(quant.vec_to_codes(z), idx)
        assert torch.equal(quant.codes_to_vec(idx).reshape(n, dm), rows)
        book = quant.get_codebook()
        assert tuple(book.shape) == (k, dm) and torch.equal(book[idx.reshape(-1)], rows)
        assert all(bool((book == row).all(1).any()) for row in out)


# ---------------------------------------------------------------------------------------------- module / model
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC = dict(num_embeddings=1000, embedding_dim=64, reinit_every_n_epochs=None, type='fsq', params=dict(levels=[8, 5, 5, 5]))


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, tmp_path):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, QC, None, TC, compute_dtype=dtype).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = tr.train_batch(m, images, 0)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    assert float(m.logged['train/quant_loss']) == 0.0
    assert int(m.quantizer.last_hist.sum()) == 4 * 8 * 8 and m.quantizer.last_hist.numel() == 1000
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    for k in ('quantizer.project_in.weight', 'quantizer.project_in.bias', 'quantizer.project_out.weight', 'quantizer.project_out.bias',
              'encoder.conv_in.weight', 'encoder.conv_out.weight', 'decoder.conv_in.weight', 'decoder.conv_out.weight'):
        assert k in changed, k
    assert 'quantizer.codebook.weight' not in changed
    assert {k.split('.')[0] for k in changed} == {'encoder', 'decoder', 'quantizer'}

    m.eval()
    with torch.no_grad():
        # index parity on latents the device produced: its own fp32 z through the float64 reference; rows within 1e-4 of a rounding
        # boundary are left out -- at most 2 % of the rows -- and every other row must match
        z = m.encoder(m.preprocess_batch(images))
        assert z.dtype == torch.float32
        _, idx, q_loss = m.quantizer(z)
        rows = z.permute(0, 2, 3, 1).reshape(-1, 64).cpu().numpy().astype(np.float64)
        qz = m.quantizer
        f64 = R.forward(rows, qz.project_in.weight.detach().reshape(4, 64).cpu().numpy(), qz.project_in.bias.detach().cpu().numpy(),
                        qz.project_out.weight.detach().reshape(64, 4).cpu().numpy(), qz.project_out.bias.detach().cpu().numpy(), (8, 5, 5, 5))
        keep = R.boundary_distance(f64['bounded']) >= 1e-4
        share = 1.0 - float(keep.mean())
        print(f'FSQMEASURE model rows left out {share:.4f} of {keep.size}')
        assert share <= 0.02
        np.testing.assert_array_equal(idx.reshape(-1).cpu().numpy()[keep], f64['idx'][keep])
        assert float(q_loss) == 0.0
        # the same decode function on both paths: bit for bit
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64) and torch.equal(tokens, idx)
        # (the autoencoder's GroupNorm sums are combined in arrival order by default: bits are compared in deterministic mode)
        ops.set_deterministic(True)
        try:
            tokens_det = m.get_tokens(images)
            assert torch.equal(m.reconstruct_from_tokens(tokens_det), m.reconstruct(images))
        finally:
            ops.set_deterministic(False)
        assert tuple(m.quantize(images).shape) == (4, 64, 64)
    path = str(tmp_path / 'fsq.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, AE, QC, None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.get_tokens(images), tokens)
    assert torch.equal(m2.quantizer.codebook.weight, m.quantizer.codebook.weight)


# The last Upsample's conv bias feeds a GroupNorm with ONE channel per group (32 channels / 32 groups): its gradient is analytically
# zero, what arrives is rounding noise, and AdamW (beta1 = 0) turns the SIGN of that noise into a full +-lr update -- its trajectory
# is not a function of the step (tests/test_gpu_train_step.py leaves the same tensor out for the same reason).
ZERO_GRAD = {'decoder.blocks.3.conv.bias'}


def test_graph_replay_matches_eager():
    """MiniTrainer.capture + three replays against eager steps from the same state: parameters and token histograms, at the tolerance
    tests/test_gpu_train_step.py uses for the standard quantizer (rtol 2e-3, atol 1e-5); the static histogram follows each replay"""
    images = [_images(seed=3 + i) for i in range(5)]
    losses, state, hists = {}, {}, {}
    for mode in ('eager', 'graph'):
        torch.manual_seed(0)
        m = model_mod.VQVAE(32, AE, QC, None, TC).to(DEV).train()
        tr = trainer_mod.MiniTrainer(num_training_batches=100)
        tr.attach(m)
        m.on_train_start()
        out, hs = [], []
        if mode == 'graph':
            tr.capture(m, images[0], warmup=2)
            for i in range(3):
                out.append(tr.train_batch_graphed(m, images[2 + i], 2 + i).item())
                hs.append(m.quantizer.last_hist.cpu().clone())
                assert m.quantizer.last_hist.data_ptr() == tr._static_hist.data_ptr()
        else:
            for i in range(5):
                out.append(tr.train_batch(m, images[0] if i < 2 else images[i], i).item())
                hs.append(m.quantizer.last_hist.cpu().clone())
            out, hs = out[2:], hs[2:]
        torch.cuda.synchronize()
        losses[mode], hists[mode] = out, hs
        state[mode] = {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()}
    np.testing.assert_allclose(losses['graph'], losses['eager'], rtol=2e-3)
    for k in state['eager']:
        if k in ZERO_GRAD:
            continue
        np.testing.assert_allclose(state['graph'][k].numpy(), state['eager'][k].numpy(), rtol=2e-3, atol=1e-5, err_msg=k)
    for a, b in zip(hists['graph'], hists['eager']):
        assert int(a.sum()) == 4 * 8 * 8
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-3, atol=1e-5)
    assert not torch.equal(hists['graph'][0], hists['graph'][1])                        # different batches: the histogram followed


SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'quantizer.embedding_dim=64', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'fsq_vqvae.yaml')
    common = ['--params_file', conf] + SMALL + ['--max_epochs', '2', '--batches_per_epoch', '3', '--seed', '0', '--dtype', 'f32']
    capsys.readouterr()
    loss = train.main(common + ['--save_path', str(tmp_path), '--run_name', 'fsq'])
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                                                  # the graph was captured, not given up
    loss_eager = train.main(common + ['--no-graph'])
    assert np.isfinite(loss_eager)
    ckpt = str(tmp_path / 'fsq' / 'epoch=01.ckpt')
    assert os.path.exists(ckpt)
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     'quantizer:\n  num_embeddings: 1000\n  embedding_dim: 64\n  type: fsq\n  params:\n'
                     '    levels: [8, 5, 5, 5]\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res)
    assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 1000.0
