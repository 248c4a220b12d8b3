"""rFID on the MI355X: every kernel of csrc/fid.hip and the whole FID Inception-v3 (fid.py) against the float64 restatement of
tests/fid_reference.py, then the test loop (VQVAE.fid_weights, MiniTrainer.test) and evaluate.py.

Bounds.  Preprocess: the quantised values are exact (at 299 x 299 the output is (q - 128) / 128 bit for bit), resized values are
within fp32 rounding.  Conv: the fp32-MFMA bound of the guide, |y - ref| <= c * sum |x w| (+ |b|), c = 1.5e-7 for K <= 1024 and
3.5e-7 beyond.  Max pools bit-exact, average pools and the mean within fp32 rounding.  Statistics: 1e-13 relative to
sum |f_i f_j|, bit-identical on repeat.  Whole network and FID: measured on an MI355X (worst per-image relative L2 of the
features 3.7e-7 at 256^2 / 299^2 / 512^2, relative FID error 4.0e-7, FID(a, a) 2.1e-6 of tr Sigma at n = 6), bounds at
about 10x.  mse / psnr / ssim of the test loop are sums of fp32 atomics across blocks (vqk_pair_stats, vqk_ssim_sum), so two runs
of the same loop may differ in the last bits: with and without rFID they are compared to 1e-6 relative."""
import importlib
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fid_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
fid = importlib.import_module(PKG + '.fid')
native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'

WHOLE_TOL = 4e-6          # measured 3.7e-7
FID_TOL = 4e-6            # measured 4.0e-7
SAME_TOL = 2e-5           # FID(a, a) / tr Sigma, measured 2.1e-6 (the square roots of rounding-level eigenvalues, n < d)
CANARY = 12345.0
# The guide's fp32-MFMA error (1.5e-7 sum |x w| at K <= 1024, 3.5e-7 beyond) is the typical size; the worst single output of a
# conv's ~10^5-10^6 reaches a few times it (measured: 3.2e-7 sum |x w| at K = 288), hence this factor.
CONV_WORST = 4.0


def _lib():
    return native.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _report(name, value):
    print(f'FIDMEASURE {name} {value:.3e}')


@pytest.fixture(scope='module')
def weights():
    return R.random_state_dict(seed=11, extras=True)


@pytest.fixture(scope='module')
def net(weights):
    return fid.InceptionFeatures(weights, DEV)


# ------------------------------------------------------------------------------------------------ 1. preprocess
def _images(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, 3, h, w, generator=g)
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = 1.0
    x.view(-1)[5::13] = 254.0 / 255.0
    return x


@pytest.mark.parametrize('hw', [(256, 256), (299, 299), (512, 512), (37, 51)])
@pytest.mark.parametrize('layout', ['nchw', 'channels_last_padded'])
def test_preprocess(net, hw, layout):
    h, w = hw
    x = _images(2, h, w, seed=h * 1000 + w)
    if layout == 'nchw':
        xd = x.to(DEV)
    else:
        pad = torch.full((2, 4, h, w), 7.0)
        pad[:, :3] = x
        xd = pad.to(DEV).contiguous(memory_format=torch.channels_last)[:, :3]
        assert not xd.is_contiguous()
    got = net.preprocess(xd).cpu()
    assert got.shape == (2, 299, 299, 4)
    assert torch.all(got[..., 3] == 0)
    want = R.preprocess(x).permute(0, 2, 3, 1)
    if hw == (299, 299):
        assert torch.equal(got[..., :3].double(), want)           # no resampling: the quantised values, exactly
    err = float((got[..., :3].double() - want).abs().max())
    _report(f'preprocess_{h}x{w}_{layout}', err)
    assert err <= 1e-6                                             # |v - 128| / 128 <= 1: a few fp32 ulps of 255 / 128


# ------------------------------------------------------------------------------------------------ 2. conv
def _table_shapes():
    seen = []
    for c in R.walk(299)[0]:
        if c['cin'] == 3:                                          # the first conv: a ragged case below (cin 3 padded to 4)
            continue
        key = (c['kh'], c['kw'], c['stride'], c['ph'], c['pw'], c['cin'], c['cout'], c['h'], c['w'])
        if key not in seen:
            seen.append(key)
    return seen


TABLE = _table_shapes()
RAGGED = [  # (kh, kw, stride, ph, pw, cin, cout, h, w, batch)
    (3, 3, 2, 0, 0, 3, 32, 299, 299, 1),          # the first conv: cin 3 padded to 4
    (1, 1, 1, 0, 0, 64, 80, 73, 73, 3),
    (5, 5, 1, 2, 2, 48, 48, 35, 35, 1),
    (3, 3, 2, 0, 0, 192, 320, 17, 17, 3),
    (1, 1, 1, 0, 0, 1280, 448, 8, 8, 3),
    (1, 7, 1, 0, 3, 20, 36, 9, 13, 1),
    (7, 1, 1, 3, 0, 8, 5, 11, 6, 3),
    (3, 3, 2, 0, 0, 4, 7, 4, 5, 1),
]


def _run_conv(kh, kw, stride, ph, pw, cin, cout, h, w, b, seed):
    g = torch.Generator().manual_seed(seed)
    cin_p = (cin + 3) // 4 * 4
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    oh, ow = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
    c_off, c_total = 4, cout + 12                                 # canaries on both sides of the slice
    xd = F.pad(x, (0, 0, 0, 0, 0, cin_p - cin)).permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = F.pad(wt, (0, 0, 0, 0, 0, cin_p - cin)).permute(0, 2, 3, 1).contiguous().to(DEV)
    bd = bias.to(DEV)
    y = torch.full((b, oh, ow, c_total), CANARY, device=DEV)
    native.check(_lib().vqk_fid_conv(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), b, h, w, cin_p, cout, kh, kw,
                                     stride, ph, pw, oh, ow, c_total, c_off, _st()), 'fid_conv')
    y = y.cpu()
    ref = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=(ph, pw))).permute(0, 2, 3, 1)
    mag = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1)
    k = kh * kw * cin
    c = CONV_WORST * (1.5e-7 if k <= 1024 else 3.5e-7)
    got = y[..., c_off:c_off + cout].double()
    ratio = float(((got - ref).abs() / (mag + 1e-30)).max())
    assert torch.all(y[..., :c_off] == CANARY) and torch.all(y[..., c_off + cout:] == CANARY)
    assert torch.all((got - ref).abs() <= c * mag + 1e-30), ratio
    return ratio


@pytest.mark.parametrize('shape', TABLE, ids=[f'{s[0]}x{s[1]}s{s[2]}p{s[3]}{s[4]}_{s[5]}-{s[6]}_{s[7]}' for s in TABLE])
def test_conv_table_shapes(shape):
    kh, kw, stride, ph, pw, cin, cout, h, w = shape
    r = _run_conv(kh, kw, stride, ph, pw, cin, cout, h, w, 2, seed=hash(shape) % 10000)
    _report(f'conv_{shape}', r)


@pytest.mark.parametrize('shape', RAGGED)
def test_conv_ragged(shape):
    r = _run_conv(*shape, seed=sum(shape))
    _report(f'conv_ragged_{shape}', r)


# ------------------------------------------------------------------------------------------------ 3. pools
@pytest.mark.parametrize('form', ['max_s2', 'max_s1p1', 'avg_s1p1'])
@pytest.mark.parametrize('hwc', [(35, 35, 288), (17, 17, 768), (8, 8, 1280), (9, 6, 12)])
def test_pools(form, hwc):
    h, w, c = hwc
    mode, stride, pad = {'max_s2': (0, 2, 0), 'max_s1p1': (0, 1, 1), 'avg_s1p1': (1, 1, 1)}[form]
    g = torch.Generator().manual_seed(h * w + c)
    x = torch.randn(2, h, w, c, generator=g)
    oh, ow = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
    c_off, c_total = 8, c + 16
    y = torch.full((2, oh, ow, c_total), CANARY, device=DEV)
    xd = x.to(DEV)
    native.check(_lib().vqk_fid_pool(xd.data_ptr(), y.data_ptr(), 2, h, w, c, mode, stride, pad, oh, ow, c_total, c_off, _st()),
                 'fid_pool')
    y = y.cpu()
    assert torch.all(y[..., :c_off] == CANARY) and torch.all(y[..., c_off + c:] == CANARY)
    xn = x.double().permute(0, 3, 1, 2)
    if mode == 0:
        ref = F.max_pool2d(xn, 3, stride, pad).permute(0, 2, 3, 1)
        assert torch.equal(y[..., c_off:c_off + c].double(), ref)
    else:
        ref = F.avg_pool2d(xn, 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1)
        err = float((y[..., c_off:c_off + c].double() - ref).abs().max())
        _report(f'avgpool_{hwc}', err)
        assert err <= 2e-6 * float(xn.abs().max())


def test_global_mean():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 8, 8, 2048, generator=g).abs()
    xd = x.to(DEV)
    y = torch.empty(3, 2048, device=DEV)
    native.check(_lib().vqk_fid_mean(xd.data_ptr(), y.data_ptr(), 3, 64, 2048, _st()), 'fid_mean')
    ref = x.double().mean(dim=(1, 2))
    err = float(((y.cpu().double() - ref).abs() / ref).max())
    _report('global_mean', err)
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. statistics
def _stats(f, sums=None, gram=None):
    d = f.shape[1]
    sums = torch.zeros(d, dtype=torch.float64, device=DEV) if sums is None else sums
    gram = torch.zeros(d, d, dtype=torch.float64, device=DEV) if gram is None else gram
    native.check(_lib().vqk_fid_stats(f.data_ptr(), f.shape[0], d, sums.data_ptr(), gram.data_ptr(), _st()), 'fid_stats')
    return sums, gram


@pytest.mark.parametrize('n', [1, 7, 64, 257])
def test_statistics(n):
    d = 2048
    g = torch.Generator().manual_seed(n)
    f = torch.relu(torch.randn(n, d, generator=g)) * 3.0
    fd = f.to(DEV)
    s, G = _stats(fd)
    f64 = f.double().numpy()
    ref_s, ref_g = f64.sum(0), f64.T @ f64
    mag = np.abs(f64).T @ np.abs(f64)
    assert np.all(np.abs(G.cpu().numpy() - ref_g) <= 1e-13 * mag + 1e-300)
    assert np.all(np.abs(s.cpu().numpy() - ref_s) <= 1e-13 * np.abs(f64).sum(0) + 1e-300)
    s2, G2 = _stats(fd)
    assert torch.equal(s, s2) and torch.equal(G, G2)
    assert torch.equal(G, G.T)
    if n > 1:
        k = n // 3 + 1
        sp, Gp = _stats(fd[:k].contiguous())
        _stats(fd[k:].contiguous(), sp, Gp)
        assert torch.equal(sp, s) and torch.equal(Gp, G)


# ------------------------------------------------------------------------------------------------ 5. whole network
@pytest.mark.parametrize('size', [256, 299, 512])
def test_whole_network(net, weights, size):
    x = _images(2, size, size, seed=size)
    got = net.features(x.to(DEV)).cpu().double()
    want = R.features(x, weights, device=DEV).cpu()
    assert got.shape == (2, 2048)
    rel = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
    _report(f'whole_{size}', rel)
    assert rel <= WHOLE_TOL


# ------------------------------------------------------------------------------------------------ 6. FID end to end
def test_fid_end_to_end(net, weights):
    g = torch.Generator().manual_seed(5)
    real = torch.rand(6, 3, 64, 64, generator=g)
    fake = (real + 0.15 * torch.randn(6, 3, 64, 64, generator=g)).clamp(0, 1)
    m = fid.FrechetInceptionDistance(net)
    m.update(real[:4].to(DEV), True)
    m.update(real[4:].to(DEV), True)
    m.update(fake.to(DEV), False)
    got = m.compute()
    fr = R.features(real, weights, device=DEV).cpu().numpy()
    ff = R.features(fake, weights, device=DEV).cpu().numpy()
    (mu1, s1), (mu2, s2) = R.stats(fr), R.stats(ff)
    want = R.fid_eigvals(mu1, s1, mu2, s2)
    rel = abs(got - want) / abs(want)
    _report('fid_rel', rel)
    assert rel <= FID_TOL, (got, want)
    same = fid.FrechetInceptionDistance(net)
    same.update(real.to(DEV), True)
    same.update(real.to(DEV), False)
    assert abs(same.compute()) <= SAME_TOL * np.trace(s1)
    m.reset()
    assert m.counts == {True: 0, False: 0} and float(m.grams[True].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 7. test loop
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
QC = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def _small_model():
    model_mod = importlib.import_module(PKG + '.model')
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, QC, None, TC)
    with torch.no_grad():
        m.quantizer.codebook.weight.mul_(32.0)
    return m.to(DEV)


@pytest.fixture(scope='module')
def weights_file(weights, tmp_path_factory):
    path = tmp_path_factory.mktemp('fid') / 'inception_random.pth'
    torch.save(weights, path)
    return str(path)


def test_test_loop_rfid(weights_file):
    trainer_mod = importlib.import_module(PKG + '.trainer')
    model = _small_model()
    keys = list(model.state_dict())
    n_params = sum(p.numel() for p in model.parameters())
    g = torch.Generator().manual_seed(9)
    batches = [torch.rand(4, 3, 32, 32, generator=g).to(DEV) for _ in range(2)]
    plain = trainer_mod.MiniTrainer().test(model, batches)
    assert 'rfid' not in plain
    model.fid_weights = weights_file
    with_fid = trainer_mod.MiniTrainer().test(model, batches)
    for k in ('mse', 'psnr', 'ssim'):
        assert abs(float(with_fid[k]) - float(plain[k])) <= 1e-6 * abs(float(plain[k])), k
    for k in ('used_codebook', 'perplexity'):
        assert float(with_fid[k]) == float(plain[k]), k
    assert list(model.state_dict()) == keys and sum(p.numel() for p in model.parameters()) == n_params
    assert not any('fid' in name or 'Mixed' in name for name, _ in model.named_modules())
    standalone = fid.FrechetInceptionDistance(weights_file, DEV)
    with torch.no_grad():
        for b in batches:
            recon = model.preprocess_visualization(model(model.preprocess_batch(b))[0].float())[:, :3]
            standalone.update(b, True)
            standalone.update(recon, False)
    want = standalone.compute()
    assert np.isfinite(with_fid['rfid']) and with_fid['rfid'] > 0
    assert abs(with_fid['rfid'] - want) <= 1e-9 * abs(want), (with_fid['rfid'], want)
    again = trainer_mod.MiniTrainer().test(model, batches)        # the cached network, statistics reset per epoch
    assert again['rfid'] == with_fid['rfid']
    model.fid_weights = None
    assert 'rfid' not in trainer_mod.MiniTrainer().test(model, batches)


# ------------------------------------------------------------------------------------------------ 8. evaluate.py
def test_evaluate_main(weights_file, tmp_path, capsys):
    trainer_mod = importlib.import_module(PKG + '.trainer')
    ev = importlib.import_module(PKG + '.evaluate')
    model = _small_model()
    tr = trainer_mod.MiniTrainer()
    tr.attach(model)
    ckpt = str(tmp_path / 'model.ckpt')
    tr.save_checkpoint(model, ckpt)
    conf = tmp_path / 'conf.yaml'
    conf.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                    'quantizer:\n  num_embeddings: 64\n  embedding_dim: 16\n  type: standard\n  params:\n'
                    '    commitment_cost: 0.25\n  reinit_every_n_epochs:\n')
    data = str(tmp_path / 'images.pt')
    torch.save(torch.rand(7, 3, 32, 32, generator=torch.Generator().manual_seed(1)), data)
    capsys.readouterr()
    out = ev.main(['--params_file', str(conf), '--dataset_path', data, '--batch_size', '3', '--seed', '0', '--loading_path',
                   ckpt, '--workers', '2', '--fid_weights', weights_file, '--dtype', 'f32'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    printed = json.loads(lines[0])
    assert set(printed) == {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity', 'rfid'}
    assert printed == out and all(np.isfinite(v) for v in printed.values())
