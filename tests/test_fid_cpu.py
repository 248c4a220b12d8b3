"""CPU checks of the rFID feature (fid.py, csrc/fid.hip): the float64 restatement of the FID Inception-v3 table
(tests/fid_reference.py) walks to the published size, the package's Frechet function agrees with the two published formulas, the
weights loader validates and folds, every new entry point refuses bad parameters before any launch, and evaluate.py accepts the
reference's command line."""
import importlib

import numpy as np
import pytest
import torch

from tests import fid_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
fid = importlib.import_module(PKG + '.fid')


def test_table_walk_counts():
    convs, out, totals = R.walk(299)
    assert len(convs) == 94
    assert out == (2048, 8, 8)
    assert totals == [192, 256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    flops = sum(2 * c['cout'] * c['oh'] * c['ow'] * c['kh'] * c['kw'] * c['cin'] for c in convs)
    assert round(flops / 1e9, 2) == 11.42, flops
    weights = sum(c['cout'] * c['cin'] * c['kh'] * c['kw'] for c in convs)
    assert round(weights / 1e6, 2) == 21.75, weights
    maps = [(c['name'], c['oh']) for c in convs]
    assert maps[0] == ('Conv2d_1a_3x3', 149) and maps[4] == ('Conv2d_4a_3x3', 71)
    assert dict(maps)['Mixed_6a.branch3x3'] == 17 and dict(maps)['Mixed_7a.branch3x3_2'] == 8


def test_package_table_matches_restatement():
    """fid.conv_specs (what the kernels run) is the restated table, conv for conv"""
    convs = R.walk(299)[0]
    specs = fid.conv_specs()
    assert list(specs) == [c['name'] for c in convs]
    for c in convs:
        assert specs[c['name']] == (c['cin'], c['cout'], c['kh'], c['kw'], c['stride'], c['ph'], c['pw']), c['name']
    assert dict(fid.expected_keys()) == R.state_dict_shapes()


def _random_cov(rng, d, n):
    f = rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) * 0.3 + rng.standard_normal(d)
    return R.stats(f)


@pytest.mark.parametrize('d,n', [(64, 200), (64, 40), (2048, 2500), (2048, 300)])
def test_frechet_matches_published_forms(d, n):
    rng = np.random.default_rng(d + n)
    mu1, s1 = _random_cov(rng, d, n)
    mu2, s2 = _random_cov(rng, d, n)
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    want_torchmetrics = R.fid_eigvals(mu1, s1, mu2, s2)
    assert abs(got - want_torchmetrics) <= 1e-6 * abs(want_torchmetrics), (got, want_torchmetrics)
    if d <= 64 or n > d:            # sqrtm of a singular product at d = 2048 takes minutes and loses its own accuracy
        want_pytorch_fid = R.fid_sqrtm(mu1, s1, mu2, s2)
        assert abs(got - want_pytorch_fid) <= 1e-6 * abs(want_pytorch_fid), (got, want_pytorch_fid)
    assert abs(got - fid.frechet_distance(mu2, s2, mu1, s1)) <= 1e-9 * abs(got)
    # FID(a, a) = 0 up to the square roots of rounding-level eigenvalues (the n - 1 < d null space when n < d)
    assert abs(fid.frechet_distance(mu1, s1, mu1, s1)) <= 1e-6 * np.trace(s1)


def test_loader_accepts_published_keys_and_folds_in_float64():
    sd = R.random_state_dict(seed=3, extras=True)
    folded = fid.load_weights(sd)
    assert len(folded) == 94
    for name in ('Conv2d_1a_3x3', 'Mixed_6c.branch7x7dbl_3', 'Mixed_7c.branch3x3dbl_3b'):
        w = sd[f'{name}.conv.weight'].double()
        g, b, m, v = (sd[f'{name}.bn.{p}'].double() for p in ('weight', 'bias', 'running_mean', 'running_var'))
        scale = g / torch.sqrt(v + 1e-3)
        fw, fb = folded[name]
        assert fw.dtype == torch.float32 and fb.dtype == torch.float32
        assert torch.equal(fw, (w * scale[:, None, None, None]).float())
        assert torch.equal(fb, (b - m * scale).float())


def test_loader_reads_a_file(tmp_path):
    sd = R.random_state_dict(seed=4, extras=False)
    path = tmp_path / 'inception.pth'
    torch.save(sd, path)
    folded = fid.load_weights(str(path))
    assert torch.equal(folded['Mixed_5b.branch_pool'][1], fid.load_weights(sd)['Mixed_5b.branch_pool'][1])


@pytest.mark.parametrize('key', ['Conv2d_1a_3x3.conv.weight', 'Mixed_6e.branch7x7dbl_5.bn.running_var',
                                 'Mixed_7c.branch_pool.bn.bias'])
def test_loader_rejects_missing_or_misshaped_keys(key):
    sd = R.random_state_dict(seed=5, extras=False)
    missing = dict(sd)
    del missing[key]
    with pytest.raises(KeyError, match=key.replace('.', r'\.')):
        fid.load_weights(missing)
    bad = dict(sd)
    bad[key] = torch.zeros(*(s + 1 for s in sd[key].shape))
    with pytest.raises(ValueError, match=key.replace('.', r'\.')):
        fid.load_weights(bad)


def test_loader_rejects_unknown_keys():
    sd = R.random_state_dict(seed=6, extras=False)
    sd['Mixed_8a.conv.weight'] = torch.zeros(1)
    with pytest.raises(KeyError, match='Mixed_8a'):
        fid.load_weights(sd)


def test_fid_entry_points_validate_without_gpu():
    lib = importlib.import_module(PKG + '._native').lib()
    SHAPE, ARG = -1, -5
    p = 4096                                                   # a non-NULL, 16-byte aligned stand-in: nothing is launched
    # conv: x, w, bias, y, n, h, wd, cin, cout, kh, kw, stride, ph, pw, oh, ow, c_total, c_off
    ok = [p, p, p, p, 2, 35, 35, 288, 64, 3, 3, 1, 1, 1, 35, 35, 288, 0, 0]

    def conv(**kw):
        args = list(ok)
        names = ['x', 'w', 'b', 'y', 'n', 'h', 'wd', 'cin', 'cout', 'kh', 'kw', 'stride', 'ph', 'pw', 'oh', 'ow', 'c_total', 'c_off']
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.vqk_fid_conv(*args)

    assert conv(kh=0) == SHAPE and conv(kw=8) == SHAPE and conv(stride=3) == SHAPE
    assert conv(c_off=250) == SHAPE                               # c_off + cout > c_total
    assert conv(cin=3) == SHAPE and conv(cin=0) == SHAPE and conv(cout=0) == SHAPE
    assert conv(ph=3) == SHAPE and conv(pw=-1) == SHAPE
    assert conv(oh=34) == SHAPE and conv(ow=36) == SHAPE and conv(n=0) == SHAPE
    assert conv(kh=1, kw=7, ph=0, pw=3, oh=36) == SHAPE            # explicit output size must be the conv's
    assert conv(x=0) == ARG and conv(b=0) == ARG                    # a valid shape gets as far as the pointers
    # pool: x, y, n, h, w, c, mode, stride, pad, oh, ow, c_total, c_off
    pool_ok = [p, p, 2, 35, 35, 288, 0, 2, 0, 17, 17, 768, 480, 0]     # valid: each case below breaks one parameter

    def pool(i, v):
        args = list(pool_ok)
        args[i] = v
        return lib.vqk_fid_pool(*args)
    assert pool(6, 2) == SHAPE                                      # mode
    assert pool(7, 3) == SHAPE                                      # stride
    assert pool(8, 2) == SHAPE                                      # pad
    assert pool(9, 18) == SHAPE                                     # output size
    assert pool(12, 484) == SHAPE                                   # c_off + c > c_total
    assert pool(12, 2) == SHAPE                                     # c_off % 4
    assert pool(5, 6) == SHAPE                                      # c % 4
    assert pool(0, 0) == ARG
    assert lib.vqk_fid_preprocess(p, 0, 256, 256, 1, 1, 1, 1, p, 0) == SHAPE
    assert lib.vqk_fid_preprocess(p, 2, 0, 256, 1, 1, 1, 1, p, 0) == SHAPE
    assert lib.vqk_fid_preprocess(p, 2, 256, 256, -1, 1, 1, 1, p, 0) == SHAPE
    assert lib.vqk_fid_preprocess(0, 2, 256, 256, 1, 1, 1, 1, p, 0) == ARG
    assert lib.vqk_fid_mean(p, p, 2, 0, 2048, 0) == SHAPE and lib.vqk_fid_mean(p, p, 0, 64, 2048, 0) == SHAPE
    assert lib.vqk_fid_mean(0, p, 2, 64, 2048, 0) == ARG
    assert lib.vqk_fid_stats(p, 0, 2048, p, p, 0) == SHAPE and lib.vqk_fid_stats(p, 4, 0, p, p, 0) == SHAPE
    assert lib.vqk_fid_stats(p, 4, 2048, 0, p, 0) == ARG


def test_evaluate_parses_reference_flags():
    ev = importlib.import_module(PKG + '.evaluate')
    a = ev.parse_args(['--params_file', 'example_confs/standard_vqvae.yaml', '--dataloader', 'standard', '--dataset_path',
                       'data.pt', '--batch_size', '16', '--seed', '0', '--loading_path', 'run.ckpt', '--workers', '4'])
    assert (a.params_file, a.dataset_path, a.batch_size, a.seed, a.loading_path, a.workers) == \
        ('example_confs/standard_vqvae.yaml', 'data.pt', 16, 0, 'run.ckpt', 4)
    assert a.fid_weights is None and a.dtype == 'bf16'
    b = ev.parse_args(['--params_file', 'c.yaml', '--dataset_path', 'd.npy', '--batch_size', '8', '--seed', '1',
                       '--loading_path', 'x.ckpt', '--fid_weights', 'pt_inception-2015-12-05-6726825d.pth', '--dtype', 'f32'])
    assert b.fid_weights == 'pt_inception-2015-12-05-6726825d.pth' and b.dtype == 'f32' and b.workers == 1
    with pytest.raises(SystemExit):
        ev.parse_args(['--params_file', 'c.yaml', '--batch_size', '8', '--seed', '1', '--loading_path', 'x.ckpt'])


def test_model_has_no_fid_by_default():
    model_mod = importlib.import_module(PKG + '.model')
    qc = dict(num_embeddings=16, embedding_dim=8, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
    m = model_mod.VQVAE(16, dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2)), qc, None, None)
    assert m.fid_weights is None
    keys = list(m.state_dict())
    m.fid_weights = 'inception.pth'
    assert list(m.state_dict()) == keys and all('fid' not in k for k in keys)
