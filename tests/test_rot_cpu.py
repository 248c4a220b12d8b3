"""The rotation-trick gradient of the standard and EMA quantizers (``quantizer.params.gradient: rotation``; csrc/vq_rot.hip) on the CPU:
the float64 reference (tests/rot_reference.py) against torch.autograd of the detached formulation and a central difference, q~ == q,
the degenerate rows, the config surface -- and the tolerance accounting of the GPU tests (tests/test_gpu_rot.py).

TOLERANCES.  The base bounds are the ones the project already uses for these two quantities in tests/test_gpu_rvq.py: dz rtol 1e-5 /
atol 1e-7, de rtol 1e-4 / atol 1e-7.  dz ends in a sum of four terms that cancel in part (lam g + A z + B q + cz (z - q)), which leaves
the rounding relative to the terms (lam |g|: a few ulp of it), not to a small result.  ``RESTATEMENT`` records, per (kind, D), the worst
error / (atol + rtol |want|) of ``rot_reference.staged_f32`` -- an fp32 evaluation through the five dot products on the CPU, NOT the
kernels -- against float64 over every case of that (kind, D), both flavours of the restatement, both gradient dtypes (fp32,
bf16-rounded) and both loss cotangents (none, 0.7), measured here (test_restatement_error_is_the_recorded_one re-measures it on every
run).  Where that figure exceeds 1 the GPU bound of that (kind, D) is 4 x the figure (``bound_scale``, as tests/test_cos_cpu.py does);
everywhere else it is the stated tolerance itself.  The inputs are chosen so that no scaling is needed at all: with a decoder gradient
of 0.03 * randn every figure is at most 0.34, which leaves the kernels -- another evaluation order, another draw of the roundings --
a factor of 2 to 3 under the unscaled bound.  (At randn the figures reach 2.9, a scale of 11.5 where 8 is the most a case may take; at
0.1 * randn they reach 0.94, so close to the bound that an evaluation order other than the restatement's lands on either side of
it: the kernels' first run gave 1.21 on (257, 32, 4, indep), a row with lam = 4.4.)"""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import rot_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
TOL = dict(dz=(1e-5, 1e-7), de=(1e-4, 1e-7))                    # (rtol, atol) of tests/test_gpu_rvq.py

# worst error / (atol + rtol |want|) of staged_f32 against float64, special rows of the degenerate case excluded.  Measured on the CPU.
RESTATEMENT = {
    ('degenerate', 16): 0.105, ('indep', 4): 0.34, ('indep', 6): 0.176, ('indep', 8): 0.154, ('indep', 64): 0.194,
    ('indep', 256): 0.213, ('indep', 260): 0.184, ('indep', 1024): 0.18, ('noise0.01', 4): 0.103, ('noise0.01', 6): 0.16,
    ('noise0.01', 8): 0.137, ('noise0.01', 64): 0.0856, ('noise0.01', 256): 0.0871, ('noise0.01', 260): 0.0763, ('noise0.01', 1024): 0.0448,
    ('noise0.1', 4): 0.162, ('noise0.1', 6): 0.158, ('noise0.1', 8): 0.159, ('noise0.1', 64): 0.113, ('noise0.1', 256): 0.0861,
    ('noise0.1', 260): 0.0738, ('noise0.1', 1024): 0.0745, ('noise0.3', 4): 0.158, ('noise0.3', 6): 0.175, ('noise0.3', 8): 0.131,
    ('noise0.3', 64): 0.183, ('noise0.3', 256): 0.114, ('noise0.3', 260): 0.144, ('noise0.3', 1024): 0.144,
}


def bound_scale(kind: str, d: int) -> float:
    """factor on (atol + rtol |want|) of the GPU comparison of dz: 1, or 4 x the restatement's own figure where that exceeds 1"""
    r = RESTATEMENT[(kind, d)]
    return 4.0 * r if r > 1.0 else 1.0


def bf16_round(g: np.ndarray) -> np.ndarray:
    return torch.from_numpy(g).to(torch.bfloat16).float().numpy()


def kept_rows(case) -> np.ndarray:
    keep = np.ones(case[0], bool)
    if case[3] == 'degenerate':
        keep[list(R.SPECIAL_ROWS)] = False
    return keep


def q_conf(qtype='standard', k=64, dim=64, **params):
    base = dict(commitment_cost=0.25)
    if qtype == 'ema':
        base.update(decay=0.95, epsilon=1e-5)
    base.update(params)
    return dict(num_embeddings=k, embedding_dim=dim, reinit_every_n_epochs=None, type=qtype, params=base)


# ---------------------------------------------------------------------------------------------- the reference itself
def _autograd_dz(z, q, g, cz):
    """float64 autograd of the detached formulation: q~ = sg[lam] (z - 2 (z.r) r + 2 (z.zh) qh), L = <g, q~> + cz/2 |z - q|^2"""
    z = torch.from_numpy(z).double().requires_grad_(True)
    q, g = torch.from_numpy(q).double(), torch.from_numpy(g).double()
    with torch.no_grad():
        nz = z.norm(dim=1, keepdim=True).clamp_min(R.EPS_N)
        nq = q.norm(dim=1, keepdim=True).clamp_min(R.EPS_N)
        zh, qh, lam = z / nz, q / nq, nq / nz
        s = zh + qh
        r = s / s.norm(dim=1, keepdim=True).clamp_min(R.EPS_S)
    qt = lam * (z - 2.0 * (z * r).sum(1, keepdim=True) * r + 2.0 * (z * zh).sum(1, keepdim=True) * qh)
    loss = (g * qt).sum() + 0.5 * cz * ((z - q) ** 2).sum()
    loss.backward()
    return z.grad.numpy(), qt.detach().numpy()


@pytest.mark.parametrize('case', [(33, 32, 64, 'noise0.3'), (31, 32, 8, 'indep'), (32, 32, 4, 'noise0.1'), (1, 32, 1024, 'noise0.01'),
                                  (31, 32, 260, 'noise0.3'), (33, 32, 6, 'indep')], ids=str)
def test_reference_equals_autograd_of_the_detached_formulation(case):
    """elementwise RELATIVE, so the cases are small: both sides round at 1e-16 of the terms, and among many thousands of elements one
    cancels to 1e-4 of its terms (the 66,820 elements of (257, 32, 260, noise0.01) reach 1e-11)"""
    z, e, idx, g = R.make_case(*case)
    q, g = e[idx], g / np.float32(R.G_SCALE)                         # (a unit-scale gradient: fewer elements that cancel against the commitment term)
    want, qt = _autograd_dz(z, q, g, R.CZ)
    got = R.dz(z, q, g, R.CZ)
    rel = np.abs(got - want) / np.abs(want)
    print(f'ROTMEASURE {case}: closed form against autograd, worst relative {rel.max():.3e}; q~ - q {np.abs(qt - q).max():.3e}')
    assert rel.max() <= 1e-12
    assert np.abs(R.q_tilde(z, q) - q.astype(np.float64)).max() <= 1e-12 and np.abs(qt - q).max() <= 1e-12


def test_central_difference_of_a_scalar_functional():
    """F(z) = <g, q~(z)> + cz/2 |z - q|^2 with the constants frozen at z0 (the detached formulation): its central difference along
    random directions against <dz, direction>"""
    z, e, idx, g = R.make_case(5, 4, 6, 'noise0.3')
    q = e[idx].astype(np.float64)
    z0, g = z.astype(np.float64), g.astype(np.float64)
    zh, qh, r, lam = R._parts(z0, q)

    def fn(zz):
        qt = lam * (zz - 2.0 * (zz * r).sum(1, keepdims=True) * r + 2.0 * (zz * zh).sum(1, keepdims=True) * qh)
        return (g * qt).sum() + 0.5 * R.CZ * ((zz - q) ** 2).sum()

    grad = R.dz(z0, q, g, R.CZ)
    rng = np.random.default_rng(3)
    for _ in range(4):
        v = rng.standard_normal(z0.shape)
        h = 1e-4
        fd = (fn(z0 + h * v) - fn(z0 - h * v)) / (2.0 * h)
        print(f'ROTMEASURE central difference {fd:.12e} against {float((grad * v).sum()):.12e}')
        np.testing.assert_allclose(fd, (grad * v).sum(), rtol=1e-9, atol=1e-12)


def test_main_cases_stay_away_from_the_antipode():
    worst = 1.0
    for case in R.all_cases():
        z, e, idx, _ = R.make_case(*case)
        worst = min(worst, float(R.cos_zq(z, e[idx])[kept_rows(case)].min()))
    print(f'ROTMEASURE smallest zh.qh over the compared rows: {worst:.4f}')
    assert worst > 0.0


def test_degenerate_rows_are_finite():
    z, e, idx, g = R.make_case(*R.DEGENERATE)
    q = e[idx]
    assert not z[0].any() and not q[1].any() and np.array_equal(z[2], -q[2]) and int((idx == 1).sum()) == 1
    assert len(R.SPECIAL_ROWS) <= 3
    for got in (R.dz(z, q, g, R.CZ), R.staged_f32(z, q, g, R.CZ), R.staged_f32(z, q, g, R.CZ, 'fma'), R.q_tilde(z, q)):
        assert np.isfinite(got).all()
    assert np.abs(R.dz(z, q, g, 0.0)[0]).max() > 1e4                # lam = |q| / 1e-6 on the zero latent


# ---------------------------------------------------------------------------------------------- the fp32 restatement
def test_restatement_error_is_the_recorded_one():
    worst = {key: 0.0 for key in RESTATEMENT}
    for case in R.all_cases():
        n, k, d, kind = case
        z, e, idx, g = R.make_case(*case)
        q, keep = e[idx], kept_rows(case)
        for gg in (g, bf16_round(g)):
            for s in (1.0, R.GS):
                want = R.dz(z, q, gg, R.CZ * s)
                for flavour in ('plain', 'fma'):
                    got = R.staged_f32(z, q, gg, R.CZ * s, flavour).astype(np.float64)
                    assert np.isfinite(got).all()
                    rtol, atol = TOL['dz']
                    worst[(kind, d)] = max(worst[(kind, d)], float((np.abs(got - want) / (atol + rtol * np.abs(want)))[keep].max()))
    for key, value in sorted(worst.items()):
        print(f'ROTMEASURE restatement {key}: {value:.4g} (recorded {RESTATEMENT[key]}), bound scale {bound_scale(*key):.3g}')
        # the table is no understatement of what this loop measures (the host's summation order may move the worst element)
        assert value <= 2.0 * RESTATEMENT[key]
        assert bound_scale(*key) <= 8.0
    assert max(worst.values()) <= 0.5 and all(bound_scale(*key) == 1.0 for key in RESTATEMENT)         # the inputs need no scaling
    assert {(c[3], c[2]) for c in R.all_cases()} == set(RESTATEMENT)


# ---------------------------------------------------------------------------------------------- module and config on the CPU
def test_config_key_and_validation():
    model_mod = importlib.import_module(PKG + '.model')
    vqm = importlib.import_module(PKG + '.modules.vector_quantizers')
    train = importlib.import_module(PKG + '.train')
    for qtype in ('standard', 'ema'):
        assert model_mod.VQVAE(32, AE, q_conf(qtype), None, TC).quantizer.rotate is False          # an absent key: today's estimator
        assert model_mod.VQVAE(32, AE, q_conf(qtype, gradient='straight_through'), None, TC).quantizer.rotate is False
        m = model_mod.VQVAE(32, AE, q_conf(qtype, gradient='rotation'), None, TC)
        assert m.quantizer.rotate is True and m.quantizer.gradient == 'rotation'
        plain = model_mod.VQVAE(32, AE, q_conf(qtype), None, TC)
        assert list(m.state_dict()) == list(plain.state_dict())                                       # no checkpoint key
        plain.load_state_dict(m.state_dict(), strict=True)
        with pytest.raises(ValueError, match='quantizer.params.gradient'):
            model_mod.VQVAE(32, AE, q_conf(qtype, gradient='rotate'), None, TC)
    with pytest.raises(ValueError, match='quantizer.params.gradient'):
        vqm.VectorQuantizer(64, 64, 0.25, gradient='ste')
    with pytest.raises(ValueError, match='quantizer.params.gradient'):
        vqm.EMAVectorQuantizer(64, 64, gradient=None)
    others = {'entropy': dict(ent_loss_ratio=0.1, ent_temperature=0.01, ent_loss_type='softmax'),
              'gumbel': dict(straight_through=False, temp=1.0, kl_cost=5e-4), 'fsq': dict(levels=[4, 4, 4]), 'lfq': dict(bits=6),
              'residual': dict(depth=2), 'cosine': {}}
    for qtype, params in others.items():
        for value in ('rotation', 'straight_through'):
            with pytest.raises(ValueError, match="quantizer.params.gradient.*'standard' and 'ema' quantizers only"):
                model_mod.VQVAE(32, AE, q_conf(qtype, gradient=value, **params), None, TC)
        model_mod.VQVAE(32, AE, q_conf(qtype, **params), None, TC)                                    # ... and builds without the key
    conf = train.get_model_conf(os.path.join(ROOT, 'example_confs', 'rotation_vqvae.yaml'))
    ema = train.get_model_conf(os.path.join(ROOT, 'example_confs', 'ema_vqvae.yaml'))
    assert conf['quantizer']['params'].pop('gradient') == 'rotation' and conf == ema                  # the EMA config plus the switch
    run = train.derive_run_config(train.get_model_conf(os.path.join(ROOT, 'example_confs', 'rotation_vqvae.yaml')), 8,
                                  {'autoencoder.channels': 32, 'quantizer.num_embeddings': 64})
    m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'])
    assert type(m.quantizer).__name__ == 'EMAVectorQuantizer' and m.quantizer.rotate is True


def test_lookup_takes_the_mode_as_a_trailing_argument():
    import inspect
    ops = importlib.import_module(PKG + '.ops')
    native = importlib.import_module(PKG + '._native')
    sig = inspect.signature(ops.VQLookupFn.forward)
    assert list(sig.parameters)[-1] == 'rotate' and sig.parameters['rotate'].default is False and len(sig.parameters) == 8
    assert native._PROTOS['vqk_vq_backward_rot_f32'] == native._PROTOS['vqk_vq_backward_f32']
    lib = native.lib()
    buf = 0x10000                                                   # never dereferenced: every call below returns before a launch
    rot = lambda **o: lib.vqk_vq_backward_rot_f32(o.get('z', buf), buf, buf, buf, o.get('dt', 0), o.get('n', 8), 4, o.get('d', 16), 0.1, 0.2,
                                                  None, o.get('dz', buf), None, None)
    assert rot(n=0) == 0                                            # nothing to do: success, no launch
    assert rot(z=None) == -5 and rot(dz=None) == -5 and rot(d=0) == -1 and rot(d=1028) == -1 and rot(n=-1) == -1 and rot(dt=7) == -2
