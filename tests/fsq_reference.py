"""The finite scalar quantizer (Mentzer et al., "Finite Scalar Quantization: VQ-VAE Made Simple", 2023) as the specification states
it, in numpy, dtype-parametrised: float64 is the reference of the FSQ tests, float32 the yardstick a device error is measured with
(``distance``).  Also the mixed-radix token arithmetic, the implicit codebook, and the input generator that keeps every kept row away
from a rounding boundary."""
import numpy as np

EPS = 1e-3


def consts(levels, dtype=np.float64):
    """per channel: half_l, offset, shift (computed in float64, then cast: what a float32 implementation holds), half_width, basis"""
    lv = np.asarray(levels, dtype=np.int64)
    half_l = (lv - 1) * (1.0 + EPS) / 2.0
    offset = np.where(lv % 2 == 0, 0.5, 0.0)
    shift = np.arctanh(offset / half_l)
    half_width = lv // 2
    basis = np.concatenate([[1], np.cumprod(lv[:-1])]).astype(np.int64)
    return half_l.astype(dtype), offset.astype(dtype), shift.astype(dtype), half_width, basis


def codes_to_indices(r, levels):
    """r [..., d] integer-valued rounded vectors (centred: -L//2 .. ) -> tokens [...]"""
    _, _, _, half_width, basis = consts(levels)
    return ((np.rint(r).astype(np.int64) + half_width) * basis).sum(-1)


def indices_to_codes(idx, levels):
    """tokens [...] -> centred integer digits [..., d] (int64)"""
    lv = np.asarray(levels, dtype=np.int64)
    _, _, _, half_width, basis = consts(levels)
    return (np.asarray(idx, dtype=np.int64)[..., None] // basis) % lv - half_width


def implicit_codebook(levels, dtype=np.float64):
    """[K, d]: row i = the c vector (digits / half_width) of token i"""
    k = int(np.prod(np.asarray(levels, dtype=np.int64)))
    _, _, _, half_width, _ = consts(levels)
    return indices_to_codes(np.arange(k), levels).astype(dtype) / half_width.astype(dtype)


def forward(z, w_in, b_in, w_out, b_out, levels, dtype=np.float64):
    """steps 1-6 of the specification; every array is cast to ``dtype`` first and every operation runs in it"""
    z, w_in, b_in, w_out, b_out = (np.asarray(a).astype(dtype) for a in (z, w_in, b_in, w_out, b_out))
    half_l, offset, shift, half_width, _ = consts(levels, dtype)
    u = z @ w_in.T + b_in
    t = np.tanh(u + shift)
    bounded = t * half_l - offset
    r = np.rint(bounded)                                     # ties to even
    c = r / half_width.astype(dtype)
    idx = codes_to_indices(r, levels)
    q = c @ w_out.T + b_out
    return dict(u=u, t=t, bounded=bounded, r=r, c=c, idx=idx, q=q)


def backward(z, w_in, b_in, w_out, b_out, dq, levels, dtype=np.float64):
    """step 7 (straight-through, closed form): dz and the four parameter gradients"""
    f = forward(z, w_in, b_in, w_out, b_out, levels, dtype)
    z, w_in, w_out, dq = (np.asarray(a).astype(dtype) for a in (z, w_in, w_out, dq))
    half_l, _, _, half_width, _ = consts(levels, dtype)
    g = dq @ w_out
    du = g / half_width.astype(dtype) * half_l * (1 - f['t'] * f['t'])
    return dict(dz=du @ w_in, dw_in=du.T @ z, db_in=du.sum(0), dw_out=dq.T @ f['c'], db_out=dq.sum(0))


def boundary_distance(bounded):
    """per row: the smallest distance of a bounded_j to a half-integer (where rint changes its value)"""
    frac = bounded - np.floor(bounded)
    return np.abs(frac - 0.5).min(-1)


def make_inputs(seed, n, d_model, levels, margin=1e-3):
    """z ~ N(0,1) [n, D], W_in ~ U(-1,1) * 2 / sqrt(D), b_in ~ U(-.5,.5), W_out ~ U(-1,1) [D, d], b_out ~ U(-.5,.5), dq ~ N(0,1), all
    float32-exact float64 arrays.  Every row in which some bounded_j lies within ``margin`` of a half-integer (float64, on the CPU) is
    drawn again until none is left: no kept row sits on a rounding boundary.  ``resampled`` = the share of rows redrawn at least once."""
    rng = np.random.default_rng(seed)
    d = len(levels)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    w_in = f32(rng.uniform(-1, 1, (d, d_model)) * 2 / np.sqrt(d_model))
    b_in = f32(rng.uniform(-.5, .5, d))
    w_out = f32(rng.uniform(-1, 1, (d_model, d)))
    b_out = f32(rng.uniform(-.5, .5, d_model))
    dq = f32(rng.standard_normal((n, d_model)))
    z = f32(rng.standard_normal((n, d_model)))
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(100):
        bad = boundary_distance(forward(z, w_in, b_in, w_out, b_out, levels)['bounded']) < margin
        if not bad.any():
            break
        redrawn |= bad
        z[bad] = f32(rng.standard_normal((int(bad.sum()), d_model)))
    else:
        raise RuntimeError('fsq_reference.make_inputs: rows still on a rounding boundary after 100 draws')
    return dict(z=z, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, dq=dq, resampled=float(redrawn.mean()))


def distance(got, want):
    """max-abs error over max-abs of the reference: the metric of the FSQ tests"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))
