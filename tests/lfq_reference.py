"""The lookup-free quantizer (Yu et al., "Language Model Beats Diffusion", 2023; Open-MAGVIT2) as the specification states it, in
numpy, dtype-parametrised: float64 is the reference of the LFQ tests, float32 the yardstick a device error is measured with
(``distance``).  H_batch is computed the EXPLICIT way -- a softmax over the 2^g_s sign codes of every group -- and so is its gradient
(through the softmax's Jacobian): an independent formulation of what the kernels compute as products of per-bit sigmoids.  Also the
token <-> bit arithmetic, the implicit codebook, and the input generator that keeps every kept row away from a sign boundary."""
import numpy as np

EPS = 1e-10


def codes(bits, dtype=np.float64):
    """[2^bits, bits]: row m, column j = +1 if bit j of m is set, else -1 (the implicit codebook; first channel = bit 0)"""
    m = np.arange(1 << bits, dtype=np.int64)
    return (((m[:, None] >> np.arange(bits)) & 1) * 2 - 1).astype(dtype)


def codes_to_indices(c):
    """c [..., d] of +-1 -> tokens [...]"""
    c = np.asarray(c)
    return ((c > 0).astype(np.int64) << np.arange(c.shape[-1])).sum(-1)


def indices_to_codes(idx, bits, dtype=np.float64):
    """tokens [...] -> +-1 vectors [..., bits]"""
    return (((np.asarray(idx, dtype=np.int64)[..., None] >> np.arange(bits)) & 1) * 2 - 1).astype(dtype)


def groups(bits, g):
    """the consecutive bit groups [(first bit, number of bits)]: ceil(bits / g) of them, the last may be shorter"""
    return [(s, min(g, bits - s)) for s in range(0, bits, g)]


def _softmax(logits):
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def h_sample_explicit(u, tau):
    """(1/N) sum_n of the entropy of softmax(2 u_n . c_k / tau) over ALL 2^d sign codes (d <= 10 or so): what the d binary
    entropies of the specification factorise"""
    u = np.asarray(u)
    p = _softmax((2.0 / tau) * (u @ codes(u.shape[1], u.dtype).T))
    return float(-(p * np.log(np.maximum(p, 1e-300))).sum() / u.shape[0])


def forward(z, w_in, b_in, w_out, b_out, g, tau, beta=0.25, ratio=0.1, gamma=1.0, dtype=np.float64):
    """steps 1-8 of the specification; every array is cast to ``dtype`` first and every operation runs in it"""
    z, w_in, b_in, w_out, b_out = (np.asarray(a).astype(dtype) for a in (z, w_in, b_in, w_out, b_out))
    n, d = z.shape[0], w_in.shape[0]
    a = dtype(4.0) / dtype(tau)
    u = z @ w_in.T + b_in
    c = np.where(u > 0, dtype(1), dtype(-1))
    idx = codes_to_indices(c)
    q = c @ w_out.T + b_out
    commit = ((u - c) ** 2).sum(dtype=dtype) / dtype(n * d)
    x = a * u
    ax = np.abs(x)
    e = np.exp(-ax)
    small, big = e / (1 + e), 1 / (1 + e)                    # sigmoid(-|x|), sigmoid(|x|)
    p, pm = np.where(x >= 0, big, small), np.where(x >= 0, small, big)
    h_sample = (np.log1p(e) + ax * small).sum(dtype=dtype) / dtype(n)
    h_batch, soft, pbar = dtype(0), [], []
    for s, gs in groups(d, g):
        ps = _softmax((dtype(2.0) / dtype(tau)) * (u[:, s:s + gs] @ codes(gs, dtype).T))         # [N, 2^gs], explicit
        pb = ps.sum(0, dtype=dtype) / dtype(n)
        h_batch = h_batch - (pb * np.log(pb + dtype(EPS))).sum(dtype=dtype)
        soft.append(ps)
        pbar.append(pb)
    loss = dtype(beta) * commit + dtype(ratio) * (h_sample - dtype(gamma) * h_batch)
    return dict(u=u, c=c, idx=idx, q=q, p=p, pm=pm, commit=commit, h_sample=h_sample, h_batch=h_batch, loss=loss, soft=soft, pbar=pbar)


def backward(z, w_in, b_in, w_out, b_out, dq, gloss, g, tau, beta=0.25, ratio=0.1, gamma=1.0, dtype=np.float64):
    """step 9: straight-through from dq at u plus gloss * dloss/du (closed forms; H_batch through the explicit softmax's Jacobian):
    dz and the four parameter gradients"""
    f = forward(z, w_in, b_in, w_out, b_out, g, tau, beta, ratio, gamma, dtype)
    z, w_in, w_out, dq = (np.asarray(a).astype(dtype) for a in (z, w_in, w_out, dq))
    n, d = z.shape[0], w_in.shape[0]
    a = dtype(4.0) / dtype(tau)
    u = f['u']
    d_commit = dtype(2) * (u - f['c']) / dtype(n * d)
    d_hs = -(a * a) * u * f['p'] * f['pm'] / dtype(n)
    d_hb = np.zeros_like(u)
    for (s, gs), ps, pb in zip(groups(d, g), f['soft'], f['pbar']):
        lm = np.log(pb + dtype(EPS)) + pb / (pb + dtype(EPS))                                  # -dH_batch / dPbar
        lp = ps * lm
        dlogit = -(lp - ps * lp.sum(-1, keepdims=True)) / dtype(n)                              # softmax Jacobian applied to -L / N
        d_hb[:, s:s + gs] = (dtype(2.0) / dtype(tau)) * (dlogit @ codes(gs, dtype))
    du = dq @ w_out + dtype(gloss) * (dtype(beta) * d_commit + dtype(ratio) * (d_hs - dtype(gamma) * d_hb))
    return dict(dz=du @ w_in, dw_in=du.T @ z, db_in=du.sum(0), dw_out=dq.T @ f['c'], db_out=dq.sum(0))


def make_inputs(seed, n, d_model, bits, margin=1e-3):
    """z ~ N(0,1) [n, D], W_in ~ U(-1,1) * 2 / sqrt(D), b_in ~ U(-.5,.5), W_out ~ U(-1,1) [D, d], b_out ~ U(-.5,.5), dq ~ N(0,1), all
    float32-exact float64 arrays.  Every row in which some |u_j| < ``margin`` (float64, on the CPU) is drawn again until none is
    left: no kept row sits on a sign boundary.  ``resampled`` = the share of rows redrawn at least once."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    w_in = f32(rng.uniform(-1, 1, (bits, d_model)) * 2 / np.sqrt(d_model))
    b_in = f32(rng.uniform(-.5, .5, bits))
    w_out = f32(rng.uniform(-1, 1, (d_model, bits)))
    b_out = f32(rng.uniform(-.5, .5, d_model))
    dq = f32(rng.standard_normal((n, d_model)))
    z = f32(rng.standard_normal((n, d_model)))
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(100):
        bad = np.abs(z @ w_in.T + b_in).min(-1) < margin
        if not bad.any():
            break
        redrawn |= bad
        z[bad] = f32(rng.standard_normal((int(bad.sum()), d_model)))
    else:
        raise RuntimeError('lfq_reference.make_inputs: rows still on a sign boundary after 100 draws')
    return dict(z=z, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, dq=dq, resampled=float(redrawn.mean()))


def distance(got, want):
    """max-abs error over max-abs of the reference: the metric of the LFQ tests"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))
