"""The binary spherical quantizer (Zhao, Xiong, Kraehenbuehl, "Image and Video Tokenization with Binary Spherical Quantization", 2024) as
the specification states it, in numpy, dtype-parametrised: float64 is the reference of the BSQ tests, float32 the yardstick a device
error is measured with (``distance``).  It is the lookup-free quantizer of tests/lfq_reference.py with the projected latent put on the
unit sphere before the sign is taken: v = W_in z + b_in, u = v / max(|v|, 1e-12), c = +-1 / sqrt(d).  H_batch is computed the EXPLICIT
way -- a softmax of the distance logits over the 2^g_s codes of every group -- and so is its gradient (through the softmax's Jacobian):
an independent formulation of what the kernels compute as products of per-bit sigmoids.  The token <-> bit arithmetic, the group split,
the input generator (no kept row has a |v_j| < 1e-3) and the metric are lfq_reference's."""
import numpy as np

from tests.lfq_reference import codes, distance, groups, make_inputs  # noqa: F401  (re-exported: the tests use them through this module)

EPS = 1e-10
NORM_EPS = 1e-12


def scale(bits, dtype=np.float64):
    """s = 1 / sqrt(bits): the magnitude of every code channel, |c| = 1"""
    return dtype(1) / np.sqrt(dtype(bits))


def sphere_codes(bits, dtype=np.float64):
    """[2^bits, bits]: the implicit codebook, row m = the +-s vector of token m (first channel = bit 0)"""
    return codes(bits, dtype) * scale(bits, dtype)


def codes_to_indices(c):
    """c [..., d] of +-s -> tokens [...]"""
    c = np.asarray(c)
    return ((c > 0).astype(np.int64) << np.arange(c.shape[-1])).sum(-1)


def indices_to_codes(idx, bits, dtype=np.float64):
    """tokens [...] (any int64: masked to ``bits`` bits) -> +-s vectors [..., bits]"""
    sign = (((np.asarray(idx, dtype=np.int64)[..., None] >> np.arange(bits)) & 1) * 2 - 1).astype(dtype)
    return sign * scale(bits, dtype)


def _softmax(logits):
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def h_sample_explicit(u, tau):
    """(1/N) sum_n of the entropy of softmax(-|u_n - c_k|^2 / tau) over ALL 2^d codes (d <= 10 or so): what the d binary entropies of
    the specification factorise"""
    u = np.asarray(u)
    ck = sphere_codes(u.shape[1], u.dtype.type)
    p = _softmax(-((u[:, None, :] - ck[None]) ** 2).sum(-1) / tau)
    return float(-(p * np.log(np.maximum(p, 1e-300))).sum() / u.shape[0])


def forward(z, w_in, b_in, w_out, b_out, g, tau, beta=0.25, ratio=0.1, gamma=1.0, dtype=np.float64):
    """steps 1-5 of the specification; every array is cast to ``dtype`` first and every operation runs in it"""
    z, w_in, b_in, w_out, b_out = (np.asarray(a).astype(dtype) for a in (z, w_in, b_in, w_out, b_out))
    n, d = z.shape[0], w_in.shape[0]
    s = scale(d, dtype)
    a = dtype(4.0) * s / dtype(tau)
    v = z @ w_in.T + b_in
    r = dtype(1) / np.maximum(np.sqrt((v * v).sum(-1, dtype=dtype)), dtype(NORM_EPS))
    u = v * r[:, None]
    c = np.where(v > 0, s, -s).astype(dtype)
    idx = codes_to_indices(c)
    q = c @ w_out.T + b_out
    commit = ((u - c) ** 2).sum(dtype=dtype) / dtype(n)
    x = a * u
    ax = np.abs(x)
    e = np.exp(-ax)
    small, big = e / (1 + e), 1 / (1 + e)                    # sigmoid(-|x|), sigmoid(|x|)
    p, pm = np.where(x >= 0, big, small), np.where(x >= 0, small, big)
    h_sample = (np.log1p(e) + ax * small).sum(dtype=dtype) / dtype(n)
    h_batch, soft, pbar = dtype(0), [], []
    for b0, gs in groups(d, g):
        # the distance logits -|u - c_k|^2 / tau restricted to the group's channels, up to a per-row constant: (2 s / tau) u . sign_k
        ps = _softmax((dtype(2.0) * s / dtype(tau)) * (u[:, b0:b0 + gs] @ codes(gs, dtype).T))        # [N, 2^gs], explicit
        pb = ps.sum(0, dtype=dtype) / dtype(n)
        h_batch = h_batch - (pb * np.log(pb + dtype(EPS))).sum(dtype=dtype)
        soft.append(ps)
        pbar.append(pb)
    loss = dtype(beta) * commit + dtype(ratio) * (h_sample - dtype(gamma) * h_batch)
    return dict(v=v, r=r, u=u, c=c, idx=idx, q=q, p=p, pm=pm, commit=commit, h_sample=h_sample, h_batch=h_batch, loss=loss, soft=soft,
                pbar=pbar)


def backward(z, w_in, b_in, w_out, b_out, dq, gloss, g, tau, beta=0.25, ratio=0.1, gamma=1.0, dtype=np.float64):
    """step 6: straight-through from dq at u plus gloss * dloss/du (closed forms; H_batch through the explicit softmax's Jacobian), then
    through the normalisation: dz and the four parameter gradients (and e, dv for the property tests)"""
    f = forward(z, w_in, b_in, w_out, b_out, g, tau, beta, ratio, gamma, dtype)
    z, w_in, w_out, dq = (np.asarray(a).astype(dtype) for a in (z, w_in, w_out, dq))
    n, d = z.shape[0], w_in.shape[0]
    s = scale(d, dtype)
    a = dtype(4.0) * s / dtype(tau)
    u = f['u']
    d_commit = dtype(2) * (u - f['c']) / dtype(n)
    d_hs = -(a * a) * u * f['p'] * f['pm'] / dtype(n)
    d_hb = np.zeros_like(u)
    for (b0, gs), ps, pb in zip(groups(d, g), f['soft'], f['pbar']):
        lm = np.log(pb + dtype(EPS)) + pb / (pb + dtype(EPS))                                  # -dH_batch / dPbar
        lp = ps * lm
        dlogit = -(lp - ps * lp.sum(-1, keepdims=True)) / dtype(n)                              # softmax Jacobian applied to -L / N
        d_hb[:, b0:b0 + gs] = (dtype(2.0) * s / dtype(tau)) * (dlogit @ codes(gs, dtype))
    e = dq @ w_out + dtype(gloss) * (dtype(beta) * d_commit + dtype(ratio) * (d_hs - dtype(gamma) * d_hb))
    dv = (e - u * (u * e).sum(-1, keepdims=True, dtype=dtype)) * f['r'][:, None]
    return dict(dz=dv @ w_in, dw_in=dv.T @ z, db_in=dv.sum(0), dw_out=dq.T @ f['c'], db_out=dq.sum(0), e=e, dv=dv)


def decode(idx, w_out, b_out, dtype=np.float64):
    """step 7: tokens -> q through the codes of their low ``bits`` bits"""
    w_out, b_out = np.asarray(w_out).astype(dtype), np.asarray(b_out).astype(dtype)
    return indices_to_codes(idx, w_out.shape[1], dtype) @ w_out.T + b_out
