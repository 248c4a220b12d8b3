"""The two softmax-based quantizers -- the Entropy (MaskGIT-style) quantizer and the Gumbel-softmax quantizer -- as their
specification states them, in numpy, dtype-parametrised: float64 is the reference of the tests, float32 the yardstick a device error is
measured with (``distance``).  No autograd: every gradient is written out, and written ANOTHER way than the kernels write it -- as the
softmax's Jacobian applied to the loss's gradient with respect to the probabilities, where csrc/entropy.hip uses the closed forms of
its header.  tests/test_entropy_cpu.py holds these formulas against torch's float64 autograd of the oracle and against finite
differences.

Entropy quantizer, on a distance matrix d [N, K] at temperature T:  a = -d / T, p = softmax_k(a), h_i = lse_i - sum_k p_ik a_ik,
pbar_k = mean_i p_ik, u_k = log(pbar_k + 1e-5) + pbar_k / (pbar_k + 1e-5), L = ratio (mean_i h_i + sum_k pbar_k log(pbar_k + 1e-5)).
'argmax': the targets are one_hot(argmin d) with the gradient of p (pbar becomes hist / N, the sample term lse_i + d[i, c_i] / T).

Gumbel quantizer, on logits [N, K] and Exp(1) noise: t = (logits - log noise) / tau, y = softmax_k(t), idx = first maximum of t,
qy = softmax_k(logits), kl_i = sum_k qy log(qy K + 1e-10).

The scalars the device accumulates with fp32 atomics (hsum, ssum, klsum, avg_term, each psum[k]) are added SEQUENTIALLY in the float32
evaluation (a cumulative sum), not with numpy's pairwise ``sum``: the yardstick then carries the error of a plain fp32 running sum."""
import numpy as np

EPS_ENT = 1e-5
EPS_KL = 1e-10
NOISE_MIN, NOISE_MAX = 1e-30, 1e4
MARGIN = 1e-4
ROUNDS = 20


def distance(got, want):
    """max-abs error over max-abs of the reference (the metric of the LFQ tests)"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def seq_sum(x, dtype, axis=0):
    """sum along ``axis`` in ``dtype``: a running sum in float32 (what an fp32 accumulator does), numpy's sum in float64"""
    x = np.asarray(x).astype(dtype)
    if dtype == np.float32:
        return np.take(np.cumsum(x, axis=axis, dtype=np.float32), -1, axis=axis)
    return x.sum(axis=axis, dtype=dtype)


def bf16(a):
    """round to nearest even to bfloat16, returned as float64 (finite values)"""
    x = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
    r = ((x >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((x + r) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)


def bf16_ulp(v):
    """spacing of bfloat16 (8 significant bits) at |v|, elementwise; the smallest normal's below it"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _softmax_parts(a):
    """(lse [N], p [N, K], log p [N, K]) of the rows of a"""
    m = a.max(-1, keepdims=True)
    s = np.exp(a - m).sum(-1, keepdims=True, dtype=a.dtype)
    lse = m + np.log(s)
    lp = a - lse
    return lse[:, 0], np.exp(lp), lp


# ----------------------------------------------------------------------------------------------------------------------------------
# Entropy quantizer
# ----------------------------------------------------------------------------------------------------------------------------------
def entropy_rows(dmat, T, dtype=np.float64):
    """-> lse [N], hrow [N], sum_i hrow"""
    a = -np.asarray(dmat).astype(dtype) / dtype(T)
    lse, p, _ = _softmax_parts(a)
    hrow = lse - (p * a).sum(-1, dtype=dtype)
    return lse, hrow, seq_sum(hrow, dtype)


def _u_of(pbar, dtype):
    return np.log(pbar + dtype(EPS_ENT)) + pbar / (pbar + dtype(EPS_ENT))


def entropy_cols(dmat, T, dtype=np.float64):
    """-> psum [K] (sum_i p_ik), u [K], avg_term = sum_k pbar_k log(pbar_k + 1e-5)"""
    d = np.asarray(dmat).astype(dtype)
    _, p, _ = _softmax_parts(-d / dtype(T))
    psum = seq_sum(p, dtype, axis=0)
    pbar = psum / dtype(d.shape[0])
    return psum, _u_of(pbar, dtype), seq_sum(pbar * np.log(pbar + dtype(EPS_ENT)), dtype)


def entropy_argmax_forward(dmat, idx, hist, T, dtype=np.float64):
    """-> lse, hrow, hsum, ssum = sum_i (lse_i + d[i, idx_i] / T), m = hist as floats, u (from hist / N), avg_term"""
    d = np.asarray(dmat).astype(dtype)
    n = d.shape[0]
    lse, hrow, hsum = entropy_rows(d, T, dtype)
    ssum = seq_sum(lse + d[np.arange(n), np.asarray(idx)] / dtype(T), dtype)
    m = np.asarray(hist).astype(dtype)
    pbar = m / dtype(n)
    return lse, hrow, hsum, ssum, m, _u_of(pbar, dtype), seq_sum(pbar * np.log(pbar + dtype(EPS_ENT)), dtype)


def entropy_dd(dmat, T, ratio, gs, loss_type, idx=None, dtype=np.float64):
    """cotangent of the distance matrix for the loss cotangent ``gs``.  With G = N dL/d(target probabilities) -- -(log p + 1) + u for
    'softmax', -log p + u for 'argmax' (the targets carry p's gradient) -- dL/da = p (G - sum_k p G) / N, for 'argmax' minus
    (one_hot - p) / N, the path through log p itself; dd = -dL/da / T.  Every row sums to zero in both forms (sum_k p (G - sum p G) = 0,
    sum_k (one_hot - p) = 0)."""
    d = np.asarray(dmat).astype(dtype)
    n, k = d.shape
    _, p, lp = _softmax_parts(-d / dtype(T))
    if loss_type == 'softmax':
        u = _u_of(p.sum(0, dtype=dtype) / dtype(n), dtype)
        g = -(lp + dtype(1)) + u
        da = p * (g - (p * g).sum(-1, keepdims=True, dtype=dtype))
    elif loss_type == 'argmax':
        idx = np.asarray(idx)
        u = _u_of(np.bincount(idx, minlength=k).astype(dtype) / dtype(n), dtype)
        g = -lp + u
        one_hot = np.zeros((n, k), dtype=dtype)
        one_hot[np.arange(n), idx] = 1
        da = p * (g - (p * g).sum(-1, keepdims=True, dtype=dtype)) - (one_hot - p)
    else:
        raise ValueError(loss_type)
    return da * (-(dtype(gs) * dtype(ratio)) / (dtype(n) * dtype(T)))


def split_emulation(dd, E, Z):
    """float64 value of the split products  hi E_hi + hi E_lo + lo E_hi  [N, D] and  hi^T Z_hi + hi^T Z_lo + lo^T Z_hi  [K, D], with
    x_hi = bf16(x), x_lo = bf16(x - x_hi): the scheme's own truncation (the dropped lo x lo products and the 16 kept bits of each
    operand), not the device's rounding"""
    def split(x):
        x = np.asarray(x, dtype=np.float32).astype(np.float64)
        hi = bf16(x)
        return hi, bf16(x - hi)
    hi, lo = split(dd)
    e_hi, e_lo = split(E)
    z_hi, z_lo = split(Z)
    return hi @ e_hi + hi @ e_lo + lo @ e_hi, hi.T @ z_hi + hi.T @ z_lo + lo.T @ z_hi


def entropy_distances(z, E, dtype=np.float64):
    """(|z|^2 - 2 z.e) + |e|^2, the association of the specification"""
    z, E = np.asarray(z).astype(dtype), np.asarray(E).astype(dtype)
    return ((z * z).sum(-1, keepdims=True, dtype=dtype) - dtype(2) * (z @ E.T)) + (E * E).sum(-1, dtype=dtype)


def entropy_vq(z, E, beta, ratio, T, loss_type, dq, gloss, dtype=np.float64, split=False):
    """the Entropy quantizer on rows z [N, D] and the codebook E [K, D]: q = E[argmin d] (first minimum), loss = beta mse + mse +
    ratio * entropy term, and the gradients for the cotangents ``dq`` (straight-through; None: absent) and ``gloss`` (None: absent).
    ``split``: the two products of dd are those of ``split_emulation`` and dd's column sums those of hi + lo."""
    z, E = np.asarray(z).astype(dtype), np.asarray(E).astype(dtype)
    n, dim = z.shape
    k = E.shape[0]
    d = entropy_distances(z, E, dtype)
    idx = d.argmin(-1)
    hist = np.bincount(idx, minlength=k)
    q = E[idx]
    mse = seq_sum(((q - z) ** 2).reshape(-1), dtype) / dtype(n * dim)
    if loss_type == 'softmax':
        ent = entropy_rows(d, T, dtype)[2] / dtype(n) + entropy_cols(d, T, dtype)[2]
    else:
        f = entropy_argmax_forward(d, idx, hist, T, dtype)
        ent = f[3] / dtype(n) + f[6]
    loss = dtype(beta) * mse + mse + dtype(ratio) * ent
    dz = np.zeros_like(z) if dq is None else np.asarray(dq).astype(dtype).copy()
    dE = np.zeros_like(E)
    if gloss is not None:
        g = dtype(gloss) * dtype(2) / dtype(n * dim)
        dz += dtype(beta) * g * (z - q)
        np.add.at(dE, idx, g * (q - z))
        dd = entropy_dd(d, T, ratio, gloss, loss_type, idx, dtype)
        if split:
            pe, pz = split_emulation(dd, E, z)
            hi = bf16(dd)
            cs = (hi + bf16(np.asarray(dd, dtype=np.float32).astype(np.float64) - hi)).sum(0)
            rs = dd.sum(-1, keepdims=True)
        else:
            pe, pz, cs, rs = dd @ E, dd.T @ z, dd.sum(0, dtype=dtype), dd.sum(-1, keepdims=True, dtype=dtype)
        dz += dtype(2) * z * rs - dtype(2) * pe                   # d = |z|^2 - 2 z.e + |e|^2 ; the row sums vanish analytically
        dE += dtype(2) * E * cs[:, None] - dtype(2) * pz
    return dict(d=d, q=q, idx=idx, hist=hist, loss=loss, dz=dz, dE=dE)


# ----------------------------------------------------------------------------------------------------------------------------------
# Gumbel quantizer
# ----------------------------------------------------------------------------------------------------------------------------------
def gumbel_t(logits, noise, tau, dtype=np.float64):
    return (np.asarray(logits).astype(dtype) - np.log(np.asarray(noise).astype(dtype))) / dtype(tau)


def gumbel_rows(logits, noise, tau, hard, dtype=np.float64):
    """-> y [N, K] (one-hot with ``hard``), idx [N] (first maximum of t), klsum = sum_i kl_i, hist [K]"""
    logits = np.asarray(logits).astype(dtype)
    n, k = logits.shape
    t = gumbel_t(logits, noise, tau, dtype)
    idx = t.argmax(-1)
    _, y, _ = _softmax_parts(t)
    if hard:
        y = np.zeros_like(y)
        y[np.arange(n), idx] = 1
    _, qy, _ = _softmax_parts(logits)
    kl = (qy * np.log(qy * dtype(k) + dtype(EPS_KL))).sum(-1, dtype=dtype)
    return y, idx, seq_sum(kl, dtype), np.bincount(idx, minlength=k)


def gumbel_rows_backward(logits, noise, dy, tau, klc_over_m, dtype=np.float64):
    """dlogits for the cotangent dy of the SOFT y and ``klc_over_m`` times the cotangent of sum_i kl_i"""
    logits, dy = np.asarray(logits).astype(dtype), np.asarray(dy).astype(dtype)
    k = logits.shape[1]
    _, y, _ = _softmax_parts(gumbel_t(logits, noise, tau, dtype))
    _, qy, _ = _softmax_parts(logits)
    qk = qy * dtype(k)
    g = np.log(qk + dtype(EPS_KL)) + qk / (qk + dtype(EPS_KL))          # d kl_i / d qy
    return (y * (dy - (y * dy).sum(-1, keepdims=True, dtype=dtype)) / dtype(tau)
            + dtype(klc_over_m) * qy * (g - (qy * g).sum(-1, keepdims=True, dtype=dtype)))


def gumbel_vq(logits, E, noise, tau, kl_cost, hard, dq, gkl, dtype=np.float64, round_y=None):
    """q = y E, kl = kl_cost mean_i kl_i and the gradients for the cotangents ``dq`` (None: zero) and ``gkl`` (None: absent).  With
    ``hard`` dE uses the one-hot y and dlogits the soft y (straight-through).  ``round_y``: applied to y and to dy = dq E^T (the
    storage format of the two matrices in a bf16 model)."""
    logits, E = np.asarray(logits).astype(dtype), np.asarray(E).astype(dtype)
    n, k = logits.shape
    y, idx, klsum, hist = gumbel_rows(logits, noise, tau, hard, dtype)
    if round_y is not None:
        y = round_y(y).astype(dtype)
    q = y @ E
    kl = dtype(kl_cost) * klsum / dtype(n)
    dq = np.zeros((n, E.shape[1]), dtype=dtype) if dq is None else np.asarray(dq).astype(dtype)
    dy = dq @ E.T
    if round_y is not None:
        dy = round_y(dy).astype(dtype)
    klc = dtype(0) if gkl is None else dtype(gkl) * dtype(kl_cost) / dtype(n)
    return dict(y=y, q=q, idx=idx, hist=hist, kl=kl, dy=dy, dlogits=gumbel_rows_backward(logits, noise, dy, tau, klc, dtype), dE=y.T @ dq)


# ----------------------------------------------------------------------------------------------------------------------------------
# input makers: a seed per case, no row left out, one planted exact tie
# ----------------------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _gap_ok(t, largest):
    """rows whose best and second-best of t (largest or smallest first) are at least MARGIN max(1, max|t|) apart"""
    s = np.sort(t, axis=-1)
    gap = (s[:, -1] - s[:, -2]) if largest else (s[:, 1] - s[:, 0])
    return gap >= MARGIN * np.maximum(1.0, np.abs(t).max(-1))


def make_dmat(seed, n, k, scale, spread=0.25):
    """a float32-exact distance-like matrix [N, K], entries scale |1 + spread N(0, 1)|: the input of the row / column kernels"""
    return f32(scale * np.abs(1.0 + spread * np.random.default_rng(seed).standard_normal((n, k))))


def make_entropy_inputs(seed, n, k, dim, scale, tie=None):
    """z [N, D], E [K, D] ~ scale N(0, 1), dq ~ 1e-3 N(0, 1), float32-exact.  Codebook rows ``tie`` = (a, b), a < b, are bit-equal
    and row 0 of z is drawn next to them, so row 0's two nearest codes tie exactly and a must win; every OTHER row is redrawn until its
    nearest and second-nearest distances (float64) are MARGIN max(1, max d) apart, and row 0 until that holds with code b left out."""
    rng = np.random.default_rng(seed)
    E = f32(scale * rng.standard_normal((k, dim)))
    tie = tie if tie is not None else ((1, 3) if k > 3 else None)
    if tie is not None:
        E[tie[1]] = E[tie[0]]
    z = f32(scale * rng.standard_normal((n, dim)))
    dq = f32(1e-3 * rng.standard_normal((n, dim)))
    redrawn = np.zeros(n, dtype=bool)
    rounds = 0
    for rounds in range(ROUNDS):
        if tie is not None and rounds == 0:
            z[0] = f32(E[tie[0]] + 0.05 * scale * rng.standard_normal(dim))
        d = entropy_distances(z, E)
        if tie is not None:
            d = np.delete(d, tie[1], axis=1)                       # the duplicate of code a (a < b: the indices below b stay)
        bad = ~_gap_ok(d, largest=False)
        if tie is not None and d[0].argmin() != tie[0]:
            bad[0] = True
        if not bad.any():
            break
        redrawn |= bad
        z[bad] = f32(scale * rng.standard_normal((int(bad.sum()), dim)))
        if tie is not None and bad[0]:
            z[0] = f32(E[tie[0]] + 0.05 * scale * rng.standard_normal(dim))
    else:
        rounds = ROUNDS
    return dict(z=z, E=E, dq=dq, tie=tie, rounds=rounds, resampled=float(redrawn.mean()))


def make_gumbel_inputs(seed, n, k, tau, ties=(), wide_row=None, logit_scale=1.0, flat=False):
    """logits [N, K] ~ logit_scale N(0, 1), noise ~ Exp(1) clamped to [1e-30, 1e4], float32-exact.  ``ties``: pairs (a, b), a < b < K;
    pair j is planted in row j -- both columns get bit-equal logits and noise, a noise small enough that they are the row's maxima --
    so a must win.  ``wide_row``: that row's noise spans 1e-30 .. 1e4 (log-uniform).  The noise row of every row whose best and
    second-best t = (logit - log noise) / tau (float64; a tie's twin left out) are closer than MARGIN max(1, max|t|) is redrawn.
    ``flat``: the noise is exp(logit - tau N(0, 1)) instead, so t ~ N(0, 1) whatever tau is: for the few-row shapes, whose rows would
    otherwise all be one-hot at a small tau and leave a gradient of rounding noise only."""
    rng = np.random.default_rng(seed)
    logits = f32(logit_scale * rng.standard_normal((n, k)))
    ties = [p for p in ties if p[1] < k]
    assert len(ties) <= n

    def draw(rows):
        nz = np.clip(rng.exponential(1.0, (len(rows), k)), NOISE_MIN, NOISE_MAX)
        if flat:
            nz = np.exp(logits[rows] - tau * rng.standard_normal((len(rows), k)))
        for j, r in enumerate(rows):
            if wide_row is not None and r == wide_row:
                nz[j] = 10.0 ** rng.uniform(-30.0, 4.0, k)
                nz[j, rng.integers(k)], nz[j, rng.integers(k)] = NOISE_MIN, NOISE_MAX
            if r < len(ties):
                a, b = ties[r]
                nz[j, a] = nz[j].min() * 1e-3 * np.exp(-abs(logits[r]).max() * 2)
                nz[j, b] = nz[j, a]
        return f32(np.clip(nz, NOISE_MIN, NOISE_MAX))
    for r, (a, b) in enumerate(ties):
        logits[r, b] = logits[r, a]
    noise = draw(list(range(n)))
    redrawn = np.zeros(n, dtype=bool)
    rounds = 0
    for rounds in range(ROUNDS):
        t = gumbel_t(logits, noise, tau)
        for r, (a, b) in enumerate(ties):
            t[r, b] = t[r].min()                                   # the twin of column a is left out of the gap
        bad = ~_gap_ok(t, largest=True) if k > 1 else np.zeros(n, dtype=bool)
        for r, (a, b) in enumerate(ties):
            if t[r].argmax() != a:
                bad[r] = True
        if not bad.any():
            break
        redrawn |= bad
        rows = np.flatnonzero(bad)
        noise[rows] = draw(list(rows))
    else:
        rounds = ROUNDS
    return dict(logits=logits, noise=noise, ties=ties, rounds=rounds, resampled=float(redrawn.mean()))


def atomic_bound(terms, m):
    """bound of a scalar summed by fp32 atomics, relative to the sum: the random-walk estimate of a sequential fp32 sum of ``m``
    addends with a margin of 4,  4 sqrt(m) 2^-24 sum|x_i| / |sum x_i|"""
    x = np.asarray(terms, dtype=np.float64)
    return float(4.0 * np.sqrt(m) * 2.0 ** -24 * np.abs(x).sum() / max(abs(x.sum()), 1e-300))
