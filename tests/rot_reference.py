"""Float64 reference of the rotation-trick backward (include/vqk.h: vqk_vq_backward_rot_f32; csrc/vq_rot.hip; no GPU):
Fifty et al., "Restructuring Vector Quantization with the Rotation Trick" (ICLR 2025).  Per latent row, z the encoder output,
q = e[idx] its code, g the decoder's gradient with respect to the quantized row:

    nz = max(|z|, 1e-6)      nq = max(|q|, 1e-6)      zh = z / nz      qh = q / nq      lam = nq / nz
    s = zh + qh              r = s / max(|s|, 1e-12)
    q~ = sg[lam] (z - 2 (z.r) r + 2 (z.zh) qh)                           zh, qh, r, lam constants (detached)
    dz = lam (g - 2 r (r.g) + 2 zh (qh.g)) + cz (z - q)                  de[idx] += ce (q - z)

``dz`` / ``q_tilde`` evaluate these lines as they stand in numpy float64; ``staged_f32`` restates dz in fp32 through the five dot
products zz, qq, zq, zg, qg -- the arithmetic of the kernels, evaluated on the CPU -- so that the CPU tests can say how far an
fp32 evaluation alone is from float64 on every input the GPU tests use.  ``make_case`` builds those inputs (seeded, shared)."""
import numpy as np

EPS_N, EPS_S = 1e-6, 1e-12
KINDS = ('noise0.01', 'noise0.1', 'noise0.3', 'indep')             # the main cases: zh.qh stays far from -1
NS = (1, 31, 32, 33, 257)
DS = (4, 6, 8, 64, 256, 260, 1024)
K_GRID = 32
ONE_CODE = (257, 1, 64, 'noise0.1')                              # every row on one code
LARGE = (4096, 1024, 256, 'noise0.1')
DEGENERATE = (67, 32, 16, 'degenerate')                          # rows 0, 1, 2: z = 0, q = 0, z = -q
SPECIAL_ROWS = (0, 1, 2)
G_SCALE = 0.03                                                   # the decoder's gradient: G_SCALE * randn
CZ, CE, GS = 0.1, 0.05, 0.7                                      # the two coefficients and the loss cotangent of the raw-kernel tests


def grid_cases():
    return [(n, K_GRID, d, kind) for kind in KINDS for d in DS for n in NS]


def all_cases():
    return grid_cases() + [ONE_CODE, LARGE, DEGENERATE]


def make_case(n, k, d, kind, seed=0):
    """(z [n, d] fp32, e [k, d] fp32, idx [n] int64, g [n, d] fp32) of one case.  noise<s>: codes ~ N(0, 1), every row a random code
    plus s * N(0, 1).  indep: z and the codes independent N(0, 1), idx the code of the largest cosine.  degenerate: noise0.1 with
    row 0 z = 0, row 1 on a zero code that no other row uses, row 2 z = -q."""
    rng = np.random.default_rng([seed, n, k, d, KINDS.index(kind) if kind in KINDS else 7])
    e = rng.standard_normal((k, d)).astype(np.float32)
    g = (G_SCALE * rng.standard_normal((n, d))).astype(np.float32)
    if kind == 'indep':
        z = rng.standard_normal((n, d)).astype(np.float32)
        zd, ed = z.astype(np.float64), e.astype(np.float64)
        cos = (zd / np.linalg.norm(zd, axis=1, keepdims=True)) @ (ed / np.linalg.norm(ed, axis=1, keepdims=True)).T
        idx = cos.argmax(1).astype(np.int64)
    else:
        scale = 0.1 if kind == 'degenerate' else float(kind[len('noise'):])
        idx = rng.integers(0, k, n).astype(np.int64)
        if kind == 'degenerate':
            idx[idx == 1] = 2
            idx[1] = 1
            e[1] = 0.0
        z = (e[idx] + scale * rng.standard_normal((n, d))).astype(np.float32)
        if kind == 'degenerate':
            z[0] = 0.0
            z[2] = -e[idx[2]]
    return z, e, idx, g


def _parts(z, q):
    nz = np.maximum(np.linalg.norm(z, axis=1, keepdims=True), EPS_N)
    nq = np.maximum(np.linalg.norm(q, axis=1, keepdims=True), EPS_N)
    zh, qh = z / nz, q / nq
    s = zh + qh
    r = s / np.maximum(np.linalg.norm(s, axis=1, keepdims=True), EPS_S)
    return zh, qh, r, nq / nz


def dz(z, q, g, cz=0.0):
    """the gradient that reaches z: float64 [n, d] (g None: the commitment term alone)"""
    z, q = np.asarray(z, np.float64), np.asarray(q, np.float64)
    out = cz * (z - q)
    if g is not None:
        g = np.asarray(g, np.float64)
        zh, qh, r, lam = _parts(z, q)
        out = lam * (g - 2.0 * r * (r * g).sum(1, keepdims=True) + 2.0 * zh * (qh * g).sum(1, keepdims=True)) + out
    return out


def q_tilde(z, q):
    """the rotated and rescaled z: equal to q up to rounding (float64 [n, d])"""
    z, q = np.asarray(z, np.float64), np.asarray(q, np.float64)
    zh, qh, r, lam = _parts(z, q)
    return lam * (z - 2.0 * (z * r).sum(1, keepdims=True) * r + 2.0 * (z * zh).sum(1, keepdims=True) * qh)


def de(z, e, idx, ce):
    """the codebook gradient of the straight-through lookup, unchanged by the estimator: float64 [k, d]"""
    z, e = np.asarray(z, np.float64), np.asarray(e, np.float64)
    out = np.zeros_like(e)
    np.add.at(out, idx, ce * (e[idx] - z))
    return out


def cos_zq(z, q):
    z, q = np.asarray(z, np.float64), np.asarray(q, np.float64)
    return (z * q).sum(1) / np.maximum(np.linalg.norm(z, axis=1) * np.linalg.norm(q, axis=1), 1e-300)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, the sum is rounded once more on its way to
    fp32 (a double rounding that differs from the hardware's single one in rare ties only)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def staged_f32(z, q, g, cz=0.0, flavour='plain'):
    """dz in fp32 through the five dot products (the expression sequence of csrc/vq_rot.hip::rot_coef), evaluated on the CPU: a
    restatement, not a bit model of the kernels.  flavour 'plain': numpy's fp32 pairwise sums, every product and sum rounded;
    'fma': the sums as 64 interleaved chains of fused multiply-adds (the columns of a lane) that are then added up, and the last line as
    fused multiply-adds -- the two ends of what a compiler may make of the expressions."""
    f = np.float32
    z, q, g = np.asarray(z, f), np.asarray(q, f), np.asarray(g, f)
    if flavour == 'plain':
        dot = lambda a, b: (a * b).sum(1, dtype=f, keepdims=True)
    else:
        def dot(a, b):                                           # 64 interleaved chains (a lane's columns), then their sum
            acc = np.zeros((a.shape[0], 64), f)
            for c0 in range(0, a.shape[1], 64):
                w = min(64, a.shape[1] - c0)
                acc[:, :w] = _fma(a[:, c0:c0 + w], b[:, c0:c0 + w], acc[:, :w])
            return acc.sum(1, dtype=f, keepdims=True)
    zz, qq, zq, zg, qg = dot(z, z), dot(q, q), dot(z, q), dot(z, g), dot(q, g)
    nz, nq = np.maximum(np.sqrt(zz), f(EPS_N)), np.maximum(np.sqrt(qq), f(EPS_N))
    inz, inq = f(1) / nz, f(1) / nq
    lam = nq * inz
    ss = zz * inz * inz + qq * inq * inq + f(2) * zq * inz * inq
    ins = f(1) / np.maximum(np.sqrt(np.maximum(ss, f(0))), f(EPS_S))
    qhg = qg * inq
    t = f(2) * lam * ((zg * inz + qhg) * ins) * ins
    a = (f(2) * lam * qhg - t) * inz
    b = -t * inq
    if flavour == 'plain':
        out = (lam * g + a * z + b * q) + f(cz) * (z - q)
    else:
        out = _fma(f(cz), z - q, _fma(b, q, _fma(a, z, lam * g)))
    assert out.dtype == f
    return out
