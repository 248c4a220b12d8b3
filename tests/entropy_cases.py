"""The cases of tests/test_gpu_entropy.py and tests/test_gpu_gumbel.py, their float64 / float32 references (tests/entropy_reference.py;
computed once per case, shared read-only) and their bounds.  Nothing here touches a device: tests/test_entropy_cpu.py evaluates every
bound from the reference alone (``cpu_bounds``) and requires each to discriminate.

Bounds.  e32 = distance(float32 evaluation, float64 evaluation) on the same inputs; the device may be at max(16 e32, floor) -- sixteen
as in tests/test_gpu_lfq.py: another summation order and the device's own __expf / __logf.  floor = 1e-6 for elementwise results; a
scalar summed by fp32 atomics takes the random-walk estimate of a sequential fp32 sum instead, 4 sqrt(m) 2^-24 sum|x_i| / |sum x_i| with
m addends (``entropy_reference.atomic_bound``)."""
import numpy as np

from tests import entropy_reference as R

F32, F64 = np.float32, np.float64
BETA, RATIO, GLOSS = 0.25, 0.1, 1.7
GS_VALUES = (1.0, 1.7)


def freeze(part):
    for arr in part.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return part


class Lazy(dict):
    """a dict whose missing entries are computed by ``make(key)`` on first use and kept, read-only: the large gradients of a case are
    built only for the tests (or bound checks) that ask for them"""

    def __init__(self, items, make):
        super().__init__(items)
        self.make = make

    def __missing__(self, key):
        value = self.make(key)
        value.setflags(write=False)
        self[key] = value
        return value


def bound(e32, floor=1e-6):
    return max(16.0 * e32, floor)


def e32_of(ref, key):
    return R.distance(ref['f32'][key], ref['f64'][key])


# ----------------------------------------------------------------------------------------------------------------------------------
# (a) the row / column kernels of csrc/entropy.hip on a given matrix
# ----------------------------------------------------------------------------------------------------------------------------------
# (N, K): one row / a partial block of four rows, one trip plus 4 columns / exactly one trip / a ragged second trip / many trips /
# rows_per_block = 16 with a 3-row last slab / rows_per_block = 17 / more than one column block in the finalize kernel's grid
ROWCOL_SHAPES = [(1, 4), (3, 68), (67, 64), (67, 100), (259, 1000), (2051, 256), (4115, 8), (131, 8192)]
# (T, scale of the entries): 2 D for D = 16 at T = 1; the trained-latent scale at T = 0.01
ROWCOL_TEMPS = [(1.0, 32.0), (0.01, 0.3)]
_ROWCOL: dict = {}


def rows_per_block(n):
    """the row slab of entropy_colsum_kernel (vqk_entropy_forward_f32)"""
    return max(16, (n + 255) // 256)


def rowcol_id(shape):
    return f'N{shape[0]}-K{shape[1]}'


def rowcol_reference(shape, temp):
    key = (shape, temp)
    if key not in _ROWCOL:
        (n, k), (t, scale) = shape, temp
        # few columns: a narrower spread of the entries (+-1 nat, not +-8), or every row is one-hot and its entropy rounding noise
        d = R.make_dmat(3000 + 10 * ROWCOL_SHAPES.index(shape) + ROWCOL_TEMPS.index(temp), n, k, scale, 0.25 if k >= 64 else 0.03)
        idx = d.argmin(-1)
        hist = np.bincount(idx, minlength=k)
        out = dict(d=d, idx=idx, hist=hist)
        for name, dt in (('f64', F64), ('f32', F32)):
            lse, hrow, hsum = R.entropy_rows(d, t, dt)
            psum, u, avg = R.entropy_cols(d, t, dt)
            am = R.entropy_argmax_forward(d, idx, hist, t, dt)
            part = dict(lse=lse, hrow=hrow, hsum=hsum, psum=psum, u=u, avg=avg, ssum=am[3], m=am[4], u_am=am[5], avg_am=am[6])
            # 'dd-<loss type>-<gs>': on first use
            out[name] = Lazy(freeze(part), lambda key, dt=dt: R.entropy_dd(d, t, RATIO, float(key.split('-')[2]), key.split('-')[1], idx, dt))
        f = out['f64']
        pbar, mbar = f['psum'] / n, f['m'] / n
        out['floor'] = dict(hsum=R.atomic_bound(f['hrow'], n), ssum=R.atomic_bound(f['lse'] + d[np.arange(n), idx] / t, n),
                            psum=R.atomic_bound([1.0], -(-n // rows_per_block(n))), avg=R.atomic_bound(pbar * np.log(pbar + R.EPS_ENT), k),
                            avg_am=R.atomic_bound(mbar * np.log(mbar + R.EPS_ENT), k))
        _ROWCOL[key] = freeze(out)
    return _ROWCOL[key]


def rowcol_bound(ref, key):
    return bound(e32_of(ref, key), ref['floor'].get(key, 1e-6))


# ----------------------------------------------------------------------------------------------------------------------------------
# (c) EntropyVQFn end to end
# ----------------------------------------------------------------------------------------------------------------------------------
# (N, K, D, T, dtype, loss type, ENTROPY_SPLIT_GEMM): ragged everything / the same with one-hot targets / many trips at the production
# temperature / fused rows, register form (259 rows), fused VQ backward / D = 256 without fused rows / the smallest split-product
# shape / split product, fused rows and LDS form together / the fp32 GEMM route from a bf16 model
VQ_CASES = [(67, 68, 16, 1.0, 'fp32', 'softmax', True), (67, 68, 16, 1.0, 'fp32', 'argmax', True),
            (515, 1000, 64, 0.01, 'fp32', 'softmax', True), (259, 128, 256, 0.01, 'fp32', 'softmax', True),
            (384, 256, 256, 0.01, 'fp32', 'argmax', True), (256, 128, 128, 0.01, 'bf16', 'softmax', True),
            (384, 256, 256, 0.01, 'bf16', 'softmax', True), (256, 128, 128, 0.01, 'bf16', 'softmax', False)]
# backward settings: name -> (dq used, loss cotangent or None)
VQ_SETTINGS = {'dq': (True, None), 'loss': (False, GLOSS), 'both': (True, GLOSS)}
_VQ: dict = {}


def vq_id(c):
    return f'N{c[0]}-K{c[1]}-D{c[2]}-T{c[3]}-{c[4]}-{c[5]}' + ('' if c[6] else '-nosplit')


def vq_split_route(c):
    """the dispatch rule of EntropyVQFn this case is meant to meet"""
    n, k, dim, _, dt, lt, on = c
    return on and dt == 'bf16' and lt == 'softmax' and n % 128 == 0 and k % 128 == 0 and dim % 128 == 0


def vq_reference(case):
    if case not in _VQ:
        n, k, dim, t, dt, lt, _ = case
        inp = R.make_entropy_inputs(4000 + VQ_CASES.index(case), n, k, dim, 1.0 if t == 1.0 else 0.05)
        assert inp['rounds'] < R.ROUNDS, 'rows still near a tie after the last round'
        dq = R.bf16(inp['dq']) if dt == 'bf16' else inp['dq']
        out = dict(inp=freeze(inp), dq_in=dq)
        for name, (use_dq, gloss) in VQ_SETTINGS.items():
            args = (inp['z'], inp['E'], BETA, RATIO, t, lt, dq if use_dq else None, gloss)
            ent = dict(f64=freeze(R.entropy_vq(*args)), f32=freeze(R.entropy_vq(*args, dtype=F32)))
            if vq_split_route(case) and gloss is not None:
                ent['split'] = freeze(R.entropy_vq(*args, split=True))
            out[name] = ent
        f = out['both']['f64']
        np.testing.assert_array_equal(out['both']['f32']['idx'], f['idx'])
        _VQ[case] = out
    return _VQ[case]


def vq_grad_bound(ent, key):
    """(e32, e_split or None, bound) of dz / dE in one backward setting"""
    e32 = R.distance(ent['f32'][key], ent['f64'][key])
    es = R.distance(ent['split'][key], ent['f64'][key]) if 'split' in ent else None
    return e32, es, bound(max(e32, es or 0.0))


def vq_loss_bound(case, ref):
    """(scale, e32, bound, plain bound): the loss over its largest term; the floor is the atomic estimate with every element of
    (q - z)^2 an addend (an upper estimate of m: the kernels add per-wave partial sums).  ``plain bound`` is the same bound in the plain
    ``distance`` (relative to |loss| itself): the entropy terms cancel, so it is larger by scale / |loss|, and it is asserted as well
    where it still discriminates (<= 1e-3)."""
    n, k, dim, t = case[:4]
    f = ref['both']['f64']
    mse = float(((f['q'] - ref['inp']['z']) ** 2).mean())
    if case[5] == 'softmax':
        a, b = R.entropy_rows(f['d'], t)[2] / n, R.entropy_cols(f['d'], t)[2]
    else:
        am = R.entropy_argmax_forward(f['d'], f['idx'], f['hist'], t)
        a, b = am[3] / n, am[6]
    scale = max((1 + BETA) * mse, RATIO * abs(a), RATIO * abs(b))
    e32 = abs(float(ref['both']['f32']['loss']) - float(f['loss'])) / scale
    b = bound(e32, R.atomic_bound([1.0], n * dim))
    return scale, e32, b, b * scale / abs(float(f['loss']))


# ----------------------------------------------------------------------------------------------------------------------------------
# (d) the Gumbel row kernels
# ----------------------------------------------------------------------------------------------------------------------------------
# (N, K): one column / a partly idle wave / exactly one trip / one column in the second trip / a ragged second trip / many trips /
# many blocks of half-idle waves
GUM_SHAPES = [(1, 1), (3, 5), (67, 64), (67, 65), (67, 100), (515, 1000), (2051, 32)]
GUM_TAUS = (1.0, 0.05)
GUM_TIES = [(0, 64), (3, 40)]                  # row 0: the same lane in two trips; row 1: two lanes of one trip
GUM_WIDE = (67, 100)                           # the case whose row 2 has noise from 1e-30 to 1e4
KL_HOST, KL_SCHED = 0.3, 0.7
# backward settings: name -> (dy used, cotangent of the KL sum or None, schedule tensor used); the KL coefficient is KL_HOST without
# and KL_SCHED with a schedule tensor (the host arguments then carry 2 tau and KL_HOST, both to be ignored), 0 without KL_HOST
GUM_SETTINGS = {'dy': (True, None, False), 'dy+kl': (True, GLOSS, False), 'kl': (False, GLOSS, False),
                'sched-dy+kl': (True, GLOSS, True), 'sched-kl': (False, GLOSS, True), 'sched-kl-nogs': (False, None, True)}
_GUM: dict = {}


def gum_id(shape):
    return f'N{shape[0]}-K{shape[1]}'


def gum_klc(setting, n):
    """the coefficient of sum_i kl_i's gradient the C ABI promises: kl_cost / n times the cotangent (absent: 1), kl_cost from the
    schedule tensor when there is one.  'dy' passes kl_cost = 0."""
    _, gs, sched = GUM_SETTINGS[setting]
    if setting == 'dy':
        return 0.0
    return (KL_SCHED if sched else KL_HOST) / n * (1.0 if gs is None else gs)


def gumbel_reference(shape, tau):
    key = (shape, tau)
    if key not in _GUM:
        n, k = shape
        seed = 5000 + 10 * GUM_SHAPES.index(shape) + GUM_TAUS.index(tau)
        inp = R.make_gumbel_inputs(seed, n, k, tau, ties=GUM_TIES, wide_row=2 if shape == GUM_WIDE else None,
                                   flat=n < 16 and k > 1)
        assert inp['rounds'] < R.ROUNDS, 'rows still near a tie after the last round'
        dy = R.f32(np.random.default_rng(seed + 1).standard_normal((n, k)))
        out = dict(inp=freeze(inp), dy={'fp32': dy, 'bf16': R.bf16(dy), 'zero': np.zeros_like(dy)})
        for name, dt in (('f64', F64), ('f32', F32)):
            y, idx, klsum, hist = R.gumbel_rows(inp['logits'], inp['noise'], tau, False, dt)
            part = dict(y=y, idx=idx, klsum=klsum, hist=hist)
            # 'dl|<setting>|<dy kind>': on first use
            out[name] = Lazy(freeze(part), lambda key, dt=dt: R.gumbel_rows_backward(inp['logits'], inp['noise'], out['dy'][key.split('|')[2]], tau,
                                                                                      gum_klc(key.split('|')[1], n), dt))
        np.testing.assert_array_equal(out['f32']['idx'], out['f64']['idx'])
        _, qy, _ = R._softmax_parts(inp['logits'])
        out['floor'] = dict(klsum=R.atomic_bound((qy * np.log(qy * k + R.EPS_KL)).sum(-1), n))
        _GUM[key] = out
    return _GUM[key]


def gum_dl_keys(settings=None):
    return [f'dl|{s}|{dyn}' for s, (use_dy, _, _) in GUM_SETTINGS.items() if settings is None or s in settings
            for dyn in (('fp32', 'bf16') if use_dy else ('zero',))]


def gum_bound(ref, key):
    return bound(e32_of(ref, key), ref['floor'].get(key, 1e-6))


# ----------------------------------------------------------------------------------------------------------------------------------
# (b) the statistics epilogues of the distance kernels
# ----------------------------------------------------------------------------------------------------------------------------------
# (96, 104) stays on the register kernel whatever the VQ_LDS slot says; (128, 64) one K part of two tiles; (384, 320) one part; K = 1024:
# four parts merged by vq_lds_merge_kernel
STATS_SHAPES = [(96, 104), (128, 64), (384, 320), (128, 1024), (384, 1024)]
# T -> scale of z and e (D = 256): distances of order 1.3 at T = 0.05 and 0.3 at T = 0.01, so |lse| ~ 25 in both -- at the scale 0.05
# with T = 0.01 it is ~120 and cancels three digits of h (the float32 yardstick of hrow is then 2.5e-4, its bound 4e-3)
STATS_TEMPS = {0.05: 0.05, 0.01: 0.025}
_STATS: dict = {}


def stats_lds_form(n, k, slot):
    """the dispatch rule of vqk_vq_distances_stats_f32 (csrc/vq.hip, D = 256): whole 128-row blocks and whole 32-code tiles"""
    return bool(slot) and n % 128 == 0 and k % 32 == 0


def stats_inputs(shape, t):
    key = (shape, t)
    if key not in _STATS:
        (n, k), scale = shape, STATS_TEMPS[t]
        rng = np.random.default_rng(6000 + n + k)
        z, e = R.f32(scale * rng.standard_normal((n, 256))), R.f32(scale * rng.standard_normal((k, 256)))
        e[:8] = R.f32(z[:8] + 0.02 * scale * rng.standard_normal((8, 256)))          # near one-hot rows
        e[5] = e[3]                                                                   # an exact tie: row 3 has two nearest codes
        _STATS[key] = freeze(dict(z=z, e=e))
    return _STATS[key]


def stats_reference(dmat, t):
    """(float64 rows, float32 rows, bounds of lse / hrow / hsum) of ONE fp32 distance matrix: the device's on the GPU, the host's float32
    evaluation in ``cpu_bounds``"""
    dmat = np.asarray(dmat, dtype=F64)
    w64, w32 = R.entropy_rows(dmat, t), R.entropy_rows(dmat, t, F32)
    floors = (1e-6, 1e-6, R.atomic_bound(w64[1], dmat.shape[0]))
    return w64, w32, tuple(bound(R.distance(a, b), f) for a, b, f in zip(w32, w64, floors))


# ----------------------------------------------------------------------------------------------------------------------------------
# (e) GumbelVQFn / GumbelVectorQuantizer, and vqk_row_scale_add_f32
# ----------------------------------------------------------------------------------------------------------------------------------
FN_SHAPES = [(67, 64, 8), (515, 128, 32), (256, 256, 64)]          # (N, K, D): K and D that the 1x1 GEMMs accept
FN_TAU, FN_KL = 0.5, 0.05
_FN: dict = {}


def fn_id(s):
    return f'N{s[0]}-K{s[1]}-D{s[2]}'


def fn_inputs(shape):
    if shape not in _FN:
        n, k, dim = shape
        seed = 7000 + FN_SHAPES.index(shape)
        inp = R.make_gumbel_inputs(seed, n, k, FN_TAU, ties=[(3, 40)])
        assert inp['rounds'] < R.ROUNDS, 'rows still near a tie after the last round'
        rng = np.random.default_rng(seed + 1)
        inp['E'], inp['dq'] = R.f32(rng.standard_normal((k, dim))), R.f32(rng.standard_normal((n, dim)))
        _FN[shape] = freeze(inp)
    return _FN[shape]


def fn_reference(shape, dt, hard, gkl, use_dq=True):
    """(float64, float32) ``gumbel_vq``; a bf16 model rounds E and dq on the way in and stores y and dy = dq E^T in bf16"""
    key = (shape, dt, hard, gkl, use_dq)
    if key not in _FN:
        inp = fn_inputs(shape)
        rnd = R.bf16 if dt == 'bf16' else (lambda a: a)
        args = (inp['logits'], rnd(inp['E']), inp['noise'], FN_TAU, FN_KL, hard, rnd(inp['dq']) if use_dq else None, gkl)
        kw = dict(round_y=R.bf16) if dt == 'bf16' else {}
        _FN[key] = (freeze(R.gumbel_vq(*args, **kw)), freeze(R.gumbel_vq(*args, dtype=F32, **kw)))
    return _FN[key]


def fn_kl_floor(shape):
    inp = fn_inputs(shape)
    _, qy, _ = R._softmax_parts(inp['logits'])
    return R.atomic_bound((qy * np.log(qy * shape[1] + R.EPS_KL)).sum(-1), shape[0])


RSA_SHAPES = [(1, 1), (67, 16), (1000, 64), (8200, 65)]            # (rows, c); the last: more elements than one pass of the grid
_RSA: dict = {}


def rsa_reference(shape):
    """out += 2 scale[r] m[r][c]: inputs and the (float64, float32) results"""
    if shape not in _RSA:
        rows, c = shape
        rng = np.random.default_rng(rows + c)
        out, m, scale = (R.f32(rng.standard_normal(s)) for s in ((rows, c), (rows, c), (rows,)))
        want = lambda dt: out.astype(dt) + dt(2.0) * scale.astype(dt)[:, None] * m.astype(dt)
        _RSA[shape] = freeze(dict(out=out, m=m, scale=scale, f64=want(F64), f32=want(F32)))
    return _RSA[shape]


# ----------------------------------------------------------------------------------------------------------------------------------
def cpu_bounds():
    """name of a quantity -> (its largest fp32 bound over the cases, that case), for (a) to (e) and row_scale_add.  Left out, each
    degenerate at ANY data scale: the one-row 'softmax' cotangent and the one-row 'argmax' avg_term of (a), and klsum at K = 1; also
    gradients that are exactly zero in float64 (the device must then return zero itself).  The bf16 results of (e) have bounds from the
    number format, not from e32: they are not in here."""
    worst: dict = {}

    def note(name, b, case):
        if b > worst.get(name, (0.0, None))[0]:
            worst[name] = (b, case)
    # only gs = 1.7 and, beyond the small shapes, one backward setting of each kind are built: the others repeat the same formulas at other
    # constants (the GPU tests evaluate each one's own bound)
    for shape in ROWCOL_SHAPES:
        for temp in ROWCOL_TEMPS:
            ref = rowcol_reference(shape, temp)
            dd_keys = [f'dd-{lt}-{gs}' for lt in ('softmax', 'argmax') for gs in GS_VALUES[1:]]
            for key in list(ref['f64']) + dd_keys:
                if shape[0] == 1 and (key.startswith('dd-softmax') or key == 'avg_am'):
                    # one row at any data scale: its entropy IS the entropy of its mean, so the 'softmax' loss and its gradient are
                    # what the 1e-5 inside the logarithm leaves (float32 keeps no digit of it); a one-hot histogram's term is
                    # log(1 + 1e-5), bound 2.2e-2.  On the device the cotangent takes the magnitude check of a vacuous bound as well.
                    continue
                if key != 'm':
                    note('rowcol ' + key.split('-1.')[0], rowcol_bound(ref, key), (shape, temp))
    for shape in STATS_SHAPES:
        for t in STATS_TEMPS:
            inp = stats_inputs(shape, t)
            bounds = stats_reference(R.entropy_distances(inp['z'], inp['e'], F32), t)[2]          # the host's fp32 matrix for the device's
            for name, b in zip(('lse', 'hrow', 'hsum'), bounds):
                note('stats ' + name, b, (shape, t))
    for case in VQ_CASES:
        ref = vq_reference(case)
        note('vq loss', vq_loss_bound(case, ref)[2], vq_id(case))
        note('vq loss, relative to itself', vq_loss_bound(case, ref)[3], vq_id(case))
        for setting in VQ_SETTINGS:
            for key in ('dz', 'dE'):
                if np.any(ref[setting]['f64'][key]):
                    note(f'vq {key} {setting}', vq_grad_bound(ref[setting], key)[2], vq_id(case))
    for shape in GUM_SHAPES:
        big = shape[0] * shape[1] > 5000
        for tau in GUM_TAUS:
            ref = gumbel_reference(shape, tau)
            for key in list(ref['f64']) + gum_dl_keys(('dy+kl', 'kl', 'sched-kl-nogs') if big else None):
                if key == 'klsum' and shape[1] == 1:
                    continue                   # K = 1: kl_i = log(1 + 1e-10), 1e-10 in float64 and 0 in float32 at any data scale
                if key not in ('idx', 'hist') and np.any(ref['f64'][key]):
                    note('gumbel ' + key.split('|fp32')[0].split('|bf16')[0], gum_bound(ref, key), (shape, tau))
    for shape in FN_SHAPES:
        for hard in (False, True):
            w64, w32 = fn_reference(shape, 'fp32', hard, GLOSS)
            for key in ('q', 'kl', 'dlogits', 'dE'):
                note('gumbel-fn ' + key, bound(R.distance(w32[key], w64[key]), fn_kl_floor(shape) if key == 'kl' else 1e-6), (fn_id(shape), hard))
    for shape in RSA_SHAPES:
        ref = rsa_reference(shape)
        note('row_scale_add', bound(R.distance(ref['f32'], ref['f64'])), shape)
    return worst
