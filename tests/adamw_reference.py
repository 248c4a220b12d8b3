"""Float64 restatement of the AdamW arena kernel (csrc/optim.hip: adamw_kernel behind vqk_adamw / vqk_adamw_guarded), its
rounding bound, the kernel's own operation order in numpy float32, and the cases the CPU and GPU tests share.  Plain numpy,
independent of the product code.

  step64   one step of torch.optim.AdamW (decoupled decay, no amsgrad) in float64 from a given state, with the hyper-parameters
           the kernel really receives: lr, betas, eps and grad_scale are C floats, the bias corrections are
           1 - (double)(float)beta ** t (vqk_adamw's host expressions).  Returns the magnitudes the bound is made of as well.
  bound    the distance a correct float32 kernel may keep from step64 (an operation count, below).
  step32   the kernel's operation order, every operation rounded to float32: the yardstick of free-running runs.
  Case     hyper-parameters + segment table + seeded inputs; TABLES / LENGTHS / *_cases() list what the tests run.
  MUTATIONS  the mistakes the cases must be able to see (tests/test_adamw_cpu.py applies each to step64).

tests/test_adamw_cpu.py checks this file against torch.optim.AdamW on CPU float64 tensors."""
import math

import numpy as np

from tests import stepguard_reference as R

F = np.float32
U32 = 2.0 ** -24          # unit roundoff of float32: one correctly rounded operation errs by at most U32 * |result|
CHUNK, STRIDE = 8192, 1024   # adamw_kernel: a block owns 8192 elements, as eight strides of 256 threads x 4 elements
N_BIG = 2 * CHUNK + 7     # two full blocks and a tail that is no multiple of 4


def f32(x):
    """the double value of ``x`` passed as a C float"""
    return float(F(x))


def bias_corrections(beta1, beta2, t):
    """(bc1, bc2) as vqk_adamw computes them: 1 - pow((double)(float)beta, t)"""
    return 1.0 - f32(beta1) ** t, 1.0 - f32(beta2) ** t


def step64(p, g, m, v, wd, lr, beta1, beta2, eps, t, grad_scale=1.0, mutate=None):
    """One AdamW step t in float64 from the state (p, g, m | None, v) (float32 arrays, or float64 ones of a free-running
    reference); ``wd`` per element.  ``m`` None: the first moment is the scaled gradient itself (beta1 must be 0).
    ``mutate``: one of MUTATIONS' arithmetic mistakes (None: the correct step).

    Returns a dict: p, m, v the new state (m: the first moment used, also when it is not stored), and -- of the correct step --
      A = |p (1 - lr wd)|                                         the decayed parameter
      M = |b1 m| + |(1 - b1) g s|                                 the first moment's terms
      U = (lr / bc1) M / (sqrt(v') / sqrt(bc2) + eps)             the update with its terms taken absolutely"""
    p, g, v, wd = (np.array(a, dtype=np.float64) for a in (p, g, v, wd))
    lr, b1, b2, eps, s = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(grad_scale)
    if m is None:
        assert b1 == 0.0
    gs = g if mutate == 'scale_dropped' else g * s
    m_old = np.zeros_like(p) if m is None else np.array(m, dtype=np.float64)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(all='ignore'):
        M = np.abs(b1 * m_old) + np.abs((1.0 - b1) * gs)
        A = np.abs(p * (1.0 - lr * wd))
    if mutate is None or mutate == 'scale_dropped':
        # the arithmetic is stepguard_reference.adamw_step, which tests/test_stepguard_cpu.py pins to torch.optim.AdamW
        out_p, out_v, m_new = p, v, m_old.copy()
        with np.errstate(all='ignore'):                 # (a non-finite gradient is data: the containment test)
            R.adamw_step(out_p, gs, m_new, out_v, wd, lr, b1, b2, eps, t)
    else:
        if mutate.startswith('bc1_t'):
            bc1 = 1.0 - b1 ** (t + (1 if mutate.endswith('+1') else -1))
        if mutate.startswith('bc2_t'):
            bc2 = 1.0 - b2 ** (t + (1 if mutate.endswith('+1') else -1))
        out_p = p * (1.0 - lr * wd)
        m_new = m_old if mutate == 'm_not_updated' else b1 * m_old + (1.0 - b1) * gs
        gv = g if mutate == 'v_unscaled_g' else gs
        out_v = b2 * v + (1.0 - b2) * gv * gv
        with np.errstate(all='ignore'):
            if mutate == 'eps_in_sqrt':
                den = np.sqrt(out_v / bc2 + eps)
            else:
                den = np.sqrt(out_v) / math.sqrt(bc2) + eps if bc2 > 0.0 else np.full_like(out_v, np.inf)
            out_p = out_p - (lr / bc1 if bc1 > 0.0 else math.inf) * m_new / den
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(all='ignore'):
        U = (lr / bc1) * M / (np.sqrt(out_v) / math.sqrt(bc2) + eps)
    return dict(p=out_p, m=m_new, v=out_v, A=A, M=M, U=U)


def bound(A, U, v_new, M):
    """(bound_p, bound_v, bound_m): how far a correct float32 evaluation may lie from step64.  Every float32 operation is
    correctly rounded (error <= U32 |result|) except sqrt and divide, which are allowed 2.5 ulp; a fused multiply-add only
    removes a rounding.  Counting roundings, each relative to the magnitude it acts on:

      v' = b2 v + ((1 - b2) gr) gr, gr = g s    gr 1 (twice: it enters squared) + two products 2 + b2 v 1 + the sum 1     = 6 on v'
                                                (1 - b2 is exact for the betas in use: Sterbenz)
      m' = b1 m + (1 - b1) gr                   gr 1, two products (at most 1 on either term), the sum 1              <= 4 on M
      p  = p (1 - lr wd)                        lr wd 1, 1 - . 1, the product 1                                       = 3 on A
      update = step (m' / (sqrt(v') inv + eps)) m' 3 (its own sum counted: relative to M, so absolute terms)
                                                sqrt(v') 6/2 + 2.5, inv = (float)(1/sqrt(bc2)) 0.5, product 1, + eps 1  = 8
                                                divide 2.5, step = (float)(lr/bc1) 0.5, product 1                      = 4
                                                                                                            3 + 8 + 4 = 15 <= 16 on U
      p -= update                               1 on |p'| <= A + U: with the above, 4 on A and 16 on U

    so  |dp| <= U32 (4 A + 16 U),  |dv| <= U32 6 v',  |dm| <= U32 4 M."""
    return U32 * (4.0 * A + 16.0 * U), U32 * 6.0 * v_new, U32 * 4.0 * M


def step32(p, g, m, v, wd, lr, beta1, beta2, eps, t, grad_scale=1.0):
    """adamw_one's operation order in numpy float32 (no fused multiply-add, correctly rounded sqrt / divide) -> (p, m, v);
    ``m`` None: the first moment is not stored and the returned m is the scaled gradient"""
    p, g, v, wd = (np.asarray(a, dtype=F) for a in (p, g, v, wd))
    bc1, bc2 = bias_corrections(beta1, beta2, t)
    lr, b1, b2, eps, s = F(lr), F(beta1), F(beta2), F(eps), F(grad_scale)
    step_size, inv_sqrt_bc2 = F(float(lr) / bc1), F(1.0 / math.sqrt(bc2))
    one = F(1.0)
    with np.errstate(all='ignore'):
        gr = g * s
        pv = p * (one - lr * wd)
        mv = gr if m is None else b1 * np.asarray(m, dtype=F) + (one - b1) * gr
        vv = b2 * v + (one - b2) * gr * gr
        den = np.sqrt(vv) * inv_sqrt_bc2 + eps
        pv = pv - step_size * (mv / den)
    assert pv.dtype == F and mv.dtype == F and vv.dtype == F
    return pv, mv, vv


# ---------------------------------------------------------------------------------------------- mistakes the cases must see
# arithmetic ones (step64's ``mutate``); the two decay mistakes are a wrong ``wd`` array: Case.neighbour_wd
MUTATIONS = ('bc1_t-1', 'bc1_t+1', 'bc2_t-1', 'bc2_t+1', 'scale_dropped', 'm_not_updated', 'v_unscaled_g', 'eps_in_sqrt')


def bias_shift(beta, t, dt):
    """relative change of 1 - beta^t when t is off by dt (inf when the wrong one is 0)"""
    b = f32(beta)
    right, wrong = 1.0 - b ** t, 1.0 - b ** (t + dt)
    return math.inf if wrong == 0.0 else abs(wrong / right - 1.0)


# ---------------------------------------------------------------------------------------------- segment tables
def _table(sizes, wds, pad=None):
    sizes = np.asarray(sizes, dtype=np.int64)
    assert (sizes >= 0).all() and len(sizes) == len(wds)
    pad = np.zeros(len(sizes), dtype=bool) if pad is None else np.asarray(pad, dtype=bool)
    return dict(ends=np.cumsum(sizes), wd=np.asarray(wds, dtype=F), pad=pad)


def _cycle(k, values=(0.1, 0.3, 0.0, 0.2)):
    return [values[i % len(values)] for i in range(k)]


def _from_ends(ends, n=N_BIG):
    ends = list(ends) + [n]
    sizes = np.diff([0] + ends)
    return _table(sizes, _cycle(len(sizes)))


def table_single(n, wd=0.1):
    return _table([n], [wd])


def table_residues():
    """segment ends at every residue mod 4, in both blocks"""
    return _from_ends([997, 2002, 3003, 4000, 9001, 12002, 15003])


def table_ones():
    """40 one-element segments with alternating decays across the block boundary at 8192: the four elements of a thread lie
    in four segments, and the cached segment is left on every element"""
    return _table([8170] + [1] * 40 + [N_BIG - 8210], [0.2] + [0.0, 0.3] * 20 + [0.1])


def table_edges():
    """ends exactly on a stride (1024), on the block (8192) and one to either side of it"""
    return _from_ends([1024, 8191, 8192, 8193])


def table_flat():
    """FlatAdamW's shape: tensors whose sizes are no multiple of 64, each followed by its padding segment (decay 0, and the
    state in it all zero); the last tensor runs to the end of the arena"""
    sizes, wds, pad, total = [], [], [], 0
    for k, n in enumerate([3, 1, 65, 577, 27, 1729, 4099, 130, 5001, 63]):
        padded = -(-n // 64) * 64
        sizes += [n, padded - n]
        wds += [(0.1, 0.3)[k % 2], 0.0]
        pad += [False, True]
        total += padded
    sizes.append(N_BIG - total)
    wds.append(0.2)
    pad.append(False)
    assert sizes[-1] > 0
    return _table(sizes, wds, pad)


def table_many():
    """256 segments with 256 distinct decays: the depth of the real model's binary search"""
    rng = np.random.default_rng(256)
    cuts = np.sort(rng.choice(np.arange(1, N_BIG), 255, replace=False))
    sizes = np.diff(np.concatenate([[0], cuts, [N_BIG]]))
    order = rng.permutation(256)
    for i in range(1, 256):                       # neighbours differ by at least 2 hundredths
        if abs(int(order[i]) - int(order[i - 1])) < 2:
            j = (i + 7) % 256
            order[i], order[j] = order[j], order[i]
    wds = 0.01 * (order + 1)
    assert len(set(wds.tolist())) == 256
    return _table(sizes, wds)


def table_empty():
    """an empty segment: a repeated end (its decay, 0.5, belongs to no element)"""
    return _table([4099, 0, 2901, 1, 0, 0, N_BIG - 7001], [0.1, 0.5, 0.3, 0.0, 0.5, 0.4, 0.2])


TABLES = dict(residues=table_residues, ones=table_ones, edges=table_edges, flat=table_flat, many=table_many, empty=table_empty)
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, N_BIG)
# betas and whether the first moment is stored
M_FORMS = {'b1=0,m=null': ((0.0, 0.99), False), 'b1=0,m': ((0.0, 0.99), True), 'b1=0.9': ((0.9, 0.999), True),
           'b1=0.5': ((0.5, 0.9), True)}
T_VALUES = (1, 2, 3, 10, 1000, 3725, 100000)
SCALES = (1.0, 0.5, 0.125)


class Case:
    """One launch: a segment table, hyper-parameters and seeded inputs.

    kind 'unit': |p| in [0.5, 2]; the scaled gradient, the first moment and sqrt(v) of a run that has taken t - 1 steps on
                 gradients of size c = 1e-3 (|g s| in c [0.5, 2], m = bc1(t) x the same with the gradient's sign, v =
                 bc2(t) c^2 [0.25, 4]): the update is lr x [1/8, 8] on every element, so a wrong decay, step count, scale or
                 moment moves p, v or m by far more than ``bound`` (tests/test_adamw_cpu.py shows it for every case)
         'wide': |g|, |m|, sqrt(v) log-uniform over 1e-12 .. 1e12 with independent signs, |p| log-uniform over 1e-3 .. 10
         'zero': g = 0 and v = 0 (m = 0): the update is exactly 0 and p takes only its decay
    Padding segments always hold g = v = m = 0."""

    def __init__(self, name, table, m_form='b1=0.9', t=3, lr=0.05, eps=1e-8, grad_scale=0.5, kind='unit', seed=0):
        self.name, self.table, self.m_form, self.t, self.lr, self.eps = name, table, m_form, t, lr, eps
        self.grad_scale, self.kind, self.seed = grad_scale, kind, seed
        self.betas, self.store_m = M_FORMS[m_form]
        self.ends, self.seg_wd, self.seg_pad = table['ends'], table['wd'], table['pad']
        self.n = int(self.ends[-1])
        sizes = np.diff(np.concatenate([[0], self.ends]))
        self.seg_of = np.repeat(np.arange(len(sizes)), sizes)         # element -> segment
        self.wd = self.seg_wd[self.seg_of]                            # per element, float32
        self.pad = self.seg_pad[self.seg_of]

    def __repr__(self):
        return self.name

    def hyper(self, lr=None):
        return dict(lr=self.lr if lr is None else lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, t=self.t,
                    grad_scale=self.grad_scale)

    def inputs(self):
        """dict p, g, m (None when not stored), v: float32 arrays"""
        rng = np.random.default_rng(1000 + self.seed)
        n = self.n
        sign = rng.choice([-1.0, 1.0], n)
        if self.kind == 'wide':
            def mag(lo, hi):
                return 10.0 ** rng.uniform(lo, hi, n)
            p = rng.choice([-1.0, 1.0], n) * mag(-3, 1)
            g = sign * mag(-12, 12)
            m = rng.choice([-1.0, 1.0], n) * mag(-12, 12)
            v = mag(-12, 12) ** 2
        else:
            c = 1e-3
            bc1, bc2 = bias_corrections(*self.betas, max(self.t - 1, 1))
            p = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)
            g = sign * c * rng.uniform(0.5, 2.0, n) / self.grad_scale
            m = sign * c * rng.uniform(0.5, 2.0, n) * (bc1 if self.betas[0] else 1.0)
            v = bc2 * c * c * rng.uniform(0.25, 4.0, n)
            if self.kind == 'zero':
                g, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
        for a in (g, m, v):
            a[self.pad] = 0.0
        out = dict(p=p.astype(F), g=g.astype(F), m=m.astype(F) if self.store_m else None, v=v.astype(F))
        return out

    def neighbour_wd(self, shift):
        """the decay mistake: every element takes the decay of the segment before (shift -1) or after (+1) its own.
        Returns (wd, hit, boundary): ``hit`` marks the elements that have such a segment, ``boundary`` -- a subset -- those whose
        neighbour i + shift lies in another segment."""
        seg = self.seg_of + shift
        hit = (seg >= 0) & (seg < len(self.seg_wd))
        wd = self.wd.copy()
        wd[hit] = self.seg_wd[seg[hit]]
        idx = np.arange(self.n) + shift
        ok = (idx >= 0) & (idx < self.n)
        boundary = np.zeros(self.n, dtype=bool)
        boundary[ok] = self.seg_of[idx[ok]] != self.seg_of[ok]
        assert not (boundary & ~hit).any()
        return wd, hit, boundary


def table_cases():
    """tables x first-moment forms (the GPU test crosses these with the pointer alignments)"""
    return [Case(f'{tn}-{mf}', fn(), m_form=mf, seed=i) for i, (tn, fn) in enumerate(TABLES.items()) for mf in M_FORMS]


def length_cases():
    return [Case(f'n={n}-{mf}', table_single(n), m_form=mf, seed=50 + n % 97) for n in LENGTHS for mf in ('b1=0,m=null', 'b1=0.9')]


def t_cases():
    return [Case(f't={t}-{mf}', table_residues(), m_form=mf, t=t, seed=100 + k) for k, t in enumerate(T_VALUES) for mf in M_FORMS]


def scale_cases():
    return [Case(f's={s}-{mf}', table_residues(), m_form=mf, grad_scale=s, seed=200 + k) for k, s in enumerate(SCALES)
            for mf in ('b1=0,m=null', 'b1=0.9')]


def magnitude_cases():
    out = []
    for k, mf in enumerate(M_FORMS):
        for t in (1, 10):
            out.append(Case(f'wide-t={t}-{mf}', table_residues(), m_form=mf, t=t, kind='wide', seed=300 + k))
        out.append(Case(f'wide-lr=2e-3-{mf}', table_flat(), m_form=mf, t=1000, lr=2e-3, kind='wide', seed=310 + k))
        out.append(Case(f'zero-{mf}', table_flat(), m_form=mf, kind='zero', seed=320 + k))
    return out


def all_cases():
    return table_cases() + length_cases() + t_cases() + scale_cases() + magnitude_cases()


def check(case, x, got_p, got_v, got_m, skip=None):
    """teacher-forced comparison of a float32 result with step64 from the state ``x`` (Case.inputs()).  Returns
    (ok, ratios): ``ok`` whether every element lies within ``bound`` (exactly equal where the bound is 0), ``ratios`` the worst
    error / bound of p, v, m (m: None when not stored).  ``skip``: elements left out (their reference is non-finite)."""
    res = step64(x['p'], x['g'], x['m'], x['v'], case.wd, **case.hyper())
    bp, bv, bm = bound(res['A'], res['U'], res['v'], res['M'])
    keep = np.ones(case.n, dtype=bool) if skip is None else ~np.asarray(skip)
    ok, ratios = True, {}
    for name, got, ref, b in (('p', got_p, res['p'], bp), ('v', got_v, res['v'], bv), ('m', got_m, res['m'], bm)):
        if got is None:
            ratios[name] = None
            continue
        with np.errstate(invalid='ignore'):
            err = np.abs(np.asarray(got, dtype=np.float64) - ref)[keep]
        b = b[keep]
        assert np.isfinite(ref[keep]).all() and np.isfinite(b).all(), (case, name, 'the reference is not finite')
        ok = ok and bool((err <= b).all())
        pos = b > 0
        ratios[name] = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
        if (err[~pos] > 0).any():
            ratios[name] = math.inf
    return ok, ratios
