"""Float64 restatement of the guarded optimizer step (csrc/optim.hip: vqk_step_guard + vqk_adamw_guarded; optim.py:
FlatAdamW.enable_guard), independent of the product code.

  verdict      torch.amp.GradScaler's rule -- an optimizer step whose gradients hold an Inf / NaN is left out and the optimizer's
               step count does not advance -- and torch.nn.utils.clip_grad_norm_'s rule -- with total_norm the 2-norm of all
               gradients, clip_coef = min(1, max_norm / (total_norm + 1e-6)) multiplies every gradient.  The norm is taken over
               the finite elements (with skipping on, a step that has others is not taken at all).
  adamw_step   torch.optim.AdamW (decoupled decay, no amsgrad), one step t on float64 arrays, weight decay per element.
  GuardedAdamW the two together over a sequence of steps, with the counters the device state block keeps.

tests/test_stepguard_cpu.py checks this file against torch.optim.AdamW + clip_grad_norm_ on CPU float64 tensors."""
import math

import numpy as np


def arena_row(g, scale=1.0, mask=None):
    """{sum x^2, max |x|, nonfinite} of x = g * scale over the elements selected by ``mask`` (all when None), float64"""
    x = np.asarray(g, dtype=np.float64) * float(scale)
    if mask is not None:
        x = x[np.asarray(mask, dtype=bool)]
    finite = np.isfinite(x)
    xf = x[finite]
    return float(math.fsum(xf * xf)), float(np.abs(xf).max()) if xf.size else 0.0, float((~finite).sum())


def verdict(sumsq, nonfinite, skip_nonfinite=True, max_norm=None):
    """(apply, coef, norm)"""
    norm = math.sqrt(sumsq)
    apply = not (skip_nonfinite and nonfinite > 0)
    coef = 1.0
    if max_norm is not None and max_norm > 0:
        coef = min(1.0, max_norm / (norm + 1e-6))
    return apply, coef, norm


def eff_scale(grad_scale, coef):
    """the float32 gradient scale the kernel multiplies with: (float)((double)grad_scale * coef)"""
    return np.float32(float(np.float32(grad_scale)) * coef)


def adamw_step(p, g, m, v, wd, lr, b1, b2, eps, t):
    """in place on float64 arrays; ``wd`` per element (or a scalar); ``m`` may be None when b1 == 0"""
    p *= 1.0 - lr * wd
    if m is None:
        mv = g
    else:
        m *= b1
        m += (1.0 - b1) * g
        mv = m
    v *= b2
    v += (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    p -= (lr / bc1) * mv / (np.sqrt(v) / math.sqrt(bc2) + eps)


class GuardedAdamW:
    def __init__(self, p, wd, lr, betas, eps, skip_nonfinite=True, max_norm=None, store_m=True):
        self.p = np.array(p, dtype=np.float64)
        self.wd = np.broadcast_to(np.asarray(wd, dtype=np.float64), self.p.shape).copy()
        self.v = np.zeros_like(self.p)
        self.m = np.zeros_like(self.p) if (store_m or betas[0] != 0.0) else None
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.skip_nonfinite, self.max_norm = bool(skip_nonfinite), max_norm
        self.applied = self.skipped = self.clipped = self.run = self.max_run = 0
        self.coef_sum, self.coef_min, self.last_norm = 0.0, 1.0, 0.0

    def step(self, g, grad_scale=1.0, lr=None, mask=None):
        """one guarded step on the gradient ``g``; ``mask`` selects the elements that count for the verdict (the device leaves the
        alignment padding out).  Returns (apply, coef)."""
        sumsq, _, nonfinite = arena_row(g, grad_scale, mask)
        apply, coef, norm = verdict(sumsq, nonfinite, self.skip_nonfinite, self.max_norm)
        self.last_norm = norm
        if not apply:
            self.skipped += 1
            self.run += 1
            self.max_run = max(self.max_run, self.run)
            return apply, coef
        self.applied += 1
        self.run = 0
        self.clipped += coef < 1.0
        self.coef_sum += coef
        self.coef_min = min(self.coef_min, coef)
        scale = float(grad_scale) * coef
        adamw_step(self.p, np.asarray(g, dtype=np.float64) * scale, self.m, self.v, self.wd, self.lr if lr is None else float(lr),
                   self.betas[0], self.betas[1], self.eps, self.applied)
        return apply, coef

    def state_block(self):
        """the eight doubles of the device state block (include/vqk.h: VQK_GUARD_*)"""
        return [float(self.applied), float(self.skipped), float(self.clipped), float(self.run), float(self.max_run), self.coef_sum,
                self.coef_min, self.last_norm]
