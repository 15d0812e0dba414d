"""The float64 reference of ``learner.target_tau`` (a0_target_blend), and the oracle's learner with its target sync replaced by the Polyak step.

The kernel's arithmetic per element:  t_new = fmaf(tau32, fl32(p - t), t),  tau32 = tau rounded to fp32 once.
The reference evaluates t + tau32 * fl32(p - t) in float64: the product of two floats is exact there, the sum is rounded once (to 53 bits), and the cast to fp32
rounds a second time.  That double rounding differs from the fused multiply-add's single one only when the float64 sum was inexact AND landed exactly half way
between two floats; ``double_rounding_suspects`` finds those elements on the CPU, from the inputs alone (Knuth's TwoSum gives the float64 sum's error exactly).
"""
from collections import OrderedDict

import numpy as np


def tau32(tau) -> np.float32:
    """tau as the kernel sees it: rounded to fp32 ONCE (a Python float is a double)."""
    return np.float32(float(tau))


def blend_terms(t: np.ndarray, p: np.ndarray, tau):
    """(t as float64, the exact float64 product tau32 * fl32(p - t))."""
    t, p = np.asarray(t, np.float32), np.asarray(p, np.float32)
    d = (p - t).astype(np.float32)                     # one rounded fp32 subtraction
    return t.astype(np.float64), np.float64(tau32(tau)) * d.astype(np.float64)


def blend_f64(t: np.ndarray, p: np.ndarray, tau) -> np.ndarray:
    """The float64 value of t + tau32 * fl32(p - t)."""
    a, x = blend_terms(t, p, tau)
    return a + x


def blend_nearest(t: np.ndarray, p: np.ndarray, tau) -> np.ndarray:
    """The fp32 nearest to ``blend_f64``."""
    return blend_f64(t, p, tau).astype(np.float32)


def double_rounding_suspects(t: np.ndarray, p: np.ndarray, tau) -> np.ndarray:
    """True where the float64 sum is inexact and its rounded value is a tie between two floats: the only elements at which the correctly rounded fused
    multiply-add may differ (by one ulp) from ``blend_nearest``."""
    a, x = blend_terms(t, p, tau)
    s = a + x
    bb = s - a
    err = (a - (s - bb)) + (x - bb)                    # TwoSum: a + x == s + err exactly
    low = s.view(np.uint64) & np.uint64((1 << 29) - 1)     # the 29 mantissa bits a float does not keep (normal range)
    return (err != 0) & (low == np.uint64(1 << 28))


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Number of floats between a and b (0 when equal; +0 and -0 coincide)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def polyak_oracle(OracleLearner):
    """The oracle's learner with ``target <- online`` replaced by ``target <- target + tau * (online - target)`` (float32 tensors, torch's arithmetic), at the same
    updates: when update_steps % target_update_freq == 0 after the update, a NaN-skipped one included."""
    import torch

    class PolyakOracleLearner(OracleLearner):
        def __init__(self, *a, tau, **kw):
            super().__init__(*a, **kw)
            self.tau, self.period = float(tau), self.target_update_freq
            self.target_update_freq = 1 << 62          # the parent never copies (update_steps stays below it)

        def train(self, *a, **kw):
            # update_steps == 0 would satisfy the parent's test (0 % f == 0): it can only be 0 after a NaN-skipped first update, which no walk here makes
            res = super().train(*a, **kw)
            assert self.update_steps > 0
            if self.update_steps % self.period == 0:
                tau = torch.tensor(tau32(self.tau))
                with torch.no_grad():
                    self.pt = OrderedDict((k, (v + tau * (self.po[k].detach() - v)) if v.is_floating_point() else v.clone()) for k, v in self.pt.items())
            return res

    return PolyakOracleLearner
