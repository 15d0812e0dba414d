"""The numpy restatement of ``learner.weight_decay`` (a0_weight_decay), and the oracle's learner with the decay in front of its Adam step.

The kernel's arithmetic per element:  t = fl32(c32 * p),  p_new = fl32(p - t),  c32 = lr * lambda formed in double and rounded to fp32 ONCE.
numpy's float32 arithmetic rounds every operation to nearest-even and keeps denormals, as the kernel does, so ``decay`` is the kernel byte for byte.
The statistic: workgroup b of P = 256 owns [b * chunk, (b + 1) * chunk) and leaves the float64 sum of the squares of the values it read; a float's square is exact
in float64 and the terms are non-negative, so any summation order of m terms is within relative m * 2^-53 of the exact sum.
"""
import math

import numpy as np

P = 256                            # A0_GRAD_NORM_PARTIALS
C_MIN = 2.0 ** -24


def coef32(lr, lam) -> np.float32:
    """c as the kernel sees it: the double product rounded to fp32 once (Python floats are doubles)."""
    return np.float32(float(lr) * float(lam))


def decay(p: np.ndarray, c) -> np.ndarray:
    """p - fl32(c32 * p) in float32: one rounded product, one rounded subtraction."""
    p = np.asarray(p, np.float32)
    c32 = np.float32(c)
    t = (c32 * p).astype(np.float32)
    return (p - t).astype(np.float32)


def chunk_of(n: int) -> int:
    """The floats one workgroup owns: a multiple of four, a function of n alone (a0_grad_norm_partials' split)."""
    return ((n + P - 1) // P + 3) // 4 * 4


def partials_f64(p: np.ndarray) -> np.ndarray:
    """The P float64 sums of squares over the chunks of p (0 for an empty chunk)."""
    p = np.asarray(p, np.float32).astype(np.float64)
    ch = chunk_of(p.size)
    return np.array([math.fsum((p[b * ch:(b + 1) * ch] ** 2).tolist()) for b in range(P)], np.float64)


def norm_of(partials) -> float:
    """The trainer's finish: the sum in index order, the square root in double."""
    total = 0.0
    for x in np.asarray(partials, np.float64).tolist():
        total += x
    return math.sqrt(total)


def decayed_oracle(OracleLearner):
    """The oracle's learner whose Adam step is preceded by p <- p * (1 - lr * lambda) on everything Adam owns (float32 tensors, torch's arithmetic) — what
    ``torch.optim.AdamW`` does.  A NaN-skipped update never reaches the optimizer, so it decays nothing."""
    import torch

    class _DecayThenStep:
        def __init__(self, inner, c):
            self.inner, self.c = inner, c

        def step(self, params, grads):
            with torch.no_grad():
                for v in params.values():
                    v.mul_(1.0 - self.c)
            return self.inner.step(params, grads)

        def __getattr__(self, name):
            return getattr(self.inner, name)

    class DecayedOracleLearner(OracleLearner):
        def __init__(self, *a, c, **kw):
            super().__init__(*a, **kw)
            self.adam = _DecayThenStep(self.adam, float(c))

    return DecayedOracleLearner
