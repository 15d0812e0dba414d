"""actor.eps_ladder restated in float64, shared by tests/test_eps_ladder_config.py (CPU) and tests/test_gpu_eps_ladder.py (the kernels).  No import of the library.

Environment i of N acts with eps^(1 + alpha i / (N - 1)), eps the scheduled scalar as the fp32 the device receives.  Three edges are exact by definition, not by
rounding: eps >= 1 stays eps (the schedule's all-random warm-up), eps <= 0 gives 0, environment 0 (and a lone environment) keeps eps."""
import numpy as np


def ladder64(eps, alpha, i0, E, n_total):
    """float64 values of environments i0 .. i0 + E - 1 of n_total; eps and alpha are taken as fp32, like the kernel's arguments."""
    eps, alpha = np.float64(np.float32(eps)), np.float64(np.float32(alpha))
    i = np.arange(i0, i0 + E, dtype=np.float64)
    if not eps > 0:
        return np.zeros(E)
    if eps >= 1 or n_total <= 1:
        return np.full(E, eps)
    out = np.power(eps, 1.0 + alpha * i / np.float64(n_total - 1))
    out[i == 0] = eps
    return out


def ladder32(eps, alpha, i0, E, n_total):
    """The same rounded to fp32 once: what the device must give, up to the rounding boundary (1 ulp)."""
    return ladder64(eps, alpha, i0, E, n_total).astype(np.float32)


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two non-negative fp32 arrays (their bit patterns are ordered like their values)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
