"""The float64 restatement of ``learner.iqn.risk``'s distortions (Dabney et al. 2018, section 4) that tests/test_gpu_iqn_risk.py holds the kernels to;
tests/test_iqn_risk_reference_helpers.py pins it on the CPU before any device run.  No scipy: ``math.erfc`` and an inverse normal CDF refined by Newton steps on
``erfc``.

    cvar   eta tau                                                                   0 < eta <= 1
    pow    eta >= 0: tau^(1 / (1 + |eta|));  eta < 0: 1 - (1 - tau)^(1 / (1 + |eta|))     |eta| <= 64
    cpw    tau^eta / (tau^eta + (1 - tau)^eta)^(1 / eta)                             0 < eta <= 1
    wang   Phi(Phi^-1(tau) + eta),  beta(0) = 0                                      |eta| <= 8

The device tolerance, derived (``spacing32``).  The kernel forms pow / cpw / wang in double from the same (double)tau and eta and rounds to fp32 ONCE.  Let x be
the exact value, x_d the kernel's double and x_r this file's.  The double-side functions (pow, erfc, the inverse normal CDF) are accurate to a few units in the
last place of double, u = 2^-53, and the formulas amplify an input error by a condition number kappa:
  * pow:  kappa <= 1 (an exponent in (0, 1]); 1 - (1 - tau)^e loses nothing relative to the result, because 1 - tau is exact for tau = k 2^-24;
  * cpw:  kappa <= 1 / eta for the outer power — 20 at eta = 0.05, the smallest the tests use;
  * wang: d beta / beta = (phi / Phi)(z + eta) dz <= (|z + eta| + 1) dz with |z| <= 5.30 on the 2^-24 grid and |eta| <= 8: kappa < 15 * 5.30 < 100, and erfc
          keeps its RELATIVE accuracy in the lower tail (which 1 + erf would not).
So |x_d - x| and |x_r - x| are below 10 * 100 * u |x| ~ 1e-13 |x|, while one fp32 spacing at x is at least 2^-24 |x| ~ 6e-8 |x| (more for a denormal result).
Rounding x_d to fp32 adds at most half a spacing: |fl32(x_d) - x_r| <= s / 2 + 2e-13 |x| < s.  The double-side error is five orders below the rounding, so the
bound is ONE fp32 spacing at the float64 value, and only where x lies within 1e-13 |x| of a rounding midpoint can fl32(x_d) differ from fl32(x_r) at all.
cvar is one fp32 multiply: numpy float32 gives its bits, the tolerance is zero.
"""
import math

import numpy as np

KINDS = {"neutral": 0, "cvar": 1, "pow": 2, "cpw": 3, "wang": 4}
PAPER_ETA = {"cvar": (0.25, 0.1), "pow": (-2.0,), "cpw": (0.71,), "wang": (0.75, -0.75)}
# the ends of each range as the tests take them; cpw's lower end is open, 0.05 is where its condition number 1 / eta (above) is still 20
RANGE_ENDS = {"cvar": (2.0 ** -20, 1.0), "pow": (-64.0, 0.0, 64.0), "cpw": (0.05, 1.0), "wang": (-8.0, 8.0)}
EDGES = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)
_SQRT2 = math.sqrt(2.0)

# Acklam's rational approximation of the inverse normal CDF (relative error 1.15e-9), the starting point of the Newton steps below
_A = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00)
_B = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
_C = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00)
_D = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)


def ncdf(u: float) -> float:
    """Phi(u) = erfc(-u / sqrt 2) / 2: relative accuracy in the lower tail."""
    return 0.5 * math.erfc(-u / _SQRT2)


def _acklam(p: float) -> float:
    if p < 0.02425:
        q = math.sqrt(-2.0 * math.log(p))
        return (((((_C[0] * q + _C[1]) * q + _C[2]) * q + _C[3]) * q + _C[4]) * q + _C[5]) / ((((_D[0] * q + _D[1]) * q + _D[2]) * q + _D[3]) * q + 1.0)
    q = p - 0.5
    r = q * q
    return (((((_A[0] * r + _A[1]) * r + _A[2]) * r + _A[3]) * r + _A[4]) * r + _A[5]) * q / (((((_B[0] * r + _B[1]) * r + _B[2]) * r + _B[3]) * r + _B[4]) * r + 1.0)


def ncdfinv(p: float) -> float:
    """Phi^-1(p), 0 < p < 1.  The upper half is solved as the lower half of 1 - p (exact for p = k 2^-24), so that the tail keeps its relative accuracy; three
    Newton steps z <- z - (Phi(z) - p) / phi(z) on erfc take Acklam's 1e-9 to the last places of double."""
    if not (0.0 < p < 1.0):
        return -math.inf if p == 0.0 else math.inf if p == 1.0 else math.nan
    if p > 0.5:
        return -ncdfinv(1.0 - p)
    if p == 0.5:
        return 0.0
    z = _acklam(p)
    for _ in range(3):
        z -= (ncdf(z) - p) / (math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
    return z


def beta(kind: str, eta: float, tau: float) -> float:
    """beta(tau) in float64, tau in [0, 1); no rounding to fp32, no clamp (none of the four leaves [0, 1])."""
    if kind == "neutral":
        return tau
    if kind == "cvar":
        return eta * tau
    if tau == 0.0:
        return 0.0
    if kind == "pow":
        e = 1.0 / (1.0 + abs(eta))
        return math.pow(tau, e) if eta >= 0 else 1.0 - math.pow(1.0 - tau, e)
    if kind == "cpw":
        a, b = math.pow(tau, eta), math.pow(1.0 - tau, eta)
        return a / math.pow(a + b, 1.0 / eta)
    if kind == "wang":
        return ncdf(ncdfinv(tau) + eta)
    raise ValueError(kind)


def beta_array(kind: str, eta: float, taus) -> np.ndarray:
    """``beta`` over fp32 fractions, as float64."""
    return np.array([beta(kind, float(eta), float(t)) for t in np.asarray(taus, dtype=np.float32).astype(np.float64)], dtype=np.float64)


def cvar_f32(eta: float, taus) -> np.ndarray:
    """cvar as the kernel forms it: eta rounded to fp32 once, one fp32 multiply."""
    return (np.float32(eta) * np.asarray(taus, dtype=np.float32)).astype(np.float32)


def spacing32(x) -> np.ndarray:
    """One fp32 spacing AT the float64 value x (not at its fp32 rounding): 2^(e - 24) for |x| in [2^(e - 1), 2^e), and the denormal spacing 2^-149 below 2^-126."""
    m, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.where(m == 0, -149, np.maximum(e - 24, -149)))


def fractions(n: int, seed: int = 20181) -> np.ndarray:
    """The edge fractions followed by random k 2^-24, n in all (cut short where n is smaller), fp32."""
    k = np.random.default_rng(seed).integers(0, 1 << 24, size=max(n, 0))
    t = np.concatenate([np.array(EDGES, dtype=np.float64), k.astype(np.float64) * 2.0 ** -24])[:n]
    return t.astype(np.float32)
