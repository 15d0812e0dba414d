"""Float64 reference, error bound and cases of the Munchausen-IQN quantile targets (a0_miqn_target, ``learner.iqn.munchausen``): the yardstick of
tests/test_gpu_miqn.py, itself held to a literal torch restatement of the paper's target, to closed forms and to six wrong computations by
tests/test_miqn_reference_helpers.py.  No import of the library.

The target (Vieillard, Pietquin, Geist 2020, section 5 and appendix B), per sample, from the target network's quantiles z'_j(a) on s' and z_j(a) on s at the
same N' fractions, element (b, j, a) at b*sb + j*sj + a*sa of the flat fp32 inputs:

    Qm'(a) = (sum_j z'_j(a)) / N',  Qm(a) = (sum_j z_j(a)) / N'
    lp(x)_a = (x_a - max x) - tau log sum_k exp((x_k - max x) / tau)
    pi'_a   = exp((Qm'_a - max) / tau) / sum_k exp((Qm'_k - max) / tau)
    m       = alpha clamp(lp(Qm)_{a_b}, lo, 0)
    y_j     = r + m + gamma_n (1 - d) sum_a pi'_a (z'_j(a) - lp(Qm')_a)

``miqn_target64`` evaluates it in float64 from the fp32 inputs, gamma_n, tau, alpha and lo rounded to fp32 as the entry point receives them, and returns with y
the bound e_y [B][N'] on an fp32 evaluation, derived stage by stage in the manner of value_loss_ref.mdqn64 / lp_err (u = 2^-24, one fp32 rounding):

  mean      n = N' values summed one after the other (n - 1 roundings of partial sums below sum |z|) and divided by N' (one more): at most (N' + 1) u mean_j|z_j(a)|
            =: e_x(a); d_a, |d_a| <= e_x(a), is the error of action a's mean.
  inputs    lp and log pi = lp / tau do not change when one number is taken off every x_k, so it does not matter which maximum the kernel subtracts: the means'
            errors reach log pi_a as (d_a - sum_k pi~_k d_k) / tau = sum_{k != a} pi~_k (d_a - d_k) / tau with pi~ the softmax at a point between the two arguments,
            pi~_k <= pi_k exp(2 max_k e_x(k) / tau).  So e_in(a) = exp(2 max e_x / tau) sum_{k != a} pi_k (e_x(a) + e_x(k)) / tau.  The mean's error enters the
            exponent DIVIDED BY TAU: at tau = 0.03 it is 33 times what it was.  This is the conditioning of the formula, not slack — any fp32 evaluation that forms
            the mean first has it — and it vanishes only where the policy is one-hot on a (no other action carries weight to compare against).  lp_a carries tau e_in(a).
  exponent  z = x - max rounds once (u |z|), the quotient z / tau once more (u |z / tau|).
  exp       relative error EXPF_REL (the project's recorded figure, doubled) + expm1 of the exponent's error =: rel_e; a result below 2^-126 may be flushed: TINY.
  sum       five butterfly stages among the 32 lanes of a half-wave: 5 u; with the pi-weighted mean of rel_e this is rel_s.
  log       LOGF_BOUND (recorded on arguments in [1, 64]; the sum lies in [1, 32]) + rel_s + A TINY.
  lp        e_lp(a) = tau e_in(a) + u |z_a| + tau (rel_s + LOGF_BOUND + A TINY) + 2 u (|z_a| + tau lse)      (the product tau * log and the subtraction).
  pi'       relative: expm1(e_in(a)) + rel_e(a) + rel_s + u (the division); absolute TINY beside it.
  product   pi'_a (z'_j(a) - lp'_a): the bracket carries e_lp(a) + u |bracket|, the product one rounding more.
  sum_a     A additions in action order: (A - 1) u sum_a pi'_a |bracket|.
  bonus     the clamp is 1-Lipschitz and continuous, so an fp32 log-policy on the other side of a seam moves m by no more than its own error: no case is left out at
            lo or at 0.  e_m = alpha e_lp(Qm)(a_b) + u |m|.
  y         g = gamma_n (1 - d) rounds twice, g * sum once, r + m once, the last addition once: 5 u (|r| + |m| + g sum_a pi'_a |bracket|) on top of e_m + g e_sum.

A NaN or an infinity among a sample's inputs: every y_j of that sample is NaN (``nan_rows`` says which samples)."""
from __future__ import annotations

import numpy as np

import recipe
from actor_tail_cases import EXPF_REL, U
from value_loss_ref import LOGF_BOUND, TINY, log_softmax_tau64

SHAPES = ((1, 1, 1), (3, 1, 2), (5, 7, 3), (4, 64, 18), (2, 65, 32), (3, 200, 6))      # (B, N', A)
LAYOUTS = ("bja", "baj")                  # the two the library uses: (N' A, A, 1) — iqn / fqf — and (A T, 1, T) — qr
TAUS = (0.03, 1.0)
ALPHA, LO, GAMMA = 0.9, -1.0, 0.99 ** 3
KINDS = ("tie", "gap10", "argmax", "below_lo", "done", "random")


def strides(layout, Nd, A):
    """(sb, sj, sa) of element (b, j, a)."""
    return (Nd * A, A, 1) if layout == "bja" else (A * Nd, 1, Nd)


def laid_out(z, layout):
    """z [B][N'][A] -> the flat fp32 array of that layout."""
    z = np.asarray(z, np.float32)
    return np.ascontiguousarray(z if layout == "bja" else z.transpose(0, 2, 1)).reshape(-1)


def gather(flat, sb, sj, sa, B, Nd, A):
    """The flat fp32 input -> [B][N'][A] (float32)."""
    idx = (np.arange(B)[:, None, None] * sb + np.arange(Nd)[None, :, None] * sj + np.arange(A)[None, None, :] * sa)
    return np.asarray(flat, np.float32).reshape(-1)[idx]


def _f64(x):
    return np.asarray(x, np.float64)


def _rows(x, idx):
    return x[np.arange(x.shape[0]), np.asarray(idx, np.int64)]


def _lp_parts(z32, tau):
    """Of the values z32 [B][N'][A] a log-policy is taken of the mean of: (mean [B][A], lp [B][A], pi [B][A], e_lp [B][A], rel_pi [B][A])."""
    z = _f64(z32)
    Nd, A = z.shape[1], z.shape[2]
    x = z.sum(1) / Nd
    e_x = (Nd + 1) * U * np.abs(z).mean(1)
    zz = x - x.max(-1, keepdims=True)
    a = zz / tau
    ex = np.exp(a)
    s = ex.sum(-1, keepdims=True)
    pi = ex / s
    lse = np.log(s)
    lp = zz - tau * lse
    # what the means' errors do to log pi_a = lp_a / tau: sum_{k != a} pi~_k |d_a - d_k| / tau, pi~ <= pi exp(2 max e_x / tau)
    spread = (pi[:, None, :] * (e_x[:, :, None] + e_x[:, None, :]) * (1.0 - np.eye(A))[None]).sum(-1)          # [B][a]: sum over k != a
    e_in = np.exp(2 * e_x.max(-1, keepdims=True) / tau) * spread / tau
    # what the evaluation adds: the subtraction and the quotient in the exponent, expf, the butterfly, logf
    rel_e = EXPF_REL + np.expm1(U * np.abs(zz) / tau + U * np.abs(a))
    rel_s = (pi * rel_e).sum(-1, keepdims=True) + 5 * U + A * TINY
    e_lp = tau * e_in + U * np.abs(zz) + tau * (rel_s + LOGF_BOUND + A * TINY) + 2 * U * (np.abs(zz) + tau * lse)
    return x, lp, pi, e_lp, np.expm1(e_in) + rel_e + rel_s + U


def miqn_target64(q_next, q_cur, sb, sj, sa, act, rew, done, gamma_n, tau, alpha, lo, B, Nd, A):
    """-> dict(y [B][N'], e_y [B][N'], nan_rows [B] bool, and the parts: q_next_mean, q_cur_mean, lp_next, lp_cur, pi, m).  The docstring of this module has the
    formulas and the derivation of e_y."""
    gam, tau, alpha, lo = (float(np.float32(v)) for v in (gamma_n, tau, alpha, lo))
    zn32, zc32 = gather(q_next, sb, sj, sa, B, Nd, A), gather(q_cur, sb, sj, sa, B, Nd, A)
    nan_rows = ~(np.isfinite(zn32).reshape(B, -1).all(1) & np.isfinite(zc32).reshape(B, -1).all(1))
    zn32, zc32 = zn32.copy(), zc32.copy()
    zn32[nan_rows], zc32[nan_rows] = 0.0, 0.0              # evaluated on zeros, overwritten with NaN below
    with np.errstate(under="ignore"):
        xn, lpn, pi, e_lpn, rel_pi = _lp_parts(zn32, tau)
        xc, lpc, _, e_lpc, _ = _lp_parts(zc32, tau)
    r, dn = _f64(np.asarray(rew, np.float32)).reshape(B), _f64(np.asarray(done, np.float32)).reshape(B)
    m = alpha * np.clip(_rows(lpc, act), lo, 0.0)
    e_m = alpha * _rows(e_lpc, act) + U * np.abs(m)
    g = gam * (1.0 - dn)
    br = _f64(zn32) - lpn[:, None, :]                                                          # [B][N'][A]
    w = pi[:, None, :] * np.abs(br)
    v = (pi[:, None, :] * br).sum(-1)                                                         # [B][N']
    e_v = (w * (rel_pi[:, None, :] + 2 * U) + pi[:, None, :] * e_lpn[:, None, :] + TINY * np.abs(br)).sum(-1) + (A - 1) * U * w.sum(-1) + A * TINY
    y = r[:, None] + m[:, None] + g[:, None] * v
    S = np.abs(r)[:, None] + np.abs(m)[:, None] + np.abs(g)[:, None] * w.sum(-1)
    e_y = e_m[:, None] + np.abs(g)[:, None] * e_v + 5 * U * S + TINY
    y[nan_rows] = np.nan
    return dict(y=y, e_y=e_y, nan_rows=nan_rows, q_next_mean=xn, q_cur_mean=xc, lp_next=lpn, lp_cur=lpc, pi=pi, m=m)


# ------------------------------------------------------------------------------------------------ wrong computations (the helper test: each lies > 100 e_y away somewhere)
def variant64(name, zn32, zc32, zon32, act, rew, done, gamma_n, tau, alpha, lo):
    """y [B][N'] of a wrong computation from z' , z (target) and zon (the ONLINE network on s) [B][N'][A]:
    temp1 — softmax at temperature 1 (mdqn's); no_alpha — alpha dropped; tau_again — tau multiplied in again (Q17: tau in alpha's place);
    no_lp — the - lp' term dropped; per_fraction — a policy per fraction instead of the mean's; online_bonus — the online values for the bonus."""
    gam, tau, alpha, lo = (float(np.float32(v)) for v in (gamma_n, tau, alpha, lo))
    zn, zc, zo = _f64(zn32), _f64(zc32), _f64(zon32)
    B, Nd, A = zn.shape
    r, dn = _f64(rew).reshape(B, 1), _f64(done).reshape(B, 1)
    xn, xc = zn.mean(1), (zo if name == "online_bonus" else zc).mean(1)
    lpn, lpc = log_softmax_tau64(xn, tau), log_softmax_tau64(xc, tau)
    pi = np.exp(log_softmax_tau64(xn, tau) / tau) if name != "temp1" else np.exp(log_softmax_tau64(xn, 1.0))
    bonus = np.clip(_rows(lpc, act), lo, 0.0)[:, None]
    m = {"no_alpha": bonus, "tau_again": tau * bonus}.get(name, alpha * bonus)
    if name == "per_fraction":
        lpj = log_softmax_tau64(zn, tau)                                                      # over the actions of every fraction
        v = (np.exp(lpj / tau) * (zn - lpj)).sum(-1)
    elif name == "no_lp":
        v = (pi[:, None, :] * zn).sum(-1)
    else:
        v = (pi[:, None, :] * (zn - lpn[:, None, :])).sum(-1)
    return r + m + gam * (1.0 - dn) * v


VARIANTS = ("temp1", "no_alpha", "tau_again", "no_lp", "per_fraction", "online_bonus")


# ------------------------------------------------------------------------------------------------ cases
_CASES = {}


def case(B, Nd, A, tau):
    """z' , z, zon [B][N'][A] (fp32), act, rew, done of one shape and temperature (computed once; never modified).  Sample b is of kind KINDS[(b + shift) % 6],
    shift chosen per shape so that the six shapes meet every kind (``planted`` maps sample -> kind; with A == 1 a kind changes nothing but done):
      tie       two actions' quantiles bit-identical on s' and on s, and the best of the sample
      gap10     the best action's mean 10 above the others' on s': at tau = 0.03 every other exponential underflows to 0 and pi' is one-hot
      argmax    the taken action is the clear maximum on s: its log-policy is about 0, the bonus at the upper seam
      below_lo  the taken action 60 tau (at least 3) below the maximum on s: its log-policy is below lo, the bonus at the lower seam
      done      done = 1"""
    key = (B, Nd, A, tau)
    if key in _CASES:
        return _CASES[key]
    g = recipe.gen(12000 + 131 * B + 17 * Nd + A + int(1000 * tau))
    mk = lambda: (g.standard_normal((B, 1, A)) * 0.7 + g.standard_normal((B, Nd, A)) * 0.5).astype(np.float32)
    zn, zc, zo = mk(), mk(), mk()
    act = g.integers(0, A, B).astype(np.int32)
    act[0] = A - 1
    act[-1] = 0 if B > 1 else act[-1]
    rew = g.standard_normal(B).astype(np.float32)
    done = np.zeros(B, np.float32)
    shift = SHAPES.index((B, Nd, A)) if (B, Nd, A) in SHAPES else 0
    planted = {}
    for b in range(B):
        kind = KINDS[(b + shift) % len(KINDS)]
        planted[b] = kind
        a = int(act[b])
        o = (a + 1) % A
        if kind == "done":
            done[b] = 1.0
        if A == 1:
            continue
        if kind == "tie":
            zn[b, :, o], zc[b, :, o] = zn[b, :, a], zc[b, :, a]
            lift_n = np.float32(max(0.0, float(zn[b].mean(0).max() - zn[b, :, a].mean())) + 0.25)
            lift_c = np.float32(max(0.0, float(zc[b].mean(0).max() - zc[b, :, a].mean())) + 0.25)
            zn[b, :, a] += lift_n
            zn[b, :, o] = zn[b, :, a]
            zc[b, :, a] += lift_c
            zc[b, :, o] = zc[b, :, a]
        elif kind == "gap10":
            top = int(zn[b].mean(0).argmax())
            zn[b, :, top] += np.float32(10.0 + float(np.delete(zn[b].mean(0), top).max() - zn[b, :, top].mean()) + 0.5)
        elif kind == "argmax":
            zc[b, :, a] += np.float32(float(zc[b].mean(0).max() - zc[b, :, a].mean()) + max(40 * tau, 2.0))
        elif kind == "below_lo":
            zc[b, :, a] -= np.float32(float(zc[b, :, a].mean() - np.delete(zc[b].mean(0), a).max()) + max(60 * tau, 3.0))
    c = dict(q_next=zn, q_cur=zc, q_online=zo, act=act, rew=rew, done=done, planted=planted, tau=tau)
    _CASES[key] = c
    return c
