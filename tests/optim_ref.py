"""Float64 references, error bounds and cases of the optimizer and step-state kernels (csrc/optim.hip: every Adam form, a0_rmsprop_step and its clip
coefficient, a0_target_sync, the loss mean's ring slot; csrc/update_tail.h: a0_step_decide / a0_step_publish): the yardstick of
tests/test_gpu_optim_reference.py, itself held to torch.optim.Adam and torch.optim.RMSprop in float64, the oracle's Adam and RMSprop,
torch.nn.utils.clip_grad_norm_, CpuOps' status words and a hand-written table by tests/test_optim_reference_helpers.py.

No import of the library.  Every reference takes the fp32 inputs and the fp32 constants exactly as the kernel receives them — (float)(1 - b1), (float)b2,
(float)(1 - b2), (float)eps, the two scalars as fp32 numbers — and evaluates the formula in float64 in its most literal form.  Every reference returns its
bounds beside its values; their derivation is in the GPU test's docstring.  ``*32`` are fp32 restatements of the kernels' two arithmetic forms, statement
by statement (the helper test holds them to half of every bound), and ``WRONG_*`` the mistakes the bounds must reject."""
from __future__ import annotations

import math

import numpy as np

import recipe
from actor_tail_cases import U, mean_rows_tol
from value_loss_ref import TINY

F32 = np.float32
MARGIN = 2.0                             # every element bound is twice its count of roundings: a literal fp32 evaluation sits within half of it
SECOND_ORDER = 1.0 + 2.0 ** -20          # products of two first-order terms, which the counts leave out
HP = dict(lr=5e-4, b1=0.9, b2=0.999)
EPS_VALUES = (1e-2 / 32, 1e-8)           # the project's value at B = 32, and torch's default
RMS = dict(lr=5e-4 / 2e4, alpha=0.95, eps=1e-5)


def f32(x) -> float:
    return float(F32(x))


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def hyper(b1, b2, eps, exact=False):
    """The constants of an Adam element as the kernels receive them (a0_adam_hyper_of); ``exact``: in double, for the comparisons with torch in float64."""
    r = (lambda x: x) if exact else f32
    return dict(w1=r(1.0 - b1), b2=r(b2), w2=r(1.0 - b2), eps=r(eps))


# ------------------------------------------------------------------------------------------------ the step's bookkeeping (a0_step_decide, a0_step_publish)
def step_decide(state, extra, lr, b1, b2, target_freq):
    """What one update decides from state[0] (NaN flag), state[1] (update_steps before it), state[7] (the count at the last reset) and the extra flag."""
    skip = int(int(state[0]) != 0 or (extra is not None and float(extra) != 0.0))
    steps = int(state[1]) + (0 if skip else 1)
    t = max(1, steps - int(state[7]))
    return dict(skip=skip, steps=steps, t=t, sync=int(target_freq > 0 and steps % target_freq == 0),
                step_size=f32(lr / (1.0 - math.pow(b1, float(t)))), bc2_sqrt=f32(math.sqrt(1.0 - math.pow(b2, float(t)))))


def step_update(state, extra, lr, b1, b2, target_freq, form):
    """One update's effect on the status words ``state`` (a list of 8 ints, changed in place) -> the decision.  ``form``: "plain" (the one-thread prep kernel
    commits: a0_adam_step, a0_adam_step_sync, a0_adam_step_sync_clip), "folded" (a0_adam_step_sync_wt: the count waits in state[5] for the weight-copy
    refresh to commit it) or "tail" (the tail-prep launch files state[5] and commits).  The last two leave the same words."""
    assert form in ("plain", "folded", "tail")
    S = step_decide(state, extra, lr, b1, b2, target_freq)
    if S["skip"]:
        state[2] += 1
    state[3], state[4] = S["skip"], S["sync"]
    if form != "plain":
        state[5] = S["steps"]
    state[1], state[0] = S["steps"], 0
    return S


def within_one_ulp(got, want) -> bool:
    got, want = F32(got), F32(want)
    return bool(abs(float(got) - float(want)) <= float(np.spacing(np.abs(want))))


# twelve consecutive updates: (how the NaN flag is raised, the value written into state[7] in front of the update, target_update_freq)
SCHEDULE = (
    (None, None, 3), (None, None, 3), (None, None, 3), ("state", None, 3), (None, None, 0), ("extra", None, 1),
    (None, None, 1), (None, 5, 3), (None, None, 3), (None, 9, 0), ("both", None, 3), (None, None, 3),
)


def schedule_flags(kind, has_extra):
    """(raise state[0], the extra flag's value or None) of a SCHEDULE entry; an entry family without an extra flag raises state[0] instead."""
    if kind is None:
        return False, (0.0 if has_extra else None)
    if not has_extra:
        return True, None
    return kind in ("state", "both"), (1.0 if kind in ("extra", "both") else 0.0)


# ------------------------------------------------------------------------------------------------ Adam's element
def adam64(p, m, v, g, H, step_size, bc2_sqrt, coef=None, coef_roundings=0):
    """oracle/learner.py:Adam.step (torch.optim.Adam, single tensor) on one element, in float64:
        m' = m + (g - m) w1;  v' = v b2 + w2 g g;  denom = sqrt(v') / bc2_sqrt + eps;  p' = p - step_size m' / denom
    with g c in place of g when ``coef`` is given (the fp32 coefficient of the clip form).  ``coef_roundings``: fp32 roundings between the reference's
    coefficient and the kernel's.  -> dict p, m, v, denom, r = m' / denom and the bounds e_p, e_m, e_v."""
    p, m, v, g = _f64(p), _f64(m), _f64(v), _f64(g)
    w1, b2, w2, eps = (float(H[k]) for k in ("w1", "b2", "w2", "eps"))
    ss, bc2 = float(step_size), float(bc2_sqrt)
    with np.errstate(all="ignore"):
        if coef is None:
            gc, e_g = g, np.zeros_like(g)
        else:
            gc = g * float(coef)
            e_g = (1 + coef_roundings) * U * np.abs(gc) + np.where((gc != 0) & (np.abs(gc) < 2.0 ** -120), TINY, 0.0)
        m1 = m + (gc - m) * w1
        v1 = v * b2 + w2 * gc * gc
        root = np.sqrt(v1)
        denom = root / bc2 + eps
        r = m1 / denom
        p1 = p - ss * r
        # the counts (the GPU test's docstring); every one relative to the magnitude named there
        e_m = 3 * U * (np.abs(m) + np.abs(gc)) + 2 * TINY + w1 * e_g
        e_v = 3 * U * v1 + 3 * TINY + 2 * w2 * np.abs(gc) * e_g
        hi = np.sqrt(v1 + e_v)
        e_root = np.maximum(root - np.sqrt(np.maximum(v1 - e_v, 0.0)), hi - root) + U * hi
        e_denom = e_root / bc2 + U * (root / bc2) + U * denom + TINY
        e_r = (e_m + np.abs(r) * e_denom) / (denom - e_denom) + U * np.abs(r) + TINY
        e_p = ss * e_r + U * (np.abs(p1) + ss * np.abs(r)) + TINY
    k = MARGIN * SECOND_ORDER
    return dict(p=p1, m=m1, v=v1, denom=denom, r=r, e_p=k * e_p, e_m=k * e_m, e_v=k * e_v)


def fma32(a, b, c):
    """The fused multiply-add of fp32 operands: the float64 product (exact) plus the addend, rounded once."""
    with np.errstate(all="ignore"):
        return (_f64(a) * _f64(b) + _f64(c)).astype(F32)


def adam32(p, m, v, g, H, step_size, bc2_sqrt, form, coef=None):
    """a0_adam_wide ("wide") and a0_adam_scalar ("scalar"), statement by statement in numpy fp32 -> (p', m', v')."""
    p, m, v, g = (np.asarray(x, F32) for x in (p, m, v, g))
    w1, b2, w2, eps, ss, bc2 = (F32(x) for x in (H["w1"], H["b2"], H["w2"], H["eps"], step_size, bc2_sqrt))
    with np.errstate(all="ignore"):
        gi = g if coef is None else (g * F32(coef)).astype(F32)
        if form == "wide":
            mi = fma32(gi - m, w1, m)
            vi = fma32(w2 * gi, gi, v * b2)
        else:
            mi = m + (gi - m) * w1
            vi = v * b2 + (w2 * gi) * gi
        denom = np.sqrt(vi) / bc2 + eps
        return fma32(-ss, mi / denom, p), mi, vi


def _wrong_adam(change):
    def run(p, m, v, g, H, ss, bc2, t, coef=None):
        p, m, v, g = _f64(p), _f64(m), _f64(v), _f64(g)
        w1, b2, w2, eps = H["w1"], H["b2"], H["w2"], H["eps"]
        gc = g if coef is None else g * float(coef)
        with np.errstate(all="ignore"):
            if change == "bc2_dropped":
                bc2 = 1.0
            if change == "bc_at_t_minus_1":
                ss, bc2 = HP["lr"] / (1.0 - HP["b1"] ** (t - 1)), math.sqrt(1.0 - HP["b2"] ** (t - 1))
            m1 = (1.0 - w1) * m + gc if change == "m_not_scaled" else m + (gc - m) * w1
            v1 = v * b2 + (b2 if change == "b2_for_w2" else w2) * gc * gc
            denom = np.sqrt(v1 + eps) / bc2 if change == "eps_in_root" else np.sqrt(v1) / bc2 + eps
            m_step = m + (g - m) * w1 if change == "step_on_unclipped" else m1
            return p - ss * m_step / denom, m1, v1
    return run


# name -> f(p, m, v, g, H, step_size, bc2_sqrt, t, coef) -> (p', m', v'): each a plausible mistake in an Adam kernel
WRONG_ADAM = {k: _wrong_adam(k) for k in ("bc2_dropped", "bc_at_t_minus_1", "eps_in_root", "b2_for_w2", "m_not_scaled", "step_on_unclipped")}


# ------------------------------------------------------------------------------------------------ RMSprop and its clip coefficient
def clip_coef64(g, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (||g|| + 1e-6)) in float64, max_norm and 1e-6 as the fp32 the kernel holds
    -> (coefficient, ||g||, relative bound on the unclamped quotient, the unclamped quotient): a0_clip_coef_kernel sums n non-negative squares in fp32, ceil(n / 256) sequential
    adds per lane, then an eight-step tree — (ceil(n / 256) + 8 + 1) U relative on the sum, half of it on the norm — and rounds the norm's square root,
    the sum with 1e-6 and the quotient."""
    g = _f64(g)
    n = g.size
    norm = math.sqrt(float((g * g).sum()))
    c = f32(max_norm) / (norm + f32(1e-6))
    rel = (0.5 * ((n + 255) // 256 + 9) + 3) * U * SECOND_ORDER
    return min(1.0, c), norm, rel, c


def clip_coef32(sumsq, max_norm):
    """The coefficient of the Adam clip forms from the sum of their double partials, as a0_adam_sync_kernel forms it: the norm rounded to fp32 once, then
    min(1, max_norm / (norm + 1e-6)) in fp32 -> (coefficient, norm), both fp32 numbers."""
    norm = F32(math.sqrt(sumsq))
    c = F32(max_norm) / (norm + F32(1e-6))
    return float(min(c, F32(1))), float(norm)


CLIP_MAX_NORM = 1.0
CLIP_SUMSQ = {"coef<1": 4.0, "coef==1": 0.25}        # the partials' sum: a norm of 2 (coefficient just below 1/2) and of 1/2 (1.99..., held to exactly 1)
CLIP_ROUNDINGS = 2                                   # norm + 1e-6 and the quotient, should a device round either differently


def rmsprop64(p, sq, g, lr, alpha, eps, coef=None, exact=False):
    """oracle/learner.py:RMSprop.step (torch.optim.RMSprop: no momentum, not centred) on one element, in float64, on g c when ``coef`` (an fp32 number) is given:
        s' = s alpha + (1 - alpha) g g;  p' = p - lr g / (sqrt(s') + eps)
    lr, alpha, (1 - alpha) and eps as the fp32 the kernel receives (``exact``: in double, for the comparison with torch in float64).  -> dict p, sq and the
    bounds e_p, e_sq; one bound for both contractions."""
    p, sq, g = _f64(p), _f64(sq), _f64(g)
    lr, al, w, eps = (lr, alpha, 1.0 - alpha, eps) if exact else (f32(lr), f32(alpha), f32(1.0 - alpha), f32(eps))
    with np.errstate(all="ignore"):
        if coef is None:
            gc, e_g = g, np.zeros_like(g)
        else:
            gc = g * float(F32(coef))
            e_g = U * np.abs(gc) + np.where((gc != 0) & (np.abs(gc) < 2.0 ** -120), TINY, 0.0)
        s1 = sq * al + w * gc * gc
        root = np.sqrt(s1)
        denom = root + eps
        r = gc / denom
        p1 = p - lr * r
        e_s = 3 * U * s1 + 3 * TINY + 2 * w * np.abs(gc) * e_g
        hi = np.sqrt(s1 + e_s)
        e_root = np.maximum(root - np.sqrt(np.maximum(s1 - e_s, 0.0)), hi - root) + U * hi
        e_denom = e_root + U * denom
        e_r = (e_g + np.abs(r) * e_denom) / (denom - e_denom) + U * np.abs(r) + TINY
        e_p = lr * e_r + U * lr * np.abs(r) + TINY + U * np.abs(p1)
    k = MARGIN * SECOND_ORDER
    return dict(p=p1, sq=s1, e_p=k * e_p, e_sq=k * e_s)


def rmsprop32(p, sq, g, lr, alpha, eps, contract, coef=None):
    """a0_rmsprop_kernel statement by statement in numpy fp32, with the compiler's contraction off or on (the products that feed an addition fused) -> (p', s')."""
    p, sq, g = (np.asarray(x, F32) for x in (p, sq, g))
    lr, al, w, eps = F32(lr), F32(alpha), F32(1.0 - alpha), F32(eps)
    with np.errstate(all="ignore"):
        gi = g if coef is None else (g * F32(coef)).astype(F32)
        if contract:
            s = fma32(w * gi, gi, sq * al)
            return fma32(-lr, gi / (np.sqrt(s) + eps), p), s
        s = sq * al + (w * gi) * gi
        return p - lr * (gi / (np.sqrt(s) + eps)), s


def _wrong_rmsprop(change):
    def run(p, sq, g, lr, alpha, eps):
        p, sq, g = _f64(p), _f64(sq), _f64(g)
        lr, al, w, eps = f32(lr), f32(alpha), f32(1.0 - alpha), f32(eps)
        s1 = sq * al + w * g * g
        if change == "eps_in_root":
            return p - lr * g / np.sqrt(s1 + eps), s1
        return p - lr * g / (np.sqrt(sq) + eps), s1
    return run


WRONG_RMSPROP = {k: _wrong_rmsprop(k) for k in ("eps_in_root", "old_square_average")}


RMSPROP_NS = (1, 255, 256, 257, 100384, 2048 * 256 + 5)       # one lane; either side of one workgroup; the fraction net; a second grid-stride trip
RMSPROP_CLIPS = ("off", "inactive", "active")


def rmsprop_case(n, zero_p, zero_sq):
    """p, sq [n] (exactly 0, or at 0.05 / 0.01 scale) and the gradients of three consecutive steps (0.1 scale, every 97th element exactly 0 where n > 1)."""
    gen = recipe.gen(600 + n % 1000 + 2 * zero_p + zero_sq)
    p = np.zeros(n, F32) if zero_p else (0.05 * gen.standard_normal(n)).astype(F32)
    sq = np.zeros(n, F32) if zero_sq else np.abs(1e-2 * gen.standard_normal(n)).astype(F32)
    gs = []
    for step in range(3):
        g = (0.1 * gen.standard_normal(n)).astype(F32)
        g[::97] = 0.0
        if n == 1:
            g[0] = (0.1, -0.2, 0.3)[step]
        gs.append(g)
    return p, sq, gs


def rmsprop_max_norm(g, clip):
    """max_grad_norm of a RMSPROP_CLIPS entry for the gradient g: none, one the norm stays below (coefficient exactly 1), one a quarter of the norm."""
    norm = float(np.sqrt((_f64(g) ** 2).sum()))
    return {"off": -1.0, "inactive": 2.0 * norm + 1.0, "active": 0.25 * norm + 1e-3}[clip]


# ------------------------------------------------------------------------------------------------ the loss mean
def loss_mean64(loss):
    """(mean, bound) of the per-sample losses: the reduction of a0_mean_rows_kernel over one row (mean_rows_tol of actor_tail_cases)."""
    x = _f64(loss)
    return float(x.mean()), float(mean_rows_tol(x.size, np.abs(x).mean()))


# ------------------------------------------------------------------------------------------------ value cases
# (steps before the update, state[7]) -> t = max(1, steps + 1 - state[7]): 1, 2, 10, 1000, 10^7 (b1^t underflows), the count equal to the reset's (t clamps
# to 1), one step behind the reset, and the second step after a reset
T_CASES = {"t=1": (0, 0), "t=2": (1, 0), "t=10": (9, 0), "t=1000": (999, 0), "t=1e7": (10 ** 7 - 1, 0), "steps==reset": (49, 50), "steps==reset-1": (48, 50),
           "reset+2": (51, 50)}
TABLE_N = 4096
_TABLE = {}


def _log_uniform(g, k, lo, hi):
    return np.exp2(g.uniform(lo, hi, k))


def _sign(g, k):
    return np.where(g.random(k) < 0.5, -1.0, 1.0)


def _draw(g, kinds, k):
    """k elements (p, m, v, g) of the kinds (p, m, v, g); m's kinds "eq" and "opp" follow g."""
    kp, km, kv, kg = kinds
    gr = {"ord": lambda: 0.1 * g.standard_normal(k), "0": lambda: np.zeros(k), "-0": lambda: -np.zeros(k), "2^-70": lambda: _sign(g, k) * 2.0 ** -70,
          "wide": lambda: _sign(g, k) * _log_uniform(g, k, -70, 60)}[kg]()
    p = {"ord": lambda: 0.05 * g.standard_normal(k), "0": lambda: np.zeros(k), "big": lambda: 1e3 * g.standard_normal(k)}[kp]()
    m = {"ord": lambda: 1e-3 * g.standard_normal(k), "0": lambda: np.zeros(k), "eq": lambda: gr.copy(), "opp": lambda: -gr * g.uniform(0.5, 2.0, k),
         "wide": lambda: _sign(g, k) * _log_uniform(g, k, -70, 55)}[km]()
    v = {"ord": lambda: np.abs(1e-3 * g.standard_normal(k)), "0": lambda: np.zeros(k), "denormal": lambda: 2.0 ** -149 * g.integers(1, 2 ** 22, k),
         "2^-126": lambda: np.full(k, 2.0 ** -126), "wide": lambda: _log_uniform(g, k, -126, 110)}[kv]()
    return [np.asarray(x, np.float64).astype(F32) for x in (p, m, v, gr)]


TABLE_KINDS = [(kp, km, kv, kg) for kp in ("ord", "0", "big") for km in ("0", "eq", "opp", "wide") for kv in ("0", "denormal", "2^-126", "wide")
               for kg in ("0", "-0", "2^-70", "wide", "ord")]
ORDINARY = ("ord", "ord", "ord", "ord")


def adam_table():
    """p, m, v, g [TABLE_N] fp32 and ``kinds``, the kinds of every element.  Every combination of TABLE_KINDS is planted twice over (two draws), each time
    as one element of a 16-byte group of otherwise ordinary values (at a position that rotates) and as a whole group of its own; ordinary values fill the
    rest.  Computed once and never written."""
    if not _TABLE:
        g = recipe.gen(31000)
        cols = [[], [], [], []]
        kinds = []
        for rep in range(2):
            for c, kd in enumerate(TABLE_KINDS):
                one, rest, own = _draw(g, kd, 1), _draw(g, ORDINARY, 4), _draw(g, kd, 4)
                at = (c + rep) % 4
                for j in range(4):
                    rest[j][at] = one[j][0]
                    cols[j] += [rest[j], own[j]]
                kinds += [kd if e == at else ORDINARY for e in range(4)] + [kd] * 4
        fill = _draw(g, ORDINARY, TABLE_N - len(kinds))
        arrs = [np.concatenate(cols[j] + [fill[j]]) for j in range(4)]
        kinds += [ORDINARY] * (TABLE_N - len(kinds))
        assert all(a.size == TABLE_N and a.dtype == F32 for a in arrs)
        for a in arrs:
            a.setflags(write=False)
        _TABLE.update(p=arrs[0], m=arrs[1], v=arrs[2], g=arrs[3], kinds=kinds)
    return _TABLE


# the non-finite table: one element of g per group at +inf, -inf, NaN, at every position of a 16-byte group, ordinary values elsewhere
NONFINITE = tuple((4 * (3 * pos + k) + pos, val) for pos in range(4) for k, val in enumerate((float("inf"), float("-inf"), float("nan"))))


def nonfinite_table():
    """p, m, v, g [64] of ordinary values (computed once), and NONFINITE: the (index, value) pairs planted one at a time into g."""
    if "nf" not in _TABLE:
        arrs = _draw(recipe.gen(31001), ORDINARY, 64)
        for a in arrs:
            a.setflags(write=False)
        _TABLE["nf"] = dict(p=arrs[0], m=arrs[1], v=arrs[2], g=arrs[3])
    return _TABLE["nf"]


def value_class(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    x = _f64(x)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def worst(name, got, ref, bound, inputs):
    """(fraction of the bound the worst element uses, a message with that element's inputs): what a failing comparison prints."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    with np.errstate(all="ignore"):
        frac = np.abs(got - ref) / bound
    frac = np.where(np.isfinite(got) & np.isfinite(frac), frac, np.inf)
    i = int(frac.argmax())
    ins = ", ".join(f"{k} {float(np.asarray(a).reshape(-1)[i] if np.ndim(a) else a)!r}" for k, a in inputs.items())
    return float(frac[i]), f"{name}[{i}]: got {got[i]!r} want {ref[i]!r} bound {bound[i]:.3e} ({frac[i]:.3f} of it); {ins}"
