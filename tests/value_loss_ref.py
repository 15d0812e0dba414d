"""Float64 references, error bounds and cases of the value and categorical losses (a0_loss_dqn, a0_dqn_head_loss, a0_loss_mdqn, a0_loss_c51): the yardstick of
tests/test_gpu_value_loss_reference.py, itself held to the G4 fixture, the oracle in float64, F.smooth_l1_loss, torch.autograd and a finite difference by
tests/test_value_loss_reference_helpers.py.

No import of the library.  Every function takes the fp32 inputs exactly as the kernel receives them and evaluates the formula of oracle/losses.py in float64
in its most literal form (the lines are cited at each function).  The one discontinuous decision, the smooth-L1 branch, is taken on the fp32 difference the
reference itself would form (torch fp32 on the CPU, ``*_d32``); both branches and both slopes meet at |d| = 1, so a kernel whose own fp32 d falls on the
other side of the seam differs by the square of its error only, and seams are planted, not avoided.  The categorical projection is continuous and
piecewise linear in the bin position: it is evaluated wholly in float64 and its bound carries the bin position's error (``c51_bounds``).  The bounds'
derivation is in the GPU test's docstring; the figures they take from measurements are EXPF_REL (actor_tail_cases) and LOGF_BOUND below."""
from __future__ import annotations

import numpy as np

import recipe
from actor_tail_cases import EXPF_REL, U, check_spread, head_roundings, tie_pair
from util import qhead64

TINY = 2.0 ** -126                       # below it fp32 loses its relative precision (or flushes to 0): an absolute allowance per term
# logf on the device, largest |logf(s) - log(s)| against the float64 logarithm of the same fp32 argument s, measured on an MI355X by
# test_logf_error_stays_within_the_recorded_figure over 99 700 arguments in [1, 64]: 6.19e-7 at s = 62.238 (1.3 ulp of log s; profiles/r12_value_loss_accuracy.md).
# The bounds take LOGF_BOUND: twice the figure (1.24e-6), rounded up to a power of two (1.91e-6); the test fails if a device exceeds it.
LOGF_MEASURED = 6.2e-7
LOGF_BOUND = 2.0 ** -19


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _rows(x, idx):
    return x[np.arange(x.shape[0]), np.asarray(idx, np.int64)]


# ------------------------------------------------------------------------------------------------ smooth L1 (F.smooth_l1_loss, losses.py:77, 87)
def smooth_l1(d, d32):
    """(loss, slope) of d in float64, the branch |d| < 1 taken on the fp32 difference ``d32``: 0.5 d^2 with slope d, else |d| - 0.5 with slope sign(d)."""
    d = _f64(d)
    quad = np.abs(np.asarray(d32, np.float32)) < np.float32(1)
    return np.where(quad, 0.5 * d * d, np.abs(d) - 0.5), np.where(quad, d, np.sign(d))


def _value_loss(q_a, y, y32, wgt, act, A):
    """d = q - y, the loss and dq = w slope at the taken action ([B][A], 0 elsewhere) from a target y and the reference's fp32 target y32."""
    q32 = np.asarray(q_a, np.float32)
    d = _f64(q32) - y
    d32 = (q32 - np.asarray(y32, np.float32)).astype(np.float32)
    loss, slope = smooth_l1(d, d32)
    dq = np.zeros((len(d), A))
    dq[np.arange(len(d)), np.asarray(act, np.int64)] = _f64(wgt) * slope
    return d, d32, loss, slope, dq


# ------------------------------------------------------------------------------------------------ DQN (losses.py:71-77)
def dqn_y32(qn, rew, done, gamma_n):
    """y as torch forms it in fp32: rewards + gamma_n * (1 - terminals) * q_next (the python scalar joins as fp32, one rounding per operation)."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    return (t(rew) + gamma_n * (1 - t(done)) * t(qn)).numpy()


def dqn64(q, q_next, A, act, a_star, rew, done, wgt, gamma_n, B):
    """losses.py:75-77 per sample: y = r + gamma_n (1 - done) q'(a*), loss = smooth_l1(q(a) - y); dq = w slope at a.  gamma_n enters as the fp32 the entry
    point receives.  Returns a dict: y, d, d32, loss, slope, dq [B][A], S = |q(a)| + |r| + gamma_n |q'(a*)| (the magnitude d works at)."""
    qa, qn = _rows(np.asarray(q, np.float32).reshape(B, A), act), _rows(np.asarray(q_next, np.float32).reshape(B, A), a_star)
    gam = float(np.float32(gamma_n))
    r, dn = _f64(rew).reshape(B), _f64(done).reshape(B)
    y = r + gam * (1.0 - dn) * _f64(qn)
    d, d32, loss, slope, dq = _value_loss(qa, y, dqn_y32(qn, rew, done, gam), wgt, act, A)
    return dict(y=y, d=d, d32=d32, loss=loss, slope=slope, dq=dq, S=np.abs(_f64(qa)) + np.abs(r) + gam * np.abs(_f64(qn)))


def dqn_bounds(ref, wgt, c_d=5.0, e_in=0.0):
    """(loss, dq at the taken action).  d carries c_d roundings of S (1 - done, its product with gamma_n, the product with q', the sum with r, q - y) and
    whatever its inputs bring (``e_in``); the loss moves by d's error times max(|d|, 1) and rounds twice itself; dq = w clamp(d) is 1-Lipschitz in d and
    rounds once."""
    e_d = c_d * U * ref["S"] + e_in
    return e_d * np.maximum(np.abs(ref["d"]), 1.0) + 2 * U * ref["loss"], np.abs(_f64(wgt)) * (e_d + U * np.abs(ref["slope"]))


# ------------------------------------------------------------------------------------------------ Munchausen DQN (losses.py:62-64, 80-87)
def log_softmax_tau64(x, tau):
    """losses.py:62-64: z - tau logsumexp(z / tau), z = x - max(x), over the last axis."""
    x = _f64(x)
    z = x - x.max(-1, keepdims=True)
    return z - tau * np.log(np.exp(z / tau).sum(-1, keepdims=True))


def softmax64(x):
    x = _f64(x)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def mdqn_y32(q_next, q_cur, act, rew, done, gamma_n, tau, lo):
    """losses.py:82-85 in torch fp32."""
    import torch
    from oracle.losses import log_softmax_tau
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    ql, qc = t(q_next), t(q_cur)
    v_next = (ql.softmax(dim=-1) * (ql - log_softmax_tau(ql, tau))).sum(dim=-1)
    add_on = log_softmax_tau(qc, tau)[torch.arange(ql.shape[0]), torch.from_numpy(np.asarray(act, np.int64))].clamp(lo, 0)
    return (t(rew) + tau * add_on + gamma_n * (1 - t(done)) * v_next).numpy()


def mdqn64(q, q_next, q_cur, A, act, rew, done, wgt, gamma_n, tau, lo, B):
    """losses.py:82-87 per sample: v_next = sum_a softmax(q')_a (q'_a - lp(q')_a) with the softmax at temperature 1, add_on = clamp(lp(q_cur)_a, lo, 0),
    y = r + tau add_on + gamma_n (1 - done) v_next.  tau, lo and gamma_n enter as the fp32 the entry point receives.  Besides dqn64's entries the dict
    holds v_next, add_on, lp_next, lp_cur and e_y, the bound on an fp32 evaluation of y (mdqn_bounds adds q - y)."""
    tau, lo, gam = float(np.float32(tau)), float(np.float32(lo)), float(np.float32(gamma_n))
    qn32, qc32 = np.asarray(q_next, np.float32).reshape(B, A), np.asarray(q_cur, np.float32).reshape(B, A)
    qn, qc = _f64(qn32), _f64(qc32)
    qa = _rows(np.asarray(q, np.float32).reshape(B, A), act)
    r, dn = _f64(rew).reshape(B), _f64(done).reshape(B)
    lpn, lpc = log_softmax_tau64(qn, tau), log_softmax_tau64(qc, tau)
    p = softmax64(qn)
    term = qn - lpn
    v_next = (p * term).sum(-1)
    add_on = np.clip(_rows(lpc, act), lo, 0.0)
    y = r + tau * add_on + gam * (1.0 - dn) * v_next

    # the bound on y, stage by stage (the GPU test's docstring); x: the A values a log-policy is taken of.  The inputs are exact fp32 values, so z = x - max
    # rounds by u |z| (nothing at all between neighbours), and the quotient z / tau once more
    def lp_err(x):
        z = x - x.max(-1, keepdims=True)
        a = z / tau
        pi = np.exp(a)
        pi /= pi.sum(-1, keepdims=True)
        lse = np.log(np.exp(a).sum(-1, keepdims=True))
        e_lse = EXPF_REL + 2 * U * (pi * np.abs(a)).sum(-1, keepdims=True) + (A - 1) * U + LOGF_BOUND + TINY
        return U * np.abs(z) + tau * e_lse + 2 * U * (np.abs(z) + tau * lse)

    e_lpn, e_lpc = lp_err(qn), lp_err(qc)
    zn = np.abs(qn - qn.max(-1, keepdims=True))
    rel_p = 2 * EXPF_REL + U * (zn + (p * zn).sum(-1, keepdims=True)) + A * U
    e_v = (p * (rel_p * np.abs(term) + e_lpn + U * (np.abs(qn) + np.abs(lpn)))).sum(-1) + (A + 1) * U * (p * np.abs(term)).sum(-1) + A * TINY
    v_abs = (p * np.abs(term)).sum(-1)
    S_y = np.abs(r) + tau * np.abs(add_on) + gam * v_abs
    e_y = tau * _rows(e_lpc, act) + gam * (1.0 - dn) * e_v + 5 * U * S_y
    d, d32, loss, slope, dq = _value_loss(qa, y, mdqn_y32(qn32, qc32, act, rew, done, gam, tau, lo), wgt, act, A)
    return dict(y=y, d=d, d32=d32, loss=loss, slope=slope, dq=dq, S=np.abs(_f64(qa)) + S_y, v_next=v_next, add_on=add_on, lp_next=lpn, lp_cur=lpc, e_y=e_y)


def mdqn_bounds(ref, wgt):
    return dqn_bounds(ref, wgt, c_d=1.0, e_in=ref["e_y"])


# ------------------------------------------------------------------------------------------------ C51 (losses.py:90-117)
def c51_project64(prob_next, rew, done, atoms, gamma_n, vmin, vmax, with_parts=False, fixup1=True, fixup2=True):
    """losses.py:90-102 in float64: tz = clamp(r + gamma_n (1 - done) z, vmin, vmax), b = (tz - vmin) / delta, lo = floor b, up = ceil b, the two fix-ups
    (up > 0 and lo == up: lo - 1; then lo < n - 1 and lo == up: up + 1) and the two scatter-adds m[lo] += p (up - b), m[up] += p (b - lo).  delta is the
    float64 quotient (vmax - vmin) / (n - 1); b is at most n - 1 in exact arithmetic and is held to it (a quotient rounded upwards would otherwise ask for
    bin n: the contract is that every index lies in [0, n)).  ``fixup1`` / ``fixup2`` = False leave a fix-up out (for the negative controls only)."""
    p = _f64(prob_next)
    B, n = p.shape
    gam = float(np.float32(gamma_n))
    z = _f64(np.asarray(atoms, np.float32)).reshape(1, n)
    r, dn = _f64(rew).reshape(B, 1), _f64(done).reshape(B, 1)
    vmin, vmax = float(np.float32(vmin)), float(np.float32(vmax))
    delta = (vmax - vmin) / (n - 1)
    tz = np.clip(r + gam * (1.0 - dn) * z, vmin, vmax)
    b = np.minimum((tz - vmin) / delta, n - 1.0)
    lo, up = np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)
    if fixup1:
        lo = np.where((up > 0) & (lo == up), lo - 1, lo)
    if fixup2:
        up = np.where((lo < n - 1) & (lo == up), up + 1, up)
    m = np.zeros((B, n))
    rows = np.broadcast_to(np.arange(B)[:, None], (B, n))
    np.add.at(m, (rows, lo), p * (up - b))
    np.add.at(m, (rows, up), p * (b - lo))
    return (m, b, delta) if with_parts else m


def c51_loss64(logits_a, m):
    """losses.py:115-116: -(m * log_softmax(logits at the taken action)).sum(-1); returns (loss, logp, softmax)."""
    x = _f64(logits_a)
    z = x - x.max(-1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(-1, keepdims=True))
    return -(m * logp).sum(-1), logp, np.exp(logp)


def c51_64(logits, tgt_logits, A, T, act, a_star, rew, done, wgt, atoms, gamma_n, vmin, vmax, B):
    """The whole of a0_loss_c51: p = softmax(target logits at a*), m = c51_project64(p), loss, and dlogits = w (softmax sum(m) - m) at the taken action
    ([B][A][T], 0 elsewhere), with the bounds of c51_bounds."""
    x = np.asarray(logits, np.float32).reshape(B, A, T)
    xt = np.asarray(tgt_logits, np.float32).reshape(B, A, T)
    xa, xs = _f64(_rows(x, act)), _f64(_rows(xt, a_star))
    p = softmax64(xs)
    m, b, delta = c51_project64(p, rew, done, atoms, gamma_n, vmin, vmax, with_parts=True)
    loss, logp, po = c51_loss64(xa, m)
    w = _f64(wgt).reshape(B, 1)
    g = w * (po * m.sum(-1, keepdims=True) - m)
    dl = np.zeros((B, A, T))
    dl[np.arange(B), np.asarray(act, np.int64)] = g
    ref = dict(p=p, m=m, b=b, delta=delta, loss=loss, logp=logp, po=po, g=g, dlogits=dl, mass=m.sum(-1), xa=xa, xs=xs, w=w)
    ref.update(c51_bounds(ref, rew, done, atoms, gamma_n, vmin))
    return ref


POS_ROUNDINGS = 6.0                      # gamma_n (1 - done), its product with z, the sum with r (or one fused multiply-add), tz - vmin, the division, fl32(delta)


def _softmax_rel(x, p):
    """Relative error bound [B][T] of an fp32 softmax with one lane per element: expf (EXPF_REL) of x - max, whose rounding u |x - max| moves the exponent;
    the denominator carries the p-weighted mean of the same, six butterfly stages and the division one more."""
    dz = np.abs(x - x.max(-1, keepdims=True))
    return 2 * EXPF_REL + U * (dz + (p * dz).sum(-1, keepdims=True)) + 7 * U


def c51_projection_bounds(p, xs, m, b, delta, rew, atoms, gamma_n, vmin):
    """(E [B][T] per atom, tol_m [B][T] per bin, tol_mass [B], the additions' share of tol_m) of an fp32 projection of p = softmax(xs) against
    c51_project64's m, b, delta."""
    B, T = p.shape
    gam = float(np.float32(gamma_n))
    z = np.abs(_f64(np.asarray(atoms, np.float32))).reshape(1, T)
    r = np.abs(_f64(rew)).reshape(B, 1)
    E = POS_ROUNDINGS * U * (r + gam * z + abs(float(np.float32(vmin)))) / delta              # [B][T] per atom k
    rel_p = _softmax_rel(_f64(xs), p)
    j = np.arange(T).reshape(1, 1, T)
    near = (np.abs(b[:, :, None] - j) < 1.0 + E[:, :, None]) & (p[:, :, None] >= TINY)        # [B][k][j]: atom k may send mass to bin j
    sliver = (near * (p * E)[:, :, None]).sum(1)                                               # sum over the near atoms of p_k E_k
    count = near.sum(1)
    rel_near = (near * rel_p[:, :, None]).max(1)
    m_abs = m + sliver
    acc = np.maximum(count - 1, 0) * U * m_abs                                                 # additions of non-zero terms into bin j
    tol_m = sliver + m_abs * (rel_near + 2 * U) + acc + T * TINY
    # the mass: (up - b) + (b - lo) = up - lo = 1 whatever b is, so the position's error does not reach it
    tol_mass = (p * (rel_p + 2 * U)).sum(-1) + acc.sum(-1) + T * T * TINY
    return E, tol_m, tol_mass


def c51_bounds(ref, rew, done, atoms, gamma_n, vmin):
    """Bounds on m [B][T], the mass sum_j m_j [B], the loss [B] and dlogits at the taken action [B][T] (the GPU test's docstring derives them)."""
    p, m = ref["p"], ref["m"]
    B, T = p.shape
    E, tol_m, tol_mass = c51_projection_bounds(p, ref["xs"], m, ref["b"], ref["delta"], rew, atoms, gamma_n, vmin)
    logp, po = ref["logp"], ref["po"]
    xa = ref["xa"]
    dz = np.abs(xa - xa.max(-1, keepdims=True))
    lse = np.abs(np.log(np.exp(-dz).sum(-1, keepdims=True)))
    e_sum = EXPF_REL + U * (po * dz).sum(-1, keepdims=True) + 6 * U
    tol_logp = U * dz + e_sum + LOGF_BOUND + U * (dz + lse)
    tol_loss = (tol_m * np.abs(logp) + m * tol_logp).sum(-1) + 7 * U * (m * np.abs(logp)).sum(-1)
    msum = ref["mass"].reshape(B, 1)
    tol_msum = tol_m.sum(-1, keepdims=True) + 6 * U * msum
    rel_po = _softmax_rel(xa, po)
    tol_g = np.abs(ref["w"]) * (po * msum * (rel_po + 2 * U) + po * tol_msum + tol_m + U * (po * msum + m) + TINY)
    return dict(E=E, tol_m=tol_m, tol_mass=tol_mass, tol_loss=tol_loss, tol_g=tol_g)


# ------------------------------------------------------------------------------------------------ the DQN head (nets.py head on 512 hidden units)
_EYE = np.eye(512)
_ZERO = np.zeros(512)


def head64(h, W, b, A, dueling):
    """(q, scale) [B][A] of the scalar head on activations h [B][512] (relu outputs, exact zeros included): util.qhead64 with fc1 the identity."""
    return qhead64(h, _EYE, _ZERO, W, b, A, dueling)


def head_tol(A, dueling, scale):
    """15 roundings per head row (eight fused multiply-adds per lane, six butterfly stages, the bias) on sum |h| |w| + |b|, then the combine's A + 3."""
    return head_roundings(14, A, dueling) * U * scale


def head_loss64(c):
    """a0_dqn_head_loss on a case of head_case: q_on, q_tg (values, bounds), the greedy next action (first float64 maximum of the selecting network's
    values), loss and draw [B][ld] with their bounds."""
    A, dueling, ld, B = c["A"], c["dueling"], c["ld"], c["B"]
    q_on, s_on = head64(c["h_on"], c["W_on"], c["b_on"], A, dueling)
    q_tg, s_tg = head64(c["h_tg"], c["W_tg"], c["b_tg"], A, dueling)
    t_on, t_tg = head_tol(A, dueling, s_on), head_tol(A, dueling, s_tg)
    if c["h_sel"] is not None:
        q_sel, s_sel = head64(c["h_sel"], c["W_on"], c["b_on"], A, dueling)
    else:
        q_sel, s_sel = q_tg, s_tg
    t_sel = head_tol(A, dueling, s_sel)
    a_star = q_sel.argmax(1)                                       # the first maximum
    # the loss on the fp32 roundings of the float64 q values (what a correct kernel holds to within t_on, t_tg), the bounds from the float64 scales
    gam = float(np.float32(c["gamma_n"]))
    act = c["act"]
    qa, qn = _rows(q_on, act), _rows(q_tg, a_star)
    r, dn, w = _f64(c["rew"]), _f64(c["done"]), _f64(c["wgt"])
    y = r + gam * (1.0 - dn) * qn
    d = qa - y
    loss, slope = smooth_l1(d, d.astype(np.float32))
    S = _rows(s_on, act) + np.abs(r) + gam * _rows(s_tg, a_star)
    e_d = _rows(t_on, act) + gam * (1.0 - dn) * _rows(t_tg, a_star) + 5 * U * S
    tol_loss = e_d * np.maximum(np.abs(d), 1.0) + 2 * U * loss
    g = w * slope
    tol_g = np.abs(w) * (e_d + U * np.abs(slope))
    draw, tol_draw = np.zeros((B, ld)), np.zeros((B, ld))
    rows = np.arange(B)
    if dueling:
        share = np.full((B, A), 1.0 / A)
        share[rows, act] += 1.0
        draw[:, :A] = -g[:, None] / A
        draw[rows, act] += g
        draw[:, A] = g
        tol_draw[:, :A] = tol_g[:, None] * share + 2 * U * np.abs(g)[:, None] * share
        tol_draw[:, A] = tol_g
    else:
        draw[rows, act] = g
        tol_draw[rows, act] = tol_g
    return dict(q_on=q_on, q_tg=q_tg, q_sel=q_sel, t_on=t_on, t_tg=t_tg, t_sel=t_sel, s_on=s_on, a_star=a_star, loss=loss, tol_loss=tol_loss, g=g, tol_g=tol_g,
                draw=draw, tol_draw=tol_draw, d=d)


HEAD_BS = (1, 3, 4, 5, 9)
HEAD_HEADS = ((1, 0), (1, 1), (4, 0), (4, 1), (18, 1), (23, 1), (24, 0))
GAMMA = 0.99 ** 3
_HEAD = {}


def head_transitions(g, B, A):
    """Actions that hit 0 and A - 1, rewards, done flags of both kinds, weights with a zero and values away from 1."""
    act = g.integers(0, A, B).astype(np.int32)
    act[0] = A - 1
    act[-1] = 0
    rew = g.standard_normal(B).astype(np.float32)
    done = (g.random(B) < 0.3).astype(np.float32)
    done[0] = 0.0
    wgt = g.uniform(0.2, 2.5, B).astype(np.float32)
    if B > 2:
        done[1], wgt[2] = 1.0, 0.0
    return act, rew, done, wgt


def _head_inputs(B, A, dueling, with_sel, seed):
    g = recipe.gen(seed)
    NQ = A + (1 if dueling else 0)
    mk_h = lambda: (np.maximum(g.standard_normal((B, 512)), 0) * (0.5 + np.arange(B)[:, None] / max(B - 1.0, 1.0))).astype(np.float32)
    c = dict(B=B, A=A, dueling=dueling, NQ=NQ, gamma_n=GAMMA, h_on=mk_h(), h_tg=mk_h(), h_sel=mk_h() if with_sel else None)
    for k in ("on", "tg"):
        c["W_" + k] = (g.standard_normal((NQ, 512)) / 16.0).astype(np.float32)
        c["b_" + k] = (0.3 * g.standard_normal(NQ)).astype(np.float32)
    c["act"], c["rew"], c["done"], c["wgt"] = head_transitions(g, B, A)
    c["tie"] = None
    if A >= 2:
        # the selecting network's rows tie_pair(A) made bit-identical (weights and bias: the tie survives the combine), and lifted so that the pair is the best
        # action of the sample where that takes the least, which becomes sample 0; the other network's rows differ, so the choice shows in the loss
        k = "on" if with_sel else "tg"
        hk = "h_sel" if with_sel else "h_tg"
        i, j = tie_pair(A)
        W, b = c["W_" + k], c["b_" + k]
        W[j], b[j] = W[i], b[i]
        if A > 2:
            q, _ = head64(c[hk], W, b, A, dueling)
            gap = np.delete(q, (i, j), 1).max(1) - q[:, i]
            e = int(gap.argmin())
            c[hk][[0, e]] = c[hk][[e, 0]]
            b[i] = b[j] = np.float32(b[i] + np.float32(gap[e] + 0.05))
        c["tie"] = (i, j)
    return c


def _spread(v, tied, A):
    try:
        check_spread(v, tied, A, "")
        return True
    except AssertionError:
        return False


def _tie_shows(c, ref):
    """Sample 0's loss with the later of the two tied actions as a*: a hundred bounds away from the loss with the first."""
    j = c["tie"][1]
    d_j = ref["q_on"][0, c["act"][0]] - (c["rew"][0] + float(np.float32(c["gamma_n"])) * (1.0 - c["done"][0]) * ref["q_tg"][0, j])
    return abs(smooth_l1(d_j, np.float32(d_j))[0] - ref["loss"][0]) > 100 * ref["tol_loss"][0]


def head_case(B, A, dueling, with_sel):
    """Inputs of one a0_dqn_head_loss case (computed once): the first seed whose float64 reference has the planted pair as sample 0's best action and, in
    every other sample, a gap between the two best selecting values above four times their bounds, and (check_spread) free samples that do not all share one
    best action; under double-Q also a loss of sample 0 that the later of the tied actions would move by a hundred bounds."""
    key = (B, A, dueling, with_sel)
    if key not in _HEAD:
        for k in range(16):
            c = _head_inputs(B, A, dueling, with_sel, 5000 + 97 * B + 7 * A + 3 * dueling + with_sel + 100000 * k)
            ref = head_loss64(dict(c, ld=c["NQ"]))
            v, t = ref["q_sel"], ref["t_sel"]
            if c["tie"] is None:
                tied = np.zeros(B, bool)
            else:
                i, j = c["tie"]
                tied = (v[:, i] == v.max(1)) & (v[:, i] == v[:, j])
            srt = np.sort(v, 1)
            gap_ok = (A == 1) | tied | ((srt[:, -1] - srt[:, -2 if A > 1 else -1]) > 4 * t.max(1))
            if gap_ok.all() and (c["tie"] is None or (tied[0] and _spread(v, tied, A) and (not with_sel or _tie_shows(c, ref)))):
                break
        else:
            raise AssertionError(f"no usable seed for {key}")
        c["tied"] = tied
        _HEAD[key] = c
    return _HEAD[key]


# ------------------------------------------------------------------------------------------------ cases of the standalone losses
LOSS_BS = (1, 127, 128, 129)
DQN_AS = (1, 4, 18)
MDQN_AS = (1, 2, 4, 18)
MDQN_TAUS = (0.03, 1.0, 0.003)
MDQN_LO = -1.0
ONE_UP, ONE_DOWN = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
# (name, q at the taken action, reward, done): d = q - r exactly, the row being done or having q' = 0
DQN_PLAN = (("d0", 0.75, 0.75, 1.0), ("dm1", 0.75, 1.75, 1.0), ("dp1", 0.75, -0.25, 0.0), ("above", 0.0, float(ONE_UP), 1.0), ("below", 0.0, float(ONE_DOWN), 0.0),
            ("done", None, None, 1.0), ("w0", None, None, None), ("w25", None, None, None))


def _hit_ends(a, A):
    a[0] = 0
    a[-1] = A - 1
    if len(a) > 2:
        a[1] = A - 1
    return a


def dqn_case(B, A, variant=0):
    """q, q_next [B][A], act, a_star (both hit 0 and A - 1), rew, done, wgt and the planted rows (cyclic from row ``variant``, so that B = 1 meets each of them
    over its variants): d = 0; d = -1 and +1 exactly; |d| one ulp either side of 1; done = 1; w = 0; w = 2.5.  Every planted d is exact in fp32: the row is
    done (y is the reward bit for bit) or has q' = 0, and q, r are small dyadic numbers."""
    g = recipe.gen(8000 + 31 * B + A + 1000 * variant)
    q = (g.standard_normal((B, A)) * 2).astype(np.float32)
    qn = (g.standard_normal((B, A)) * 2).astype(np.float32)
    act, a_star = _hit_ends(g.integers(0, A, B).astype(np.int32), A), _hit_ends(g.integers(0, A, B).astype(np.int32), A)[::-1].copy()
    rew = g.standard_normal(B).astype(np.float32)
    done = (g.random(B) < 0.25).astype(np.float32)
    wgt = g.uniform(0.2, 1.0, B).astype(np.float32)
    planted = {}
    for k, (name, qv, rv, dv) in enumerate(DQN_PLAN):
        if B == 1:
            if k != variant % len(DQN_PLAN):
                continue
            b = 0
        else:
            b = 3 + 7 * k
        if qv is not None:
            q[b, act[b]], rew[b], done[b] = qv, rv, dv
            if not dv:
                qn[b, a_star[b]] = 0.0
        elif name == "done":
            done[b] = 1.0
        else:
            wgt[b] = 0.0 if name == "w0" else 2.5
        planted[name] = b
    return dict(q=q, q_next=qn, act=act, a_star=a_star, rew=rew, done=done, wgt=wgt, planted=planted)


def mdqn_case(B, A, tau, variant=0):
    """q, q_next, q_cur [B][A] and the transitions.  Planted rows (cyclic from ``variant``): the clamp at lo active (the taken action far below q_cur's maximum),
    inactive (just below it), the taken action q_cur's argmax (add-on about 0, the upper clamp), all q equal, |q| about 100, done = 1, and a row whose q puts
    the fp32 reference's d on the |d| = 1 seam."""
    g = recipe.gen(9000 + 31 * B + A + int(1000 * tau) + 777 * variant)
    q = (g.standard_normal((B, A)) * 2).astype(np.float32)
    qn = (g.standard_normal((B, A)) * 2).astype(np.float32)
    qc = (g.standard_normal((B, A)) * 2).astype(np.float32)
    act = _hit_ends(g.integers(0, A, B).astype(np.int32), A)
    rew = g.standard_normal(B).astype(np.float32)
    done = (g.random(B) < 0.25).astype(np.float32)
    wgt = g.uniform(0.2, 2.5, B).astype(np.float32)
    names = ["lo_active", "lo_inactive", "argmax", "equal", "big", "done", "seam"]
    planted = {}
    for k, name in enumerate(names):
        if B == 1:
            if k > 0:
                break
            name = names[variant % len(names)]
            b = 0
        elif B < len(names):
            continue
        else:
            b = 2 + 9 * k
        a = act[b]
        if name == "lo_active":
            qc[b] = 1.0
            qc[b, a] = 1.0 - 50.0 * max(tau, 0.02) if A > 1 else 1.0
        elif name == "lo_inactive":
            qc[b] = -30.0
            qc[b, a] = 0.5
            if A > 1:
                qc[b, (a + 1) % A] = 0.5 + np.float32(0.1 * tau)           # the log-policy of a is about -0.74 tau
        elif name == "argmax":
            qc[b] = -30.0
            qc[b, a] = 2.0
        elif name == "equal":
            qn[b], qc[b] = 0.37, -1.25
        elif name == "big":
            qn[b] = (100.0 + g.standard_normal(A) * 0.01).astype(np.float32)
            qc[b] = (-100.0 + g.standard_normal(A) * 0.01).astype(np.float32)
            q[b] = 99.0
        elif name == "done":
            done[b] = 1.0
        planted[name] = b
    c = dict(q=q, q_next=qn, q_cur=qc, act=act, rew=rew, done=done, wgt=wgt, planted=planted, tau=tau, lo=MDQN_LO)
    if "seam" in planted or (B == 1 and names[variant % len(names)] == "seam"):
        b = planted.get("seam", 0)
        y32 = mdqn_y32(qn, qc, act, rew, done, float(np.float32(GAMMA)), float(np.float32(tau)), float(np.float32(MDQN_LO)))
        q[b, act[b]] = np.float32(y32[b] + np.float32(1.0))
        planted["seam"] = b
    return c


C51_TS = (2, 3, 32, 51, 63, 64)
C51_AS = (1, 4, 18)
C51_SUPPORTS = ((-10.0, 10.0), (0.0, 200.0), (-1.0, 1.0))
C51_GAMMAS = (0.99, 0.99 ** 3)
C51_KINDS = ("clamp_high", "clamp_low", "bin0", "binlast", "interior", "terminal", "tgt_peak", "on_peak", "w0", "w25", "r0", "random")


def c51_atoms(vmin, vmax, T):
    return np.linspace(vmin, vmax, T).astype(np.float32)


def c51_rows(kinds, T, A, vmin, vmax, seed):
    """One sample per entry of ``kinds``: logits, tgt_logits [B][A][T], act, a_star (hitting 0 and A - 1), rew, done, wgt."""
    g = recipe.gen(seed)
    B = len(kinds)
    span = vmax - vmin
    atoms = c51_atoms(vmin, vmax, T)
    x = (g.standard_normal((B, A, T)) * 1.5).astype(np.float32)
    xt = (g.standard_normal((B, A, T)) * 1.5).astype(np.float32)
    act, a_star = g.integers(0, A, B).astype(np.int32), g.integers(0, A, B).astype(np.int32)
    act[0], a_star[0] = 0, A - 1
    if B > 1:
        act[-1], a_star[-1] = A - 1, 0
    rew = (vmin + span * (0.5 + 0.2 * g.standard_normal(B))).astype(np.float32) * np.float32(0.2)
    done = np.zeros(B, np.float32)
    wgt = g.uniform(0.2, 1.0, B).astype(np.float32)

    def peak(row):
        k = int(g.integers(0, T))
        row[:] = (-80.0 + g.standard_normal(T)).astype(np.float32)
        row[k] = 80.0

    for b, kind in enumerate(kinds):
        if kind == "clamp_high":
            rew[b] = vmax + 5 * span
        elif kind == "clamp_low":
            rew[b] = vmin - 5 * span
        elif kind == "bin0":
            rew[b], done[b] = vmin, 1.0
        elif kind == "binlast":
            rew[b], done[b] = vmax, 1.0
        elif kind == "interior":
            rew[b], done[b] = atoms[T // 2], 1.0
        elif kind == "terminal":
            rew[b], done[b] = np.float32(vmin + span * g.uniform(0.1, 0.9)), 1.0
        elif kind == "tgt_peak":
            peak(xt[b, a_star[b]])
        elif kind == "on_peak":
            peak(x[b, act[b]])
        elif kind == "w0":
            wgt[b] = 0.0
        elif kind == "w25":
            wgt[b] = 2.5
        elif kind == "r0":
            rew[b] = 0.0
    return dict(logits=x, tgt_logits=xt, act=act, a_star=a_star, rew=rew, done=done, wgt=wgt, atoms=atoms, kinds=tuple(kinds))


def c51_launches(T, A):
    """The launches of one (T, A): for every support and gamma_n, B = 5 three times (the twelve kinds of row, the last launch wrapping round) and B = 1 once
    (one kind, rotating); m_out alternately given and null.  Yields (vmin, vmax, gamma_n, with_m, rows)."""
    n = 0
    for si, (vmin, vmax) in enumerate(C51_SUPPORTS):
        for gi, gam in enumerate(C51_GAMMAS):
            sets = [C51_KINDS[0:5], C51_KINDS[5:10], C51_KINDS[10:12] + C51_KINDS[0:3], (C51_KINDS[(T + A + 2 * si + gi) % 12],)]
            for kinds in sets:
                yield vmin, vmax, gam, n % 3 != 2, c51_rows(kinds, T, A, vmin, vmax, 11000 + 131 * T + 17 * A + 7 * si + gi + 1000 * n)
                n += 1


FINDING = ((-1.0, 1.0, 62), (0.0, 1.0, 62), (-10.5, 10.5, 30), (-10.5, 10.5, 59))        # fl32(delta) lies below the exact width: vmax lands above bin T - 1
