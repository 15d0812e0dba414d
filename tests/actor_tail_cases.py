"""Cases, inputs, error bounds and an fp32 restatement of the actor's action-selection kernels, shared by tests/test_actor_tail_reference_helpers.py (CPU:
the bound is fixed there, before any device run) and tests/test_gpu_actor_tail_reference.py (the kernels).  The derivation of the bound is in the GPU
test's docstring.  No import of the library."""
from __future__ import annotations

import math

import numpy as np

import recipe
from util import action_values64, head_from_slabs64, qhead64

U = 2.0 ** -24                  # one fp32 rounding, relative to the magnitude it happens at
GEMM_TOL = 2e-6                 # the split-operand GEMM's bound on its accumulated magnitude (tests/test_gpu_gemm.py, tests/test_gpu_conv_reference.py)
# expf on the device, worst relative error against float64 exp, measured on an MI355X by test_expf_error_stays_within_the_recorded_figure on the 57 000 of
# its 1e5 arguments in [-40, 0] that lie below -17, where the quotient it reads is expf itself: 9.07e-8 (profiles/r11_actor_tail_accuracy.md; over the whole
# range, two further roundings included, 1.71e-7).  The bound takes twice the figure; the test fails if a device exceeds it.
EXPF_MEASURED = 9.1e-8
EXPF_REL = 2.0 * EXPF_MEASURED
MAX_UNDECIDED = 0.02

# (A, T, dueling, mode, ld, nslab, E[, offset]): offset = floats between a 16-byte boundary and the first slab
DIST_CASES = [
    (4, 51, False, 2, 204, 8, 5, 0),
    (3, 51, True, 2, 204, 3, 1, 0),
    (3, 51, False, 2, 153, 9, 6, 0),
    (18, 51, True, 2, 972, 1, 7, 0),
    (4, 200, True, 1, 1000, 12, 5, 0),
    (6, 11, True, 1, 77, 7, 9, 0),
    (5, 65, False, 1, 328, 16, 4, 0),
    (2, 1, False, 1, 4, 4, 4, 0),
    (4, 51, False, 2, 204, 8, 5, 1),
]
QUANTILE_CASES = [
    (4, 32, False, 1, 32, 8, 5, 0),
    (18, 32, True, 3, 20, 3, 5, 0),
    (9, 32, False, 3, 9, 9, 6, 0),
    (6, 8, True, 1, 7, 1, 9, 0),
    (3, 65, True, 1, 4, 4, 1, 0),
]
QHEAD_K = 544                   # the smallest K at which the fc1 split-K GEMM takes 17 splits (splits <= ceil(K / 32))
QHEAD_SPLITS = (1, 3, 4, 7, 8, 9, 12, 13, 16, 17)
QHEAD_HEADS = ((4, False), (18, True), (23, True), (2, True), (6, False))
QHEAD_ES = (1, 5, 9)
QHEAD_ENV_K = 3136


def fc1_splits(E, K):
    """The split count the library's fc1 GEMM chooses for E <= 256 rows of K features and 512 outputs (64 x 64 tiles, about 256 workgroups, at least two
    32-wide k steps per split): what actor_qhead and the merged forms run with; the GPU test checks it against actor_qhead_scratch."""
    assert E <= 256
    return max(1, min(256 // (((E + 63) // 64) * 8), (K // 32) // 2, 64))


QHEAD_ENV_CASES = [(A, d, E) for (A, d) in ((4, False), (18, True)) for E in (1, 5)]
SELECT_SHAPES = ((4, 1), (18, 51), (6, 11), (4, 200), (9, 65))
SELECT_BS = (1, 7)
MEAN_ROWS_ES = (1, 255, 256, 257, 300)
PAD = 1.0e4                     # what the pad columns of a slab hold: summed by the 16-byte path, never read


def case_id(c):
    return "A{}_T{}_{}_m{}_ld{}_ns{}_E{}{}".format(c[0], c[1], "duel" if c[2] else "plain", c[3], c[4], c[5], c[6], "_off%d" % c[7] if c[7] else "")


def tie_pair(A):
    """The two actions made bit-identical: not adjacent wherever the action set allows it."""
    return (1, A - 1) if A >= 4 else (0, A - 1)


def trips(T):
    return (T + 63) // 64


# ------------------------------------------------------------------------------------------------ bounds
def head_roundings(nslab, A, dueling):
    """Roundings on the longest path of one head output: slab sum + bias (nslab + 1), dueling combine (A - 1 additions, the division, the subtraction and
    the addition: counted as A + 3)."""
    return nslab + 1 + (A + 3 if dueling else 0)


def values_tol(mode, T, c_in, qscale, vscale):
    """Bound [E][A] on an fp32 evaluation of the action values of q whose elements carry c_in roundings of their scale ``qscale`` [E][A][T];
    ``vscale``: action_values64's scale."""
    if mode == 0:
        return c_in * U * qscale[:, :, 0]
    if mode == 1:
        return (c_in + trips(T) + 7) * U * vscale                 # lane's strided sum (ceil(T / 64)), butterfly (6), division (1)
    if mode == 3:
        return (c_in + trips(T) + 8) * U * vscale                 # + the fraction's width and its product with q (one less where they fuse)
    # mode 2: a logit error delta moves sum_t p_t z_t by at most 2 delta sum_t p_t |z_t|; the logit also takes the rounding of (q - max) on |q| + |max|
    delta = (c_in + 2) * U * qscale.max(2)
    # every exp carries EXPF_REL; numerator: product (1) + strided sum + butterfly (6); denominator: strided sum + butterfly; the division (1)
    return (2.0 * delta + 2.0 * EXPF_REL + (2 * trips(T) + 14) * U) * vscale


def qhead_tol(nslab, A, dueling, scale):
    """fc1: the GEMM's bound on every slab's accumulated magnitude, then slab sum + bias (nslab + 1 roundings); head: 8 fused multiply-adds per lane,
    butterfly (6), bias (1); dueling combine (A + 3).  All of them on ``scale``, fc1's magnitude carried through |W2| (util.qhead64)."""
    return (GEMM_TOL + (nslab + 1 + 15 + (A + 3 if dueling else 0)) * U) * scale


def mean_rows_tol(E, scale):
    return ((E + 255) // 256 + 9) * U * scale                      # thread's strided sum, tree over 256 (8), division (1)


# ------------------------------------------------------------------------------------------------ inputs
def _bump(T, c, mode):
    """What moves an action's value by about c / 2 ... c: a ramp towards the high atoms under the softmax expectation (mode 2: a constant would cancel), a
    constant elsewhere."""
    return (c * np.arange(T) / (T - 1.0) if mode == 2 and T > 1 else np.full(T, c)).astype(np.float32)


LOWER, LIFT = 3.0, 7.0           # the pair sits about 3 below the others everywhere and about 4 above them in sample 0


def _plant(mode, T):
    """(what the tied pair is lowered by in every sample, what it is lifted by in sample 0): the pair is the best action of sample 0 and, being well below
    the others elsewhere, leaves the other samples their own maximum."""
    return _bump(T, LOWER, mode), _bump(T, LIFT, mode)


def check_spread(values, tied, A, what):
    """Beyond the planted pair there must be something to judge: with more than one sample and more than two actions most samples are not tied, and (more than
    three actions: with three the pair leaves one other action) their maxima are not all the same action."""
    E = len(tied)
    assert tied.any(), f"{what}: no sample has the planted tie as its best action"
    if E > 1 and A > 2:
        free = ~tied
        assert 2 * free.sum() > E, f"{what}: {int(tied.sum())} of {E} samples are tied"
        if A > 3 and free.sum() > 1:
            assert len(set(values.argmax(1)[free].tolist())) > 1, f"{what}: every free sample has the same best action"


def _taus(g, E, T):
    """Fraction boundaries [E][T + 1] of a float64 softmax-cumsum rounded to fp32, tau[0] = 0, tau[T] = 1, zero-width fractions planted."""
    p = np.exp(g.standard_normal((E, T)))
    if T >= 3:
        p[:, T // 3] = 0.0
        p[0, 0] = 0.0
    p /= p.sum(1, keepdims=True)
    tau = np.concatenate((np.zeros((E, 1)), np.cumsum(p, 1)), 1).astype(np.float32)
    tau[:, 0], tau[:, T] = 0.0, 1.0
    assert T < 3 or (tau[:, 1:] == tau[:, :-1]).any()
    return tau


def tail_inputs(case, kt, seed):
    """Slabs [nslab][rows][ld] (standard normal / sqrt(nslab), pad columns PAD), a non-zero bias, the mode's aux, and one exact tie: the columns of the
    actions tie_pair(A) are bit-identical in every slab and in the bias, and env 0 gets a ramp over t added to both in slab 0 (the tie becomes its best)."""
    A, T, dueling, mode, ld, nslab, E = case[:7]
    g = recipe.gen(seed)
    NQ = A + (1 if dueling else 0)
    rows, used = (E * T, NQ) if kt else (E, NQ * T)
    slabs = (g.standard_normal((nslab, rows, ld)) / math.sqrt(nslab)).astype(np.float32)
    slabs[:, :, used:] = PAD
    bias = ((0.1 if kt else 0.5) * g.standard_normal(max(NQ, 4) if kt else ld)).astype(np.float32)     # per action (kt): small beside the spread over envs
    bias[bias == 0] = 0.25
    i, j = tie_pair(A)
    lower, bump = _plant(mode, T)
    if kt:
        slabs[:, :, j] = slabs[:, :, i]
        bias[i] -= lower[0]                           # a bias per action: the constant (the quantile heads have no mode 2)
        bias[j] = bias[i]
        slabs[0, :T, i] += bump
        slabs[0, :T, j] = slabs[0, :T, i]
    else:
        slabs[:, :, j * T:(j + 1) * T] = slabs[:, :, i * T:(i + 1) * T]
        bias[i * T:(i + 1) * T] -= lower
        bias[j * T:(j + 1) * T] = bias[i * T:(i + 1) * T]
        slabs[0, 0, i * T:(i + 1) * T] += bump
        slabs[0, 0, j * T:(j + 1) * T] = slabs[0, 0, i * T:(i + 1) * T]
    aux = None
    if mode == 2:
        aux = np.linspace(-10.0, 10.0, T).astype(np.float32)
    elif mode == 3:
        aux = _taus(g, E, T)
    return slabs, bias, aux


_TAIL = {}


def _seeds(first):
    """The seeds a case tries in turn: it takes the first whose float64 reference leaves something to judge (check_spread) and no env undecided."""
    return [first + 100000 * k for k in range(16)]


def _usable(v, tol, tied, A):
    from util import greedy_check
    try:
        assert tied[0]
        check_spread(v, tied, A, "")
        a, qm = first_max(v)
        return greedy_check(v, tol, a, qm, exclude=tied, allow_empty=True) <= MAX_UNDECIDED
    except AssertionError:
        return False


def tail_reference(case, kt):
    """Inputs, float64 action values, their bound and the planted tie of one case of the tables (computed once)."""
    key = (case, kt)
    if key not in _TAIL:
        A, T, dueling, mode, ld, nslab, E = case[:7]
        i, j = tie_pair(A)
        for seed in _seeds(1000 + 17 * (DIST_CASES, QUANTILE_CASES)[kt].index(case) + kt):
            slabs, bias, aux = tail_inputs(case, kt, seed)
            q, qs = head_from_slabs64(slabs, bias, A, T, dueling, kt)
            v, vs = action_values64(q, mode, aux, qs)
            tol = values_tol(mode, T, head_roundings(nslab, A, dueling), qs, vs)
            tied = (v[:, i] == v.max(1)) & (v[:, i] == v[:, j])          # envs whose best action is the planted pair
            if _usable(v, tol, tied, A):
                break
        assert tied[0], f"{case}: the planted tie is not env 0's best action"
        check_spread(v, tied, A, case_id(case))
        _TAIL[key] = dict(slabs=slabs, bias=bias, aux=aux, q=q, qscale=qs, values=v, vscale=vs, tol=tol, tie=(i, j), tied=tied)
    return _TAIL[key]


def qhead_inputs(E, K, A, dueling, seed):
    """Features relu(normal) [E][K], each env's scaled differently, fc1 and head parameters with non-zero biases; the head's rows tie_pair(A) (and their b2
    entries) are bit-identical.  b2 is per action, not per env: the pair's entry is set 0.05 above the other actions' maximum in the env where that takes the
    least, and that env is made env 0 — the pair is its best action and the other envs keep their own."""
    g = recipe.gen(seed)
    NQ = A + (1 if dueling else 0)
    feat = (np.maximum(g.standard_normal((E, K)), 0) * (0.5 + np.arange(E)[:, None] / max(E - 1.0, 1.0))).astype(np.float32)
    W1 = (g.standard_normal((512, K)) * math.sqrt(2.0 / K)).astype(np.float32)
    b1 = (0.5 * g.standard_normal(512)).astype(np.float32)
    W2 = (g.standard_normal((NQ, 512)) / 16.0).astype(np.float32)
    b2 = (0.3 * g.standard_normal(NQ)).astype(np.float32)
    i, j = tie_pair(A)
    W2[j] = W2[i]
    b2[j] = b2[i]
    if A > 2:
        q, _ = qhead64(feat, W1, b1, W2, b2, A, dueling)
        gap = np.delete(q, (i, j), 1).max(1) - q[:, i]           # a lift of the pair's b2 entries moves it past the others by exactly that lift, dueling or not
        e = int(gap.argmin())
        feat[[0, e]] = feat[[e, 0]]
        b2[i] = b2[j] = np.float32(b2[i] + np.float32(gap[e] + 0.05))
    return feat, W1, b1, W2, b2


_QHEAD = {}


def qhead_reference(E, K, A, dueling):
    key = (E, K, A, dueling)
    if key not in _QHEAD:
        i, j = tie_pair(A)
        for seed in _seeds(2000 + 31 * E + A + K):
            feat, W1, b1, W2, b2 = qhead_inputs(E, K, A, dueling, seed)
            v, vs = qhead64(feat, W1, b1, W2, b2, A, dueling)
            tied = (v[:, i] == v.max(1)) & (v[:, i] == v[:, j])
            if _usable(v, qhead_tol(64, A, dueling, vs), tied, A):          # at the bound of the largest split count there is
                break
        check_spread(v, tied, A, str(key))
        _QHEAD[key] = dict(feat=feat, W1=W1, b1=b1, W2=W2, b2=b2, values=v, vscale=vs, tie=(i, j), tied=tied)
    return _QHEAD[key]


def select_inputs(A, T, B, mode, transposed, seed):
    """x as select_action reads it — contiguous [B][A][T] (strides A T, T, 1) or [B][T][ld] with ld = A + 3 (strides T ld, 1, ld), pad PAD — with the actions
    tie_pair(A) bit-identical and the best of sample 0; returns (flat x, strides, q [B][A][T] as fp32, aux)."""
    g = recipe.gen(seed)
    q = g.standard_normal((B, A, T)).astype(np.float32)
    i, j = tie_pair(A)
    lower, bump = _plant(mode, T)
    q[:, i] -= lower
    q[0, i] += bump
    q[:, j] = q[:, i]
    aux = np.linspace(-10.0, 10.0, T).astype(np.float32) if mode == 2 else (_taus(g, B, T) if mode == 3 else None)
    if not transposed:
        return q.reshape(-1).copy(), (A * T, T, 1), q, aux
    ld = A + 3
    x = np.full((B, T, ld), PAD, np.float32)
    x[:, :, :A] = q.transpose(0, 2, 1)
    return x.reshape(-1), (T * ld, 1, ld), q, aux


# ------------------------------------------------------------------------------------------------ draws
def egreedy_expected(seed, stream_a, stream_u, off_a, off_u, eps, A, greedy):
    """The epsilon-greedy action of every env from the oracle's Philox draws at offset + e: greedy where u > eps, else word % A; and the mask of greedy envs."""
    from oracle import core
    E = len(greedy)
    ra = (core.rng_u32(seed, stream_a, off_a, E) % np.uint32(A)).astype(np.int64)
    u = core.rng_uniform(seed, stream_u, off_u, E)
    keep = u > np.float32(eps)
    return np.where(keep, np.asarray(greedy, np.int64), ra), keep


RNG_SEED, STREAM_A, STREAM_U, EPS = 0x1234_0077, 2, 1, 0.3


def draw_offsets(E, A, lone_greedy=False):
    """(off_a, off_u) at which the oracle's draws alone send at least one of the E envs down each branch (a lone env: the random branch, or the greedy one
    with ``lone_greedy``; the two launches of a case take one each); searched deterministically from a fixed start."""
    from oracle import core
    for k in range(4096):
        off_a, off_u = 40 + 3 * k, 44 + 5 * k
        keep = core.rng_uniform(RNG_SEED, STREAM_U, off_u, E) > np.float32(EPS)
        if (E == 1 and bool(keep[0]) == lone_greedy) or (keep.any() and not keep.all()):
            return off_a, off_u
    raise AssertionError("no offsets found")


# ------------------------------------------------------------------------------------------------ fp32 restatement, in the kernels' order of additions
F32 = np.float32
_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _butterfly(v):
    """The wave reduction: six exchange-and-add stages over the last axis (64 lanes); lane 0's result."""
    for idx in _XOR:
        v = (v + v[..., idx]).astype(F32)
    return v[..., 0]


def _lanes(x, fill=0.0):
    """x [..., T] -> [..., trips][64] with element t at trip t // 64, lane t % 64."""
    T = x.shape[-1]
    n = trips(T) * 64
    out = np.full(x.shape[:-1] + (n,), fill, F32)
    out[..., :T] = x
    return out.reshape(x.shape[:-1] + (trips(T), 64))


def _strided_sum(xl):
    s = np.zeros(xl.shape[:-2] + (64,), F32)
    for k in range(xl.shape[-2]):
        s = (s + xl[..., k, :]).astype(F32)
    return s


def head_from_slabs32(slabs, bias, A, T, dueling, kt):
    slabs, bias = np.asarray(slabs, F32), np.asarray(bias, F32)
    NQ = A + (1 if dueling else 0)
    acc = np.zeros(slabs.shape[1:], F32)
    for z in range(slabs.shape[0]):
        acc = (acc + slabs[z]).astype(F32)
    if kt:
        x = (acc.reshape(-1, T, acc.shape[-1])[:, :, :NQ] + bias[:NQ]).astype(F32).transpose(0, 2, 1)
    else:
        x = (acc[:, :NQ * T] + bias[:NQ * T]).astype(F32).reshape(-1, NQ, T)
    if dueling:
        s = np.zeros_like(x[:, 0])
        for a in range(A):
            s = (s + x[:, a]).astype(F32)
        mean = (s / F32(A)).astype(F32)
        x = (x[:, A:A + 1] + (x[:, :A] - mean[:, None]).astype(F32)).astype(F32)
    return np.ascontiguousarray(x[:, :A])


def action_values32(q, mode, aux=None):
    q = np.asarray(q, F32)
    T = q.shape[2]
    if mode == 0:
        return q[:, :, 0].copy()
    if mode == 1:
        return (_butterfly(_strided_sum(_lanes(q))) / F32(T)).astype(F32)
    if mode == 3:
        tau = np.asarray(aux, F32)
        d = (tau[:, 1:] - tau[:, :-1]).astype(F32)[:, None, :]
        return _butterfly(_strided_sum(_lanes((d * q).astype(F32))))
    z = np.asarray(aux, F32)
    mx = q.max(2, keepdims=True)
    ex = np.exp((q - mx).astype(F32)).astype(F32)
    se = _butterfly(_strided_sum(_lanes(ex)))
    sz = _butterfly(_strided_sum(_lanes((ex * z).astype(F32))))
    return (sz / se).astype(F32)


def qhead32(feat, W1, b1, W2, b2, A, dueling, nslab):
    """fc1 as nslab slabs over consecutive k ranges (exact products, one fp32 rounding per slab: the best a split-K GEMM can deliver), then a0_qhead_wave's
    order: slab sum in slab order, bias, ReLU; per head row eight fused multiply-adds per lane (k = lane + 64 i), the butterfly, the bias; the combine."""
    f, w1 = np.asarray(feat, np.float64), np.asarray(W1, np.float64)
    K = f.shape[1]
    edges = [(K * z) // nslab for z in range(nslab + 1)]
    h = np.zeros((f.shape[0], 512), F32)
    for z in range(nslab):
        h = (h + (f[:, edges[z]:edges[z + 1]] @ w1[:, edges[z]:edges[z + 1]].T).astype(F32)).astype(F32)
    h = np.maximum((h + np.asarray(b1, F32)).astype(F32), F32(0))
    NQ = A + (1 if dueling else 0)
    hl = h.reshape(-1, 1, 8, 64).astype(np.float64)
    wl = np.asarray(W2, np.float64).reshape(1, NQ, 8, 64)
    sa = np.zeros((h.shape[0], NQ, 64), F32)
    for i in range(8):
        sa = (hl[:, :, i] * wl[:, :, i] + sa.astype(np.float64)).astype(F32)          # fmaf: the exact product and sum rounded once
    raw = (_butterfly(sa) + np.asarray(b2, F32)).astype(F32)
    if dueling:
        t = np.zeros(raw.shape[0], F32)
        for a in range(A):
            t = (t + raw[:, a]).astype(F32)
        mean = (t / F32(A)).astype(F32)
        raw = (raw[:, A:A + 1] + (raw[:, :A] - mean[:, None]).astype(F32)).astype(F32)
    return np.ascontiguousarray(raw[:, :A])


def first_max(v):
    """(first maximum's index, its value) per row."""
    a = np.asarray(v).argmax(1)
    return a, np.asarray(v)[np.arange(len(a)), a]
