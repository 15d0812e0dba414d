"""Float64 references, error bounds and cases of the prioritized-replay kernels (csrc/replay.hip: the sum-tree set, range set, rebuild and the three sampling
walks, the priority transform, the importance weights, the flat-priority bookkeeping, a0_sum_f32): the yardstick of tests/test_gpu_replay_reference.py,
itself held to oracle.core.SumTree, core.sumtree_find_numpy / sumtree_set_numpy, oracle.replay.ReferenceReplay / is_weights and a hand-written table by
tests/test_replay_reference_helpers.py.

No import of the library.  Every reference takes the fp32 inputs exactly as the kernel receives them — eps, alpha and beta as fp32 numbers, the tree's root
as the fp32 the device holds — and evaluates the formula in float64 in its most literal form.  Every reference returns its bound beside its value; the
derivations are in the GPU test's docstring.  ``*32`` are fp32 restatements of the kernels, statement by statement (the helper test holds them to half of
every bound), and ``WRONG_*`` the mistakes the bounds must reject.

What the sampler is for, stated without the oracle: with c the cumulative mass in front of every leaf (float64), draw k of B lands on a live leaf i whose
interval [c_i, c_{i+1}] holds u_k = (k + xi_k) total / B.  What the tree is: every internal node is fp32(left + right) of its children."""
from __future__ import annotations

import math

import numpy as np

import recipe

F32 = np.float32
U = 2.0 ** -24                           # one fp32 rounding, relative to the magnitude it happens at
MARGIN = 2.0                             # every bound is twice its count of roundings: a literal fp32 evaluation sits within half of it (optim_ref.py)
# powf on the device, largest error in fp32 ulps against the float64 power, measured on an MI355X by test_priorities_against_float64 over its cases:
# 1.177 ulp at alpha = 0.6, 1.083 at 0.25 and 1.000 at alpha = 1 (powf(x, 1) is not always x).  Its error is not derivable from the code; the bound is twice
# the figure and never less than 2 ulp, and the test fails if a device exceeds it.
POWF_MEASURED_ULP = 1.177
POWF_ULP = max(2.0, 2.0 * POWF_MEASURED_ULP)
EPS = 0.01                               # replay.eps of the project's configurations
ALPHAS = (0.5, 0.6, 1.0, 0.25)
BETAS = (0.0, 0.4, 1.0)
ST_TOP = 2048                            # A0_ST_TOP: the levels with at most this many nodes are the "top"


def f32(x) -> float:
    return float(F32(x))


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def ulp(v):
    """The fp32 unit in the last place at |v| (the denormal spacing at 0), as float64."""
    return np.spacing(np.abs(_f64(v)).astype(F32)).astype(np.float64)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def worst(name, got, ref, bound, inputs=None):
    """(fraction of the bound the worst element uses, a message with that element's inputs); a zero bound asks for equality (fraction 0 or inf)."""
    got, ref = _f64(got).reshape(-1), _f64(ref).reshape(-1)
    bound = np.broadcast_to(_f64(bound), ref.shape)
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    frac = np.where(np.isfinite(got) & ~np.isnan(frac), frac, np.inf)
    i = int(frac.argmax())
    ins = ", ".join(f"{k} {float(np.asarray(a).reshape(-1)[i] if np.ndim(a) else a)!r}" for k, a in (inputs or {}).items())
    return float(frac[i]), f"{name}[{i}]: got {got[i]!r} want {ref[i]!r} bound {bound[i]:.3e} ({frac[i]:.3f} of it); {ins}"


# ------------------------------------------------------------------------------------------------ priorities (replay.py:55-59)
def prio(loss, eps, alpha):
    """(loss + eps)^alpha -> (value, bound): the sum is the kernel's one fp32 addition, the power is taken in float64.  alpha == 0.5: the value is the
    correctly rounded fp32 square root of that sum (the double root rounded once: 53 >= 2 * 24 + 2) and the bound is zero; any other alpha: POWF_ULP."""
    x = (np.asarray(loss, F32) + F32(eps)).astype(F32)
    a = f32(alpha)
    with np.errstate(all="ignore"):
        if a == 0.5:
            v = np.sqrt(_f64(x)).astype(F32).astype(np.float64)
            return v, np.zeros_like(v)
        v = np.power(_f64(x), a)
    return v, POWF_ULP * ulp(v)


def prio32(loss, eps, alpha):
    """a0_prio_from_loss in numpy fp32."""
    x = (np.asarray(loss, F32) + F32(eps)).astype(F32)
    with np.errstate(all="ignore"):
        return np.sqrt(x) if F32(alpha) == F32(0.5) else np.power(x, F32(alpha))


def max_p(old, loss):
    """max_p tracks the RAW losses: exact."""
    return float(max(F32(old), np.asarray(loss, F32).max()))


def last_wins(base, ids, vals):
    """base with base[ids[j]] = vals[j] applied in batch order: when a batch names an id twice the last entry wins.  Every other entry keeps its bits."""
    out = np.array(base, F32, copy=True)
    for i, v in zip(np.asarray(ids, np.int64).tolist(), np.asarray(vals, F32)):
        out[i] = v
    return out


def priority_tail(maxp, alpha):
    """fp32(float64(max_p) ** float64(alpha)) -> (value, bound): python's float ** float on the fp32 numbers the kernel holds; device double pow is not
    correctly rounded, so the cast may land on the neighbour: 1 fp32 ulp."""
    v = f32(math.pow(f32(maxp), f32(alpha)))
    return v, float(ulp(v))


# ------------------------------------------------------------------------------------------------ a0_sum_f32
def sum_f32(x):
    """(float64 sum, bound).  The fixed two-level tree: stage 1 has min(256, ceil(n / 256)) workgroups of 256 lanes, so a lane's chain is at most
    ceil(n / 65536) additions; eight tree steps end each stage; stage 2's chain adds one partial per lane to 0 (at most 256 partials): one more.  Every
    partial sum is at most sum |x|."""
    x = _f64(x)
    n = x.size
    count = (n + 65535) // 65536 + 8 + 1 + 8
    return float(x.sum()), MARGIN * count * U * float(np.abs(x).sum())


def _tree256(v):
    """The LDS reduction over 256 lanes, halving: v [..., 256] fp32 -> [...]."""
    v = np.array(v, F32, copy=True)
    o = 128
    while o > 0:
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def sum_f32_32(x):
    """a0_sum_stage1 + a0_sum_stage2 in numpy fp32, lane by lane."""
    x = np.asarray(x, F32)
    n = x.size
    blocks = min(256, (n + 255) // 256)
    stride = blocks * 256
    pad = np.zeros(((n + stride - 1) // stride) * stride, F32)
    pad[:n] = x
    trips = pad.reshape(-1, blocks, 256)
    s = np.zeros((blocks, 256), F32)
    for t in trips:
        s = s + t
    part = np.zeros(256, F32)
    part[:blocks] = _tree256(s)
    return F32(_tree256(F32(0) + part))


# ------------------------------------------------------------------------------------------------ importance weights (trainer.py:91-94)
def is_weights(p, total, top, beta):
    """w = (top p / total)^-beta / (max_b w + fp32(1e-8)) in float64 -> (w, bound); total, float(top) and beta as the fp32 the kernel holds.
    Five steps, all relative: the division p / total (U) and the product with top (U) make the power's argument, whose error the power amplifies by beta;
    powf itself errs by POWF_ULP ulps of at most 2 U each; the maximum picks one such element; the sum with 1e-8 and the final division round once each."""
    p = _f64(np.asarray(p, F32))
    b = f32(beta)
    with np.errstate(all="ignore"):
        raw = np.power(f32(float(top)) * (p / f32(total)), -b)
        w = raw / (raw.max() + f32(1e-8))
    e_raw = 2 * b * U + POWF_ULP * 2 * U
    rel = 2 * e_raw + 2 * U
    return w, MARGIN * rel * w


def is_weights32(p, total, top, beta):
    """a0_is_weight + a0_is_weights_normalise in numpy fp32."""
    p = np.asarray(p, F32)
    with np.errstate(all="ignore"):
        raw = np.power(F32(float(top)) * (p / F32(total)), -F32(beta))
        return raw / (raw.max() + F32(1e-8))


def _wrong_no_1e8(p, total, top, beta):
    p = _f64(np.asarray(p, F32))
    raw = np.power(f32(float(top)) * (p / f32(total)), -f32(beta))
    return raw / raw.max()


def _wrong_eps_outside(loss, eps, alpha):
    with np.errstate(all="ignore"):
        return np.power(_f64(np.asarray(loss, F32)), f32(alpha))


def _wrong_block_max(old, loss):
    """A halving reduction launched at B rounded up to a multiple of 64 lanes: from a width that is no power of two it never reaches some lanes."""
    loss = np.asarray(loss, F32)
    width = min(1024, (loss.size + 63) // 64 * 64)
    red = np.full(width, -np.inf, F32)
    for b in range(loss.size):
        red[b % width] = max(red[b % width], loss[b])
    o = width >> 1
    while o > 0:
        red[:o] = np.maximum(red[:o], red[o:2 * o])
        o >>= 1
    return float(max(F32(old), red[0]))


def _wrong_first_wins(base, ids, vals):
    out = np.array(base, F32, copy=True)
    seen = set()
    for i, v in zip(np.asarray(ids, np.int64).tolist(), np.asarray(vals, F32)):
        if i not in seen:
            out[i] = v
            seen.add(i)
    return out


# ------------------------------------------------------------------------------------------------ the tree
def cap2_of(size):
    c = 1
    while c < size:
        c <<= 1
    return c


def tree_from_leaves(leaves, cap2):
    """The tree [2 * cap2] whose leaves (tree[cap2 + i]) are given: every internal node fp32(left + right), level by level in numpy float32.  tree[0] = 0."""
    tree = np.zeros(2 * cap2, F32)
    tree[cap2:cap2 + len(leaves)] = leaves
    n = cap2 >> 1
    while n >= 1:
        tree[n:2 * n] = tree[2 * n:4 * n:2] + tree[2 * n + 1:4 * n:2]
        n >>= 1
    return tree


def tree_violations(tree, cap2, first=1):
    """Indices in [first, cap2) of the internal nodes that are not fp32(left + right) of their children, bit for bit."""
    tree = np.asarray(tree, F32)
    p = np.arange(max(first, 1), cap2)
    return p[bits(tree[p]) != bits(tree[2 * p] + tree[2 * p + 1])]


def tree_mismatch(got, want, lo=1, hi=None):
    """Indices in [lo, hi) at which two trees differ as bit patterns."""
    a, b = bits(got)[lo:hi], bits(want)[lo:hi]
    return np.nonzero(a != b)[0] + lo


def _wrong_tree_by_delta(tree, cap2, ids, vals):
    """The update that adds (new - old) to every ancestor instead of recomputing it from its children."""
    tree = np.array(tree, F32, copy=True)
    for i, v in zip(np.asarray(ids, np.int64).tolist(), np.asarray(vals, F32)):
        n = cap2 + i
        d = F32(v - tree[n])
        tree[n] = v
        n >>= 1
        while n >= 1:
            tree[n] = tree[n] + d
            n >>= 1
    return tree


# ------------------------------------------------------------------------------------------------ sampling
def walk32(tree, cap2, xi, B, le=False, guard=True):
    """a0_sumtree_sample_kernel in numpy fp32, all draws at once -> (leaf indices, leaf priorities).  ``le``: u <= left goes left; ``guard`` off: the right
    child is entered whatever it holds (the two WRONG walks)."""
    tree = np.asarray(tree, F32)
    xi = np.asarray(xi, F32)
    seg = F32(tree[1] / F32(B))
    u = ((np.arange(B).astype(F32) + xi).astype(F32) * seg).astype(F32)
    n = np.ones(B, np.int64)
    c = 1
    while c < cap2:
        left, right = tree[2 * n], tree[2 * n + 1]
        go_left = (u <= left) if le else (u < left)
        if guard:
            go_left = go_left | ~(right > 0)
        u = np.where(go_left, u, u - left).astype(F32)
        n = 2 * n + (~go_left)
        c <<= 1
    return n - cap2, tree[n]


def sample_tol(cap2, total):
    """MARGIN (2 L + 3) 2^-24 total, L = log2(cap2): one rounding per level from u -= left, one per level from the node sums above the leaf, three from
    k + xi, total / B and their product."""
    L = int(cap2).bit_length() - 1
    return MARGIN * (2 * L + 3) * U * float(total)


def sample_check(leaves, cap2, xi, B, idx, p, exact):
    """Draw k of B must land on a leaf i with p_i > 0, return that leaf's bits, and hold c_i - tol <= u_k <= c_{i+1} + tol, where c is the float64 cumulative
    mass in front of every leaf and u_k = (k + xi_k) c[-1] / B.  ``exact`` (the tree is one of exact_tree's: every fp32 operation behind k + xi is exact):
    tol = 0, u_k takes k + xi as the fp32 sum the kernel forms (exact too whenever xi is a multiple of 1/8) and the index must be
    searchsorted(c, u, "right") - 1.  -> dict: ok, message, worst (largest distance outside the interval over tol; 0 inside), mismatch (share of draws off
    the float64 index)."""
    leaves = np.asarray(leaves, F32)
    idx = np.asarray(idx, np.int64)
    xi = np.asarray(xi, F32)
    c = np.concatenate([[0.0], np.cumsum(_f64(leaves))])
    total = c[-1]
    k = np.arange(B)
    if exact:
        u = _f64((k.astype(F32) + xi).astype(F32)) * total / B
        tol = 0.0
    else:
        u = (k + _f64(xi)) * total / B
        tol = sample_tol(cap2, total)
    want = np.minimum(np.searchsorted(c, u, side="right") - 1, leaves.size - 1)
    if idx.min() < 0 or idx.max() >= leaves.size:
        return dict(ok=False, message=f"index out of range: {idx.min()} .. {idx.max()}", worst=np.inf, mismatch=1.0)
    lo, hi = c[idx], c[idx + 1]
    out = np.maximum(np.maximum(lo - u, u - hi), 0.0)
    live = leaves[idx] > 0
    same_bits = bits(p) == bits(leaves[idx])
    mismatch = float((idx != want).mean())
    bad = ~live | ~same_bits | (out > tol) | ((idx != want) if exact else False)
    msg = ""
    if bad.any():
        j = int(np.nonzero(bad)[0][0])
        msg = (f"{int(bad.sum())} of {B} draws, first k = {j}: xi {float(xi[j])!r} u {u[j]!r} -> leaf {int(idx[j])} (p {float(leaves[idx[j]])!r}, returned "
               f"{float(np.asarray(p, F32)[j])!r}), interval [{lo[j]!r}, {hi[j]!r}], tol {tol:.3e}, float64 index {int(want[j])}")
    return dict(ok=not bad.any(), message=msg, worst=float(out.max() / tol) if tol > 0 else float(out.max() > 0), mismatch=mismatch, want=want)


MISMATCH_CAP = 0.05          # share of a general case's draws that may differ from the float64 index: the tolerance must not hide a shifted sampler


# ------------------------------------------------------------------------------------------------ the mistakes
WRONG_PRIO = {"eps_outside_the_power": _wrong_eps_outside}
WRONG_MAX = {"block_max_drops_lanes": _wrong_block_max}
WRONG_LEAVES = {"first_duplicate_wins": _wrong_first_wins}
WRONG_TREE = {"ancestors_by_delta": _wrong_tree_by_delta}
WRONG_WALK = {"u_le_left_goes_left": dict(le=True), "no_right_guard": dict(guard=False)}
WRONG_WEIGHTS = {"no_1e-8": _wrong_no_1e8}


# ------------------------------------------------------------------------------------------------ cases: tree sets
SET_CAP2 = (1, 2, 32, 2048, 4096, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22)      # one workgroup; the five M of the per-wave kernel; one workgroup
SUB_CAP2 = tuple(c for c in SET_CAP2 if c // ST_TOP in (64, 128, 256, 512, 1024))
SET_NS = (1, 63, 64, 65, 1024)
_CACHE = {}


def set_size(cap2):
    """Live leaves of the set cases' tree: a few short of cap2, so that the tail is padding."""
    return cap2 if cap2 <= 2 else cap2 - 5


def set_start_leaves(cap2):
    key = ("set_leaves", cap2)
    if key not in _CACHE:
        size = set_size(cap2)
        leaves = np.zeros(cap2, F32)
        leaves[:size] = recipe.gen(5000 + cap2 % 1000).uniform(0.0, 2.0, size).astype(F32)
        leaves.setflags(write=False)
        _CACHE[key] = leaves
    return _CACHE[key]


def set_batches(cap2):
    """name -> (idx int64 [n], losses fp32 [n]) for a tree of cap2 leaves, applied one after the other.  The values written are the losses themselves
    (a0_sumtree_set) or their priorities at alpha = 0.5 (the from-loss entries); a loss of -fp32(EPS) gives the priority 0.  S: leaves per subtree of the
    per-wave kernel (cap2 / 2048), M = S / 64 leaves per lane; trees off that path get the same index patterns."""
    key = ("set_batches", cap2)
    if key in _CACHE:
        return _CACHE[key]
    size = set_size(cap2)
    g = recipe.gen(5100 + cap2 % 1000)
    S = cap2 // ST_TOP if cap2 >= (1 << 17) else max(1, cap2 // 8)
    M = max(1, S // 64)
    nsub = cap2 // S
    out = {}

    def put(name, idx, loss=None):
        idx = np.asarray(idx, np.int64) % size
        loss = g.uniform(0.0, 3.0, idx.size).astype(F32) if loss is None else np.asarray(loss, F32)
        assert idx.size == loss.size and 1 <= idx.size <= 1024
        out[name] = (idx, loss)

    for n in SET_NS:
        put(f"n={n}", g.integers(0, size, n))
    t = nsub // 3
    put("one_subtree", t * S + g.integers(0, S, 200))
    put("one_leaf_1024_times", np.full(1024, size // 2 + 1))
    put("leaves_0_and_size-1", [0, size - 1, 0, size - 1])
    ts = np.array(sorted({1, nsub // 2, nsub - 1} - {0}), np.int64) if nsub > 1 else np.array([0], np.int64)
    put("subtree_border", np.concatenate([ts * S - 1, ts * S]))
    lanes = np.array([0, M - 1, M, S - 1, 63 * M, 63 * M + M - 1], np.int64) % S
    put("lane_border", np.concatenate([tt * S + lanes for tt in (0, nsub // 2, nsub - 1)]))
    put("zero_values", g.integers(0, size, 65), np.full(65, -F32(EPS), F32))
    _CACHE[key] = out
    return out


RANGE_CASES = ((1 << 19, 1000, 3000), (1 << 22, 70000, 200000))        # (cap2, leaves in front of the ring's end at which the range starts, n): both wrap


def range_case(cap2, back, n):
    size = set_size(cap2)
    start = size - back
    idx = (start + np.arange(n)) % size
    return size, start, idx


# ------------------------------------------------------------------------------------------------ cases: sampling
EXACT_CAP2 = (32, 2048, 4096, 8192, 1 << 17, 1 << 21)
EXACT_B = (1, 64, 1024)
EXACT_XI = (0.0, 0.125, 0.5, 0.875)
GENERAL_SIZES = (24, 3000, 300_000, 1_000_000, 1_500_000, 3_000_000)       # cap2 32, 4096, 2^19, 2^20, 2^21, 2^22; the last for a0_sumtree_sample only
GENERAL_B = (64, 512, 1000)
GENERAL_SEED = 9300
BATCH_RNG = (0x1234_0000_002A, 5, 4096)          # (seed, stream, offset) of the Philox stream a0_sumtree_sample_batch draws its xi from in these cases
GENERAL_B_BATCH = (64, 512, 1024)


def exact_tree(cap2, B):
    """A tree on which the sampler's fp32 arithmetic is exact: leaves in {0, 1, 2, 4}, a dead stretch, a zero tail, the last live leaf padded so that the
    total T is a power of two; with B a power of two and xi a multiple of 1/8 every u, every node and every u - left is representable.  The dead stretch
    (an eighth of the leaves: with B >= 64 wider than several strata's worth of leaves) starts where the mass in front of it is exactly edge_k T / B, so
    draw edge_k with xi = 0 targets its edge.  -> dict leaves [cap2], size, total, dead (a, b), edge_k (None when no stratum boundary can fall there: B = 1)."""
    key = ("exact", cap2, B)
    if key in _CACHE:
        return _CACHE[key]
    g = recipe.gen(5200 + cap2 % 1000 + B)
    size = cap2 - cap2 // 8
    live = g.choice(np.array([0.0, 1.0, 2.0, 4.0]), size, p=[0.3, 0.3, 0.2, 0.2])
    live[0] = 1.0
    T = 2.0 ** math.ceil(math.log2(live.sum()))
    seg = T / B
    dead_len = max(3, size // 8)
    prefix = np.concatenate([[0.0], np.cumsum(live)])
    a0 = size // 4
    cand = np.nonzero((prefix[a0:size - dead_len - 1] % seg == 0) & (prefix[a0:size - dead_len - 1] > 0))[0]
    a, edge_k = (a0 + int(cand[0]), None) if cand.size else (a0, None)
    if cand.size:
        edge_k = int(prefix[a] / seg)
    live[a:a + dead_len] = 0.0
    live[size - 1] += T - live.sum()
    assert live.sum() == T and live[size - 1] >= 0 and T < 2.0 ** 24
    leaves = np.zeros(cap2, F32)
    leaves[:size] = live
    leaves.setflags(write=False)
    _CACHE[key] = dict(leaves=leaves, size=size, total=T, dead=(a, a + dead_len), edge_k=edge_k)
    return _CACHE[key]


def general_tree(size):
    """uniform(0, 2) leaves, a third of them zero, a dead stretch, and a zero tail up to cap2 > size."""
    key = ("general", size)
    if key in _CACHE:
        return _CACHE[key]
    g = recipe.gen(GENERAL_SEED + size % 1000)
    cap2 = cap2_of(size + 1)
    leaves = np.zeros(cap2, F32)
    leaves[:size] = g.uniform(0.0, 2.0, size).astype(F32)
    leaves[:size][g.random(size) < 1.0 / 3.0] = 0.0
    dead = (max(3, size // 1000), max(10, size // 20))
    leaves[dead[0]:dead[1]] = 0.0
    leaves[size - 1] = F32(1.5)                       # the last live leaf is live: a draw at the very end of the mass has a leaf to land on
    leaves.setflags(write=False)
    _CACHE[key] = dict(leaves=leaves, size=size, cap2=cap2, dead=dead)
    return _CACHE[key]


def general_xi(size, B):
    xi = recipe.gen(GENERAL_SEED + 400 + size % 1000 + B).random(B).astype(F32)
    xi[xi >= 1.0] = 0.5
    xi[0], xi[-1] = 0.0, F32(1.0 - 2.0 ** -24)
    return xi


# ------------------------------------------------------------------------------------------------ cases: priorities, weights, sums
PRIO_B = (1, 65, 192, 1024)
SPECIAL_LOSSES = (0.0, -f32(EPS), 1e-8, 1e4)
TAIL_MAX_P = (1.0, 7.5, 1e-3)


def prio_case(B, variant=0):
    """ids (distinct but for one pair: the last entry repeats the first), losses [B]: log-uniform over 1e-8 .. 1e4 and uniform(0, 3) in halves, with
    SPECIAL_LOSSES planted (at B = 1: the one loss is SPECIAL_LOSSES[variant]).  B = 2048 (a0_priority_update only): the largest loss sits at entry 1500."""
    g = recipe.gen(5500 + B + variant)
    loss = np.where(g.random(B) < 0.5, np.exp(g.uniform(math.log(1e-8), math.log(1e4), B)), g.uniform(0.0, 3.0, B)).astype(F32)
    ids = g.permutation(4096)[:B].astype(np.int64)
    if B == 1:
        loss[0] = SPECIAL_LOSSES[variant]
    else:
        at = g.permutation(B)[:4]
        loss[at] = np.asarray(SPECIAL_LOSSES, F32)
        ids[-1] = ids[0]
    if B == 2048:
        loss[1500] = F32(2e4)
    return ids, loss


WEIGHT_B = (1, 65, 192, 1000, 1024)
WEIGHT_KINDS = ("equal", "one_small", "random")


def weights_case(B, kind):
    """(p [B], total, top): all priorities equal; one of them at 1e-6 of the total; random.  B = 2048: the smallest priority — the largest weight — sits at
    entry 1500."""
    g = recipe.gen(5600 + B)
    top = 50_000
    p = np.full(B, 0.7, F32) if kind == "equal" else g.uniform(0.05, 2.0, B).astype(F32)
    total = f32(0.9 * top)
    if kind == "one_small":
        p[B // 2] = F32(1e-6 * total)
    if B == 2048:
        p[1500] = F32(0.01)
    return p, total, top


DOMINANT = dict(p=np.array([np.nextafter(F32(3.0), F32(0.0))], F32), total=3.0, top=10 ** 6, beta=1.0)    # w = 1e-6 / (1e-6 + 1e-8)

SUM_NS = (1, 255, 256, 257, 65536, 65537, 1_000_000)


def sum_case(n):
    """Values of both signs spanning ten binades."""
    g = recipe.gen(5700 + n % 1000)
    return (np.where(g.random(n) < 0.5, -1.0, 1.0) * np.exp2(g.uniform(-5.0, 5.0, n))).astype(F32)
