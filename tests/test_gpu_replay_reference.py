"""GPU (MI355X): the prioritized-replay kernels (csrc/replay.hip) against float64 and against what a sum-tree IS, at their edges.

tests/test_gpu_kernels.py holds these kernels to oracle/sumtree.c, written statement for statement like them, and to each other; this file holds each of
them to tests/replay_ref.py, which states the operation itself (tests/test_replay_reference_helpers.py anchors it to the oracle, to the reference's torch
forms and to a hand-written table, and shows that its bounds reject seven known mistakes).

  * The tree.  After any set, every internal node is fp32(left + right) of its children (level by level in numpy float32), the leaves hold the batch's
    values with a later duplicate winning, and every other leaf keeps its bits: the whole tree is compared as bit patterns with the tree rebuilt from the
    expected leaves.  Guard floats behind the tree and tree[0] keep their bits.
  * The walk.  With c the float64 cumulative mass in front of every leaf, draw k returns a leaf i with p_i > 0, that leaf's bits, and
    c_i - tol <= u_k <= c_{i+1} + tol for u_k = (k + xi_k) c[-1] / B, tol = MARGIN (2 L + 3) 2^-24 total, L = log2(cap2): one rounding per level from
    u -= left, one per level from the node sums above the leaf (the root among them: the kernel scales by the fp32 root, the reference by c[-1]), three
    from k + xi, total / B and their product.  At a million leaves tol is about five mean leaf masses.  So that the tolerance cannot hide a shifted walk,
    at most 5 % of a case's draws may differ from the float64 index searchsorted(c, u, "right") - 1; and on the exact trees (integer leaves, power-of-two
    total and B: every fp32 operation behind k + xi is exact) tol = 0 and the index IS that index — targets exactly on leaf boundaries and on the edge of a
    dead stretch included (u == left goes right; a zero right child is never entered).  The batch kernel draws its own xi: the same stream is written with
    a0_rng_uniform and handed to the reference as input.
  * Priorities.  (loss + eps)^alpha: the sum is one fp32 addition, taken as the kernel takes it.  alpha = 0.5: the kernel rounds a double square root
    once, which is the correctly rounded fp32 root (53 >= 2 * 24 + 2): bound zero.  Any other alpha goes through powf, whose error the code does not tell.
    MEASURED on an MI355X over this file's priority cases (losses 0 .. 2e4) against the float64 power: 1.177 ulp at alpha = 0.6, 1.083 ulp at 0.25, 1.000 ulp
    at alpha = 1 (POWF_MEASURED_ULP of tests/replay_ref.py); the bound is twice the largest, 2.354 ulp, and never below 2 ulp.  max_p is the exact maximum of the old value and the raw losses.
    a0_priority_tail: fp32(float64(max_p) ** float64(alpha)) within 1 ulp (device double pow is not correctly rounded).
  * Importance weights, relative: the division p / total and the product with top (2 U on powf's argument, amplified by beta), powf (POWF_ULP ulps of at
    most 2 U), the same once more for the element the maximum picks, the sum with 1e-8 and the final division (2 U); doubled (MARGIN).
  * a0_sum_f32: (ceil(n / 65536) + 8 + 1 + 8) 2^-24 sum |x|, doubled: a lane's chain, stage 1's tree, stage 2's one addition per lane and its tree."""
import numpy as np
import pytest
import torch

import replay_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 8
SENT = -7.25


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


def D(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


class _Guarded:
    """values followed by GUARD sentinel floats; ``view`` is what the kernel gets."""

    def __init__(self, hip, values):
        values = np.ascontiguousarray(values, F32)
        host = np.full(values.size + GUARD, SENT, F32)
        host[:values.size] = values
        self.full = D(hip, host)
        self.n = values.size
        self.view = self.full[:self.n]

    def host(self):
        return self.view.cpu().numpy()

    def guard_ok(self):
        return bool((self.full[self.n:] == SENT).all())


def _assert_tree(got, want, what, lo=1, hi=None):
    bad = R.tree_mismatch(got, want, lo, hi)
    if bad.size:
        print(f"{what}: {bad.size} nodes differ from the tree of the expected leaves, first {bad[:8].tolist()}: got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}")
    assert bad.size == 0, f"{what}: {bad.size} nodes differ, first {bad[:8].tolist()}"


# ------------------------------------------------------------------------------------------------ tree sets
@pytest.mark.parametrize("cap2", R.SET_CAP2)
def test_tree_sets_hold_the_invariants(hip, cap2):
    """a0_sumtree_set, a0_priority_from_loss + a0_sumtree_set, and on the per-wave path a0_sumtree_set_from_loss with the top in the same call and deferred
    (then a0_sumtree_top_rebuild), each on a tree of its own through the same batches.  alpha = 0.5, so the leaves are known to the bit."""
    sub = cap2 in R.SUB_CAP2
    assert hip.sumtree_set_from_loss_ok(cap2) == sub
    entries = ["set", "prio+set"] + (["from_loss", "from_loss_deferred"] if sub else [])
    leaves = R.set_start_leaves(cap2).copy()
    want = R.tree_from_leaves(leaves, cap2)
    trees = {e: _Guarded(hip, want) for e in entries}
    pstate = {e: D(hip, np.ones(1, F32)) for e in entries}
    mp = 1.0
    stale_seen = 0
    for name, (idx, loss) in R.set_batches(cap2).items():
        n = idx.size
        val = R.prio(loss, R.EPS, 0.5)[0].astype(F32)
        old = want
        leaves = R.last_wins(leaves, idx, val)
        want = R.tree_from_leaves(leaves, cap2)
        mp = R.max_p(mp, loss)
        d_idx, d_loss, d_val = D(hip, idx), D(hip, loss), D(hip, val)
        for e in entries:
            t = trees[e]
            what = f"cap2 {cap2} {name} {e}"
            if e == "set":
                hip.sumtree_set(t.view, cap2, d_idx, d_val, n)
            elif e == "prio+set":
                buf = _Guarded(hip, np.zeros(n, F32))
                hip.priority_from_loss(d_loss, n, R.EPS, 0.5, buf.view, pstate[e])
                assert np.array_equal(R.bits(buf.host()), R.bits(val)) and buf.guard_ok(), f"{what}: the staged priorities"
                hip.sumtree_set(t.view, cap2, d_idx, buf.view, n)
            elif e == "from_loss":
                hip.sumtree_set_from_loss(t.view, cap2, d_idx, d_loss, n, R.EPS, 0.5, pstate[e])
            else:
                hip.sumtree_set_from_loss(t.view, cap2, d_idx, d_loss, n, R.EPS, 0.5, pstate[e], defer_top=True)
                got = t.host()
                _assert_tree(got, want, what + ": at and below the level of 2048 nodes", R.ST_TOP)
                _assert_tree(got, old, what + ": the deferred levels keep the bits they had", 1, R.ST_TOP)
                stale_seen += int(R.tree_mismatch(got, want, 1, R.ST_TOP).size > 0)
                hip.sumtree_top_rebuild(t.view, cap2)
            torch.cuda.synchronize()
            got = t.host()
            _assert_tree(got, want, what)
            assert got[0] == 0 and t.guard_ok(), f"{what}: tree[0] and the floats behind the tree"
            if e != "set":
                assert float(pstate[e][0]) == mp, f"{what}: max_p {float(pstate[e][0])!r}, the exact maximum is {mp!r}"
    print(f"cap2 {cap2}: {len(entries)} entries x {len(R.set_batches(cap2))} batches, every node bit-equal to the tree of the expected leaves")
    assert not sub or stale_seen >= 8, "the deferred calls left the top stale"
    assert R.tree_violations(want, cap2).size == 0
    # a0_sumtree_top_rebuild on its own: the levels it owns are overwritten with garbage first (below 4096 leaves: every internal node — it is a full rebuild)
    t = trees["set"]
    hi = cap2 if cap2 < 2 * R.ST_TOP else R.ST_TOP
    if hi > 1:
        t.view[1:hi] = 3.5
    hip.sumtree_top_rebuild(t.view, cap2)
    torch.cuda.synchronize()
    _assert_tree(t.host(), want, f"cap2 {cap2} a0_sumtree_top_rebuild")
    assert t.guard_ok() and float(t.view[0]) == 0
    if cap2 < 2 * R.ST_TOP:
        full = _Guarded(hip, want)
        if cap2 > 1:
            full.view[1:cap2] = 3.5
        hip.sumtree_rebuild(full.view, cap2)
        torch.cuda.synchronize()
        assert torch.equal(full.full.view(torch.int32), t.full.view(torch.int32)), "below 4096 leaves a0_sumtree_top_rebuild equals a full rebuild"


@pytest.mark.parametrize("cap2,back,n", R.RANGE_CASES)
def test_range_set_on_a_wrapping_range(hip, cap2, back, n):
    size, start, idx = R.range_case(cap2, back, n)
    leaves = R.set_start_leaves(cap2).copy()
    t = _Guarded(hip, R.tree_from_leaves(leaves, cap2))
    hip.sumtree_set_range(t.view, cap2, start, n, size, D(hip, np.array([1.25], F32)))
    torch.cuda.synchronize()
    leaves[idx] = 1.25
    assert start + n > size
    got = t.host()
    assert np.array_equal(R.bits(got[cap2:]), R.bits(leaves)), "the leaves: the range, wrapped, and nothing else"
    _assert_tree(got, R.tree_from_leaves(leaves, cap2), f"cap2 {cap2} range [{start}, {start} + {n}) of {size}")
    assert got[0] == 0 and t.guard_ok()


# ------------------------------------------------------------------------------------------------ sampling
class _Ring:
    """What the fused walkers read beside the tree: 16-byte rows and metadata that name their own slot — one per leaf of the tree, the zero tail included, so
    that a walk that strays into the tail reads inside the buffers and is reported by the checks."""

    def __init__(self, hip, cap):
        self.hip, self.cap = hip, cap
        slot = torch.arange(cap, dtype=torch.int32, device=hip.device)
        self.frames = slot.repeat_interleave(4).view(torch.uint8)
        self.r_act, self.r_rew, self.r_done = slot, slot.to(torch.float32), (slot % 2).to(torch.float32)

    def outputs(self, B):
        hip = self.hip
        return dict(idx=hip.zeros(B, dtype=torch.int64), slot=hip.zeros(B, dtype=torch.int32), act=hip.zeros(B, dtype=torch.int32), rew=hip.zeros(B),
                    done=hip.zeros(B), prio=hip.zeros(B), w=hip.zeros(B))

    def check_rows(self, o, what, rows=None):
        idx = o["idx"].cpu().numpy()
        assert np.array_equal(o["slot"].cpu().numpy(), idx) and np.array_equal(o["act"].cpu().numpy(), idx), f"{what}: slot and action of the sampled leaf"
        assert np.array_equal(o["done"].cpu().numpy(), (idx % 2).astype(F32)) and np.array_equal(o["rew"].cpu().numpy(), idx.astype(F32)), f"{what}: reward and done"
        if rows is not None:
            assert np.array_equal(rows.view(torch.int32).view(-1, 4).cpu().numpy(), np.repeat(idx[:, None], 4, 1).astype(np.int32)), f"{what}: the gathered rows"


def _walk(hip, walker, tree, cap2, size, ring, B, xi=None, beta=0.4, rng=R.BATCH_RNG):
    """-> (xi as the reference's input, leaf indices, priorities, weights or None)."""
    if walker == "sample":
        idx, p = hip.zeros(B, dtype=torch.int64), hip.zeros(B)
        hip.sumtree_sample(tree, cap2, D(hip, xi), B, idx, p)
        return xi, idx.cpu().numpy(), p.cpu().numpy(), None
    o = ring.outputs(B)
    if walker == "gather":
        rows = torch.zeros(B * 16, dtype=torch.uint8, device=hip.device)
        hip.replay_sample_gather(1, 0, 0, 0, tree, cap2, D(hip, xi), size, 0, cap2, ring.frames, 16, ring.r_act, ring.r_rew, ring.r_done, None, B, rows,
                                 o["idx"], o["slot"], o["act"], o["rew"], o["done"], o["prio"])
        ring.check_rows(o, f"a0_replay_sample_gather B {B}", rows)
        return xi, o["idx"].cpu().numpy(), o["prio"].cpu().numpy(), None
    d_xi = hip.zeros(B)
    hip.rng_uniform(*rng, d_xi, B)
    hip.sumtree_sample_batch(*rng, tree, cap2, B, size, size, beta, ring.r_act, ring.r_rew, ring.r_done, o["idx"], o["slot"], o["act"], o["rew"], o["done"], o["prio"], o["w"])
    ring.check_rows(o, f"a0_sumtree_sample_batch B {B}")
    return d_xi.cpu().numpy(), o["idx"].cpu().numpy(), o["prio"].cpu().numpy(), o["w"].cpu().numpy()


WALKERS = ("sample", "gather", "batch")


@pytest.mark.parametrize("cap2", R.EXACT_CAP2)
def test_sampling_on_exact_trees_is_the_float64_index(hip, cap2):
    draws = 0
    for B in R.EXACT_B:
        T = R.exact_tree(cap2, B)
        host = R.tree_from_leaves(T["leaves"], cap2)
        tree = D(hip, host)
        assert float(host[1]) == T["total"]
        ring = _Ring(hip, cap2)
        for walker in WALKERS:
            for x in (R.EXACT_XI if walker != "batch" else (None,)):
                xi, idx, p, _ = _walk(hip, walker, tree, cap2, T["size"], ring, B, None if x is None else np.full(B, x, F32))
                res = R.sample_check(T["leaves"], cap2, xi, B, idx, p, exact=True)
                assert res["ok"], f"cap2 {cap2} B {B} {walker} xi {x}: {res['message']}"
                draws += B
                if x == 0.0 and B > 1:
                    assert idx[T["edge_k"]] >= T["dead"][1], "the draw that targets the edge of the dead stretch lands behind it"
    print(f"cap2 {cap2}: {draws} draws, every index the float64 index")


@pytest.mark.parametrize("size", R.GENERAL_SIZES)
def test_sampling_stays_inside_the_interval_bound_and_the_cap(hip, size):
    T = R.general_tree(size)
    cap2, leaves = T["cap2"], T["leaves"]
    tree = D(hip, R.tree_from_leaves(leaves, cap2))
    ring = _Ring(hip, cap2) if size < 3_000_000 else None
    for walker in (WALKERS if ring else WALKERS[:1]):
        for B in (R.GENERAL_B_BATCH if walker == "batch" else R.GENERAL_B):
            xi, idx, p, _ = _walk(hip, walker, tree, cap2, size, ring, B, None if walker == "batch" else R.general_xi(size, B))
            res = R.sample_check(leaves, cap2, xi, B, idx, p, exact=False)
            print(f"size {size} {walker} B {B}: worst draw at {res['worst']:.4f} of tol, {100 * res['mismatch']:.2f} % off the float64 index (cap {100 * R.MISMATCH_CAP:.0f} %)")
            assert res["ok"], f"size {size} {walker} B {B}: {res['message']}"
            assert res["mismatch"] <= R.MISMATCH_CAP, f"size {size} {walker} B {B}: {100 * res['mismatch']:.2f} % of the draws differ from the float64 index"


# ------------------------------------------------------------------------------------------------ priorities
def _ulps(got, want):
    return float((np.abs(np.asarray(got, np.float64) - want) / R.ulp(want)).max())


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_priorities_against_float64(hip, alpha):
    """a0_priority_update, a0_priority_from_loss and a0_sumtree_set_from_loss.  powf's worst error over these cases, measured on an MI355X: 1.177 ulp (alpha 0.6),
    1.000 ulp (alpha 1), 1.083 ulp (alpha 0.25); alpha = 0.5 is exact."""
    cap2 = 1 << 17
    measured, frac_worst = 0.0, 0.0
    for B in R.PRIO_B + (2048,):
        for variant in range(4 if B == 1 else 1):
            ids, loss = R.prio_case(B, variant)
            want, bound = R.prio(loss, R.EPS, alpha)
            mp = R.max_p(1.0, loss)
            d_ids, d_loss = D(hip, ids), D(hip, loss)
            what = f"alpha {alpha} B {B} variant {variant}"
            ref_vec, bound_vec = np.ones(4096), np.zeros(4096)
            for i, v, b in zip(ids.tolist(), want, bound):
                ref_vec[i], bound_vec[i] = v, b
            # the flat priority vector
            prio, ps = _Guarded(hip, np.ones(4096, F32)), D(hip, np.ones(1, F32))
            hip.priority_update(prio.view, d_ids, d_loss, B, R.EPS, alpha, ps, None)
            torch.cuda.synchronize()
            frac, msg = R.worst("a0_priority_update", prio.host(), ref_vec, bound_vec)
            assert frac <= 1.0 and prio.guard_ok(), f"{what}: {msg}"
            assert float(ps[0]) == mp, f"{what}: a0_priority_update max_p {float(ps[0])!r}, the exact maximum is {mp!r}"
            measured, frac_worst = max(measured, _ulps(prio.host()[ids], ref_vec[ids])), max(frac_worst, frac)
            if B > 1024:
                continue
            # the staged values
            val, ps = _Guarded(hip, np.zeros(B, F32)), D(hip, np.ones(1, F32))
            hip.priority_from_loss(d_loss, B, R.EPS, alpha, val.view, ps)
            torch.cuda.synchronize()
            frac, msg = R.worst("a0_priority_from_loss", val.host(), want, bound, dict(loss=loss))
            assert frac <= 1.0 and val.guard_ok(), f"{what}: {msg}"
            assert float(ps[0]) == mp, f"{what}: a0_priority_from_loss max_p"
            measured, frac_worst = max(measured, _ulps(val.host(), want)), max(frac_worst, frac)
            # the tree's leaves
            for defer in (False, True):
                t, ps = _Guarded(hip, R.tree_from_leaves(np.ones(4096, F32), cap2)), D(hip, np.ones(1, F32))
                hip.sumtree_set_from_loss(t.view, cap2, d_ids, d_loss, B, R.EPS, alpha, ps, defer_top=defer)
                if defer:
                    hip.sumtree_top_rebuild(t.view, cap2)
                torch.cuda.synchronize()
                got = t.host()
                frac, msg = R.worst("a0_sumtree_set_from_loss", got[cap2:cap2 + 4096], ref_vec, bound_vec)
                assert frac <= 1.0 and t.guard_ok() and not got[cap2 + 4096:].any(), f"{what} defer {defer}: {msg}"
                assert R.tree_violations(got, cap2).size == 0, f"{what} defer {defer}: internal nodes"
                assert float(ps[0]) == mp, f"{what}: a0_sumtree_set_from_loss max_p"
                measured, frac_worst = max(measured, _ulps(got[cap2 + ids], ref_vec[ids])), max(frac_worst, frac)
    print(f"alpha {alpha}: worst error {measured:.3f} ulp against the float64 power (bound {0.0 if alpha == 0.5 else R.POWF_ULP} ulp), worst fraction of the bound {frac_worst:.3f}")
    assert measured <= (0.5 if alpha == 0.5 else R.POWF_ULP)


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_priority_tail_against_pythons_power(hip, alpha):
    for mp in R.TAIL_MAX_P:
        size, n = 1000, 7
        prio, ps = _Guarded(hip, np.full(size, 0.5, F32)), D(hip, np.array([mp], F32))
        hip.priority_tail(prio.view, size, n, ps, alpha)
        torch.cuda.synchronize()
        v, b = R.priority_tail(mp, alpha)
        got = prio.host()
        print(f"alpha {alpha} max_p {mp}: {float(got[-1])!r}, python {v!r}, {abs(float(got[-1]) - v) / b:.3f} of its bound")
        assert (got[:size - n] == 0.5).all() and prio.guard_ok() and (got[size - n:] == got[-1]).all()
        assert abs(float(got[-1]) - v) <= b, f"alpha {alpha} max_p {mp}: {float(got[-1])!r}, python {v!r}"


# ------------------------------------------------------------------------------------------------ importance weights
def _check_weights(what, got, p, total, top, beta):
    w, bound = R.is_weights(p, total, top, beta)
    frac, msg = R.worst("w", got, w, bound, dict(p=p))
    assert frac <= 1.0, f"{what}: {msg}"
    return frac


@pytest.mark.parametrize("B", R.WEIGHT_B + (2048,))
def test_is_weights_against_float64(hip, B):
    worst = 0.0
    cases = [(f"{kind} beta {beta}", *R.weights_case(B, kind), beta) for kind in R.WEIGHT_KINDS for beta in R.BETAS]
    if B == 1:
        cases.append(("dominant", R.DOMINANT["p"], R.DOMINANT["total"], R.DOMINANT["top"], R.DOMINANT["beta"]))
    for what, p, total, top, beta in cases:
        w = _Guarded(hip, np.zeros(B, F32))
        hip.is_weights(D(hip, p), B, D(hip, np.array([total], F32)), top, beta, w.view)
        torch.cuda.synchronize()
        assert w.guard_ok()
        worst = max(worst, _check_weights(f"B {B} {what}", w.host(), p, total, top, beta))
        if B == 2048:
            assert beta == 0 or int(w.host().argmax()) == 1500, f"B {B} {what}: the largest weight belongs to entry 1500"
    print(f"a0_is_weights B {B}: worst fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["general-3000", "general-300000", "equal", "dominant"])
def test_sample_batch_weights_against_float64(hip, kind):
    """The weights of a0_sumtree_sample_batch from the priorities it returns and the root it read.  A leaf at 1e-6 of the total cannot be made to be drawn by
    a kernel that draws its own xi: that case is a0_is_weights' alone."""
    if kind == "dominant":
        size = 1_000_000
        leaves = np.full(1 << 20, 1e-6, F32)
        leaves[size:] = 0
        leaves[123_457] = 1e6
        runs = [(1, 1.0)]
    elif kind == "equal":
        size = 3000
        leaves = np.zeros(4096, F32)
        leaves[:size] = 0.7
        runs = [(B, beta) for B in R.WEIGHT_B for beta in R.BETAS]
    else:
        T = R.general_tree(int(kind.split("-")[1]))
        size, leaves = T["size"], T["leaves"]
        runs = [(B, beta) for B in R.WEIGHT_B for beta in R.BETAS]
    cap2 = leaves.size
    host = R.tree_from_leaves(leaves, cap2)
    tree, ring = D(hip, host), _Ring(hip, cap2)
    worst = 0.0
    for B, beta in runs:
        _, idx, p, w = _walk(hip, "batch", tree, cap2, size, ring, B, beta=beta)
        assert np.array_equal(R.bits(p), R.bits(leaves[idx]))
        worst = max(worst, _check_weights(f"{kind} B {B} beta {beta}", w, p, host[1], size, beta))
    if kind == "dominant":
        assert idx[0] == 123_457 and abs(float(w[0]) - 1e-6 / (1e-6 + 1e-8)) < 1e-6, f"w = {float(w[0])!r}"
    print(f"a0_sumtree_sample_batch {kind}: worst fraction of the bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ a0_sum_f32
@pytest.mark.parametrize("n", R.SUM_NS)
def test_sum_f32_against_float64(hip, n):
    x = R.sum_case(n)
    out, scratch = _Guarded(hip, np.zeros(1, F32)), _Guarded(hip, np.zeros(256, F32))
    hip.sum_f32(D(hip, x), n, scratch.view, out.view)
    torch.cuda.synchronize()
    s, bound = R.sum_f32(x)
    got = float(out.host()[0])
    print(f"n {n}: sum {got!r}, float64 {s!r}, {abs(got - s) / bound:.3f} of its bound")
    assert abs(got - s) <= bound and out.guard_ok() and scratch.guard_ok(), f"n {n}: {got!r} against {s!r}, bound {bound:.3e}"
