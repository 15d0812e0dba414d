"""CPU: the yardstick of tests/test_gpu_replay_reference.py (tests/replay_ref.py) against what the project already trusts.

  * the tree invariants, the interval check, the exact-index check and the 5 % cap against oracle.core.SumTree (set, rebuild, sample) at every tree case
    the GPU test runs, and against core.sumtree_set_numpy / core.sumtree_find_numpy;
  * the priorities and max_p against oracle.replay.ReferenceReplay, the importance weights against oracle.replay.is_weights (the torch forms of the
    reference's replay.py and trainer.py);
  * a hand-written table;
  * the fp32 restatements of every kernel within HALF of every bound, on every case the GPU test runs;
  * seven deliberately wrong computations, each rejected on a listed case."""
import numpy as np
import pytest

import replay_ref as R
import recipe
from oracle import core
from oracle import replay as oreplay

F32 = np.float32


def _oracle_tree(cap2, leaves):
    t = core.SumTree(R.set_size(cap2) if cap2 > 2 else cap2)
    assert t.cap2 == cap2
    t.tree[cap2:] = leaves
    t.rebuild()
    return t


# ------------------------------------------------------------------------------------------------ the tree
@pytest.mark.parametrize("cap2", R.SET_CAP2)
def test_the_oracles_set_and_rebuild_hold_the_tree_invariants(cap2):
    leaves = R.set_start_leaves(cap2).copy()
    t = _oracle_tree(cap2, leaves)
    assert R.tree_mismatch(t.tree, R.tree_from_leaves(leaves, cap2)).size == 0, "rebuild"
    mirror = t.tree.copy()
    for name, (idx, loss) in R.set_batches(cap2).items():
        val = R.prio(loss, R.EPS, 0.5)[0].astype(F32)
        assert val.min() >= 0 and (name != "zero_values" or not val.any())
        t.set(idx, val)
        core.sumtree_set_numpy(mirror, cap2, idx, val)
        leaves = R.last_wins(leaves, idx, val)
        want = R.tree_from_leaves(leaves, cap2)
        assert R.tree_mismatch(t.tree, want).size == 0 and R.tree_violations(t.tree, cap2).size == 0, f"{name}: oracle/sumtree.c"
        assert R.tree_mismatch(mirror, want).size == 0, f"{name}: sumtree_set_numpy"


def test_the_set_cases_reach_what_they_name():
    for cap2 in R.SET_CAP2:
        size, B = R.set_size(cap2), R.set_batches(cap2)
        assert [B[f"n={n}"][0].size for n in R.SET_NS] == list(R.SET_NS)
        assert all(0 <= idx.min() and idx.max() < size for idx, _ in B.values())
        assert {0, size - 1} <= set(B["leaves_0_and_size-1"][0].tolist())
        assert len(set(B["one_leaf_1024_times"][0].tolist())) == 1 and len(set(B["one_leaf_1024_times"][1].tolist())) > 1000
    for cap2 in R.SUB_CAP2:
        S = cap2 // R.ST_TOP
        M = S // 64
        B = R.set_batches(cap2)
        assert len(set((B["one_subtree"][0] // S).tolist())) == 1
        border = B["subtree_border"][0]
        assert {S - 1, 0} <= set((border % S).tolist()) and len(set((border // S).tolist())) >= 4
        assert {0, M - 1, M % S, S - 1} <= set((B["lane_border"][0] % S).tolist())
    assert sorted(c // R.ST_TOP // 64 for c in R.SUB_CAP2) == [1, 2, 4, 8, 16]
    for cap2, back, n in R.RANGE_CASES:
        size, start, idx = R.range_case(cap2, back, n)
        assert start + n > size and idx[0] == start and idx[-1] == n - back - 1 and len(set(idx.tolist())) == n


@pytest.mark.parametrize("cap2,back,n", R.RANGE_CASES)
def test_the_oracles_set_on_a_wrapping_range(cap2, back, n):
    leaves = R.set_start_leaves(cap2).copy()
    t = _oracle_tree(cap2, leaves)
    _, _, idx = R.range_case(cap2, back, n)
    t.set(idx, np.full(n, 1.25, F32))
    leaves[idx] = 1.25
    assert R.tree_mismatch(t.tree, R.tree_from_leaves(leaves, cap2)).size == 0


# ------------------------------------------------------------------------------------------------ sampling
def _oracle_sample(leaves, cap2, xi):
    t = core.SumTree(cap2)
    t.tree[cap2:] = leaves
    t.rebuild()
    return t, t.sample(xi)


@pytest.mark.parametrize("cap2", R.EXACT_CAP2)
def test_the_oracle_matches_the_float64_index_on_the_exact_trees(cap2):
    for B in R.EXACT_B:
        T = R.exact_tree(cap2, B)
        a, b = T["dead"]
        assert set(np.unique(T["leaves"][:T["size"] - 1]).tolist()) <= {0.0, 1.0, 2.0, 4.0} and not T["leaves"][a:b].any() and b - a >= T["size"] // 8
        assert not T["leaves"][T["size"]:].any() and float(T["leaves"].astype(np.float64).sum()) == T["total"] == 2.0 ** round(np.log2(T["total"]))
        assert (T["edge_k"] is not None) == (B > 1)
        for x in R.EXACT_XI:
            xi = np.full(B, x, F32)
            t, (idx, p) = _oracle_sample(T["leaves"], cap2, xi)
            assert float(t.total) == T["total"]
            res = R.sample_check(T["leaves"], cap2, xi, B, idx, p, exact=True)
            assert res["ok"], f"cap2 {cap2} B {B} xi {x}: {res['message']}"
            i32, p32 = R.walk32(t.tree, cap2, xi, B)
            assert np.array_equal(i32, idx) and np.array_equal(p32, p), "walk32 is the oracle's walk"
            xi = core.rng_uniform(*R.BATCH_RNG, B)                       # the batch kernel's own xi: k + xi rounds, nothing else does
            _, (idx, p) = _oracle_sample(T["leaves"], cap2, xi)
            res = R.sample_check(T["leaves"], cap2, xi, B, idx, p, exact=True)
            assert res["ok"], f"cap2 {cap2} B {B} Philox xi: {res['message']}"
            if x == 0.0 and B > 1:
                k = T["edge_k"]
                c = np.cumsum(T["leaves"].astype(np.float64))
                assert c[a - 1] == k * T["total"] / B and idx[k] >= b and T["leaves"][a - 1] > 0, "a stratum boundary on the dead stretch's edge: the draw lands behind it"
                on_boundary = np.isin(np.arange(B) * T["total"] / B, c)
                assert on_boundary.sum() >= 8,"targets exactly on leaf boundaries"


@pytest.mark.parametrize("size", R.GENERAL_SIZES)
def test_the_oracle_stays_inside_the_interval_bound_and_the_cap(size):
    T = R.general_tree(size)
    cap2, leaves = T["cap2"], T["leaves"]
    assert cap2 > size and not leaves[size:].any() and not leaves[T["dead"][0]:T["dead"][1]].any() and 0.25 < (leaves[:size] == 0).mean() < 0.7
    for B in sorted(set(R.GENERAL_B + R.GENERAL_B_BATCH)):
        xi = R.general_xi(size, B)
        assert xi[0] == 0 and xi[-1] == F32(1 - 2.0 ** -24) and xi.max() < 1
        t, (idx, p) = _oracle_sample(leaves, cap2, xi)
        res = R.sample_check(leaves, cap2, xi, B, idx, p, exact=False)
        print(f"size {size} B {B}: worst draw at {res['worst']:.4f} of tol, {100 * res['mismatch']:.2f} % off the float64 index")
        assert res["ok"], f"size {size} B {B}: {res['message']}"
        assert res["worst"] <= 0.5 and res["mismatch"] <= R.MISMATCH_CAP
        i32, p32 = R.walk32(t.tree, cap2, xi, B)
        assert np.array_equal(i32, idx) and np.array_equal(p32, p), "walk32 is the oracle's walk"
    if size < 3_000_000:                          # the xi the batch kernel draws for itself, from the oracle's Philox
        for B in R.GENERAL_B_BATCH:
            xi = core.rng_uniform(*R.BATCH_RNG, B)
            _, (idx, p) = _oracle_sample(leaves, cap2, xi)
            res = R.sample_check(leaves, cap2, xi, B, idx, p, exact=False)
            assert res["ok"] and res["worst"] <= 0.5 and res["mismatch"] <= R.MISMATCH_CAP, f"size {size} B {B} (Philox xi): {res['mismatch']} {res['message']}"
    for k in (0, 7, 63):                          # the scalar numpy mirror, draw by draw
        seg = F32(t.tree[1] / F32(64))
        u = F32(F32(F32(k) + R.general_xi(size, 64)[k]) * seg)
        assert core.sumtree_find_numpy(t.tree, cap2, u) == _oracle_sample(leaves, cap2, R.general_xi(size, 64))[1][0][k]


def test_the_tolerance_pins_a_draw_to_a_handful_of_leaves():
    T = R.general_tree(1_000_000)
    total = float(T["leaves"].astype(np.float64).sum())
    assert R.sample_tol(T["cap2"], total) < 8 * total / 1_000_000


# ------------------------------------------------------------------------------------------------ priorities and weights against the reference's torch forms
@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_prio_and_max_p_are_the_reference_replays(alpha):
    """The reference's torch form takes the exponent as the fp32 number the kernel receives.  At alpha = 0.5 torch's vectorised CPU pow is within one ulp of
    the correctly rounded root (it is not always that root: 1.2048439 ** 0.5 comes out one ulp low), the numpy fp32 root is the root itself."""
    for B in R.PRIO_B + (2048,):
        for variant in range(4 if B == 1 else 1):
            ids, loss = R.prio_case(B, variant)
            rp = oreplay.ReferenceReplay(4096, True, alpha=float(F32(alpha)), eps=R.EPS)
            rp.update_priority(ids, loss)
            want, bound = R.prio(loss, R.EPS, alpha)
            assert np.isfinite(want).all() and want.min() >= 0
            base = np.ones(4096, F32)
            allowed = R.ulp(want) if alpha == 0.5 else 0.5 * bound
            frac, msg = R.worst("priority", rp.priority, _f64_last(base, ids, want), _f64_last(np.ones(4096), ids, allowed), {})
            assert frac <= 1.0, f"alpha {alpha} B {B}: {msg}"
            assert rp.max_p == R.max_p(1.0, loss)
            frac32, msg = R.worst("prio32", R.prio32(loss, R.EPS, alpha), want, bound, dict(loss=loss))
            assert frac32 <= 0.5 and (alpha != 0.5 or frac32 == 0.0), f"alpha {alpha} B {B}: {msg}"
            if B > 1:
                assert want[(loss == -F32(R.EPS))].tolist() == [0.0] and ids[-1] == ids[0] and abs(rp.priority[ids[0]] - want[-1]) <= allowed[-1]


def _f64_last(base, ids, vals):
    out = np.array(base, np.float64, copy=True)
    for i, v in zip(ids.tolist(), np.asarray(vals, np.float64)):
        out[i] = v
    return out


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_priority_tail_is_pythons_power(alpha):
    for mp in R.TAIL_MAX_P:
        rp = oreplay.ReferenceReplay(8, True, alpha=float(F32(alpha)))
        rp.max_p = float(F32(mp))
        rp.extend([None, None])
        v, b = R.priority_tail(mp, alpha)
        assert rp.priority[-1] == rp.priority[-2] == F32(v) and rp.priority[0] == 1.0 and b == float(np.spacing(F32(v)))


def _weight_cases():
    for B in R.WEIGHT_B + (2048,):
        for kind in R.WEIGHT_KINDS:
            for beta in R.BETAS:
                yield (f"B {B} {kind} beta {beta}", *R.weights_case(B, kind), beta)
    D = R.DOMINANT
    yield "dominant", D["p"], D["total"], D["top"], D["beta"]


def test_is_weights_is_the_reference_trainers_and_fp32_stays_within_half_of_the_bound():
    worst = 0.0
    for what, p, total, top, beta in _weight_cases():
        w, bound = R.is_weights(p, total, top, beta)
        assert np.isfinite(w).all() and w.max() <= 1.0 and (bound > 0).all()
        for name, got in (("oracle.replay.is_weights", oreplay.is_weights(p, F32(total), top, float(F32(beta)))), ("is_weights32", R.is_weights32(p, total, top, beta))):
            frac, msg = R.worst(name, got, w, bound, dict(p=p))
            assert frac <= 0.5, f"{what}: {msg}"
            worst = max(worst, frac)
    assert worst > 0.02, f"bound far wider than an fp32 evaluation needs: worst fraction {worst}"
    assert abs(R.is_weights(**R.DOMINANT)[0][0] - 1e-6 / (1e-6 + 1e-8)) < 1e-7


@pytest.mark.parametrize("n", R.SUM_NS)
def test_sum_f32_restatement_stays_within_half_of_the_bound(n):
    x = R.sum_case(n)
    s, bound = R.sum_f32(x)
    assert np.log2(np.abs(x).max() / np.abs(x).min()) > (9 if n > 200 else -1)
    got = float(R.sum_f32_32(x))
    assert abs(s - float(np.sum(x.astype(np.float64)))) == 0 and abs(got - s) <= 0.5 * bound, f"n {n}: {got!r} against {s!r}, bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------ a hand-written table
HAND_LEAVES = (1, 0, 2, 1, 0, 0, 4, 0)          # c = 0 1 1 3 4 4 4 8 8; B = 8: u_k = k + xi
HAND_DRAWS = ((0.0, (0, 2, 2, 3, 6, 6, 6, 6)), (0.5, (0, 2, 2, 3, 6, 6, 6, 6)), (0.875, (0, 2, 2, 3, 6, 6, 6, 6)))
HAND_PRIO = ((0.1875, 0.0625, 0.5, 0.5), (0.1875, 0.0625, 1.0, 0.25), (15.9375, 0.0625, 0.25, 2.0), (-0.0625, 0.0625, 0.25, 0.0), (0.0, 0.0625, 0.5, 0.25))
HAND_WEIGHTS = (((1.0, 4.0), 8.0, 2, 1.0, (1.0, 0.25)), ((1.0, 4.0), 8.0, 2, 0.5, (1.0, 0.5)), ((1.0, 4.0), 8.0, 2, 0.0, (1.0, 1.0)))
HAND_TREE = (0, 8, 4, 4, 1, 3, 0, 4, 1, 0, 2, 1, 0, 0, 4, 0)


def test_the_hand_written_table():
    leaves = np.array(HAND_LEAVES, F32)
    assert R.tree_from_leaves(leaves, 8).tolist() == list(HAND_TREE)
    for x, want in HAND_DRAWS:
        xi = np.full(8, x, F32)
        res = R.sample_check(leaves, 8, xi, 8, np.array(want), leaves[list(want)], exact=True)
        assert res["ok"] and res["want"].tolist() == list(want), res["message"]
        assert R.walk32(R.tree_from_leaves(leaves, 8), 8, xi, 8)[0].tolist() == list(want)
        off = np.array(want)
        off[1] = 1                                # the dead leaf in front of leaf 2
        assert not R.sample_check(leaves, 8, xi, 8, off, leaves[off], exact=True)["ok"]
    for loss, eps, alpha, want in HAND_PRIO:
        v, b = R.prio(np.array([loss], F32), eps, alpha)
        assert abs(v[0] - want) <= b[0] and (alpha != 0.5 or v[0] == want)
    for p, total, top, beta, want in HAND_WEIGHTS:
        w, b = R.is_weights(np.array(p, F32), total, top, beta)
        assert np.abs(w - np.array(want)).max() < 1e-8 and (b < 1e-5).all()
    assert R.last_wins(np.zeros(4, F32), [1, 3, 1], [5.0, 6.0, 7.0]).tolist() == [0, 7, 0, 6]
    assert R.max_p(1.0, [0.5, 0.25]) == 1.0 and R.max_p(1.0, [0.5, 2.25]) == 2.25
    assert R.priority_tail(4.0, 0.5)[0] == 2.0 and R.sum_f32(np.array([1, 2, -4], F32))[0] == -1.0


# ------------------------------------------------------------------------------------------------ the mistakes
def test_wrong_first_duplicate_wins_is_rejected():
    idx, loss = R.set_batches(1 << 19)["one_leaf_1024_times"]
    base = R.set_start_leaves(1 << 19)
    assert R.tree_mismatch(R.WRONG_LEAVES["first_duplicate_wins"](base, idx, loss), R.last_wins(base, idx, loss), 0).size == 1
    ids, loss = R.prio_case(65)
    want = R.prio(loss, R.EPS, 0.5)[0]
    assert not np.array_equal(R.WRONG_LEAVES["first_duplicate_wins"](np.ones(4096, F32), ids, want), R.last_wins(np.ones(4096, F32), ids, want))


@pytest.mark.parametrize("cap2", [32, 1 << 17])
def test_wrong_walk_that_sends_u_equal_left_to_the_left_is_rejected(cap2):
    T = R.exact_tree(cap2, 64)
    tree = R.tree_from_leaves(T["leaves"], cap2)
    xi = np.zeros(64, F32)
    idx, p = R.walk32(tree, cap2, xi, 64, **R.WRONG_WALK["u_le_left_goes_left"])
    assert not R.sample_check(T["leaves"], cap2, xi, 64, idx, p, exact=True)["ok"]
    idx, p = R.walk32(tree, cap2, xi, 64)
    assert R.sample_check(T["leaves"], cap2, xi, 64, idx, p, exact=True)["ok"]


def test_wrong_walk_without_the_right_guard_is_rejected():
    """xi[-1] = 1 - 2^-24: (B - 1) + xi rounds to B and u to the root itself.  On the 24-leaf tree every subtraction is then exact enough for u to stay at
    the right edge and an unguarded walk ends in the zero tail; on the large trees the roundings of u -= left may or may not pull it back into a live leaf."""
    rejected = {}
    for size in R.GENERAL_SIZES[:4]:
        T = R.general_tree(size)
        tree = R.tree_from_leaves(T["leaves"], T["cap2"])
        for B in R.GENERAL_B:
            xi = R.general_xi(size, B)
            idx, p = R.walk32(tree, T["cap2"], xi, B, **R.WRONG_WALK["no_right_guard"])
            res = R.sample_check(T["leaves"], T["cap2"], xi, B, idx, p, exact=False)
            rejected[size, B] = not res["ok"]
            assert res["ok"] or (idx[-1] >= size and p[-1] == 0)
    assert all(rejected[24, B] for B in R.GENERAL_B), rejected


def test_a_walk_shifted_by_one_leaf_is_caught_by_the_cap_or_the_interval():
    T = R.general_tree(300_000)
    tree = R.tree_from_leaves(T["leaves"], T["cap2"])
    xi = R.general_xi(300_000, 512)
    idx, _ = R.walk32(tree, T["cap2"], xi, 512)
    live = np.nonzero(T["leaves"] > 0)[0]
    shifted = live[np.minimum(np.searchsorted(live, idx) + 1, live.size - 1)]          # the next live leaf
    res = R.sample_check(T["leaves"], T["cap2"], xi, 512, shifted, T["leaves"][shifted], exact=False)
    assert not res["ok"] or res["mismatch"] > R.MISMATCH_CAP


def test_wrong_weights_without_the_1e8_are_rejected():
    D = R.DOMINANT
    w, bound = R.is_weights(**D)
    got = R.WRONG_WEIGHTS["no_1e-8"](**D)
    assert got[0] == 1.0 and abs(got[0] - w[0]) > 1000 * bound[0] and abs(got[0] - w[0]) > 0.009


@pytest.mark.parametrize("alpha", [0.6, 1.0, 0.25])
def test_wrong_priority_with_eps_outside_the_power_is_rejected(alpha):
    ids, loss = R.prio_case(65)
    want, bound = R.prio(loss, R.EPS, alpha)
    frac, _ = R.worst("wrong", R.WRONG_PRIO["eps_outside_the_power"](loss, R.EPS, alpha), want, bound)
    assert frac > 10.0


def test_wrong_block_max_that_drops_lanes_is_rejected():
    """B = 192: a halving reduction from 192 lanes never reaches lane 2 (tests/test_gpu_kernels.py::test_priority_update_keeps_the_max_loss_at_any_batch_size)."""
    ids, loss = R.prio_case(192)
    loss = loss.copy()
    loss[2] = F32(5e4)
    assert R.max_p(1.0, loss) == 5e4 and R.WRONG_MAX["block_max_drops_lanes"](1.0, loss) != 5e4
    ids, loss = R.prio_case(1024)
    assert R.WRONG_MAX["block_max_drops_lanes"](1.0, loss) == R.max_p(1.0, loss), "at a power of two the reduction reaches every lane"


@pytest.mark.parametrize("cap2", [4096, 1 << 19])
def test_wrong_tree_updated_by_delta_is_rejected(cap2):
    leaves = R.set_start_leaves(cap2)
    tree = R.tree_from_leaves(leaves, cap2)
    idx, loss = R.set_batches(cap2)["n=65"]
    got = R.WRONG_TREE["ancestors_by_delta"](tree, cap2, idx, loss)
    assert R.tree_violations(got, cap2).size > 0
    assert R.tree_mismatch(got, R.tree_from_leaves(R.last_wins(leaves, idx, loss), cap2)).size > 0
