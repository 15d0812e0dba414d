"""CPU: the float64 action-selection references of tests/util.py (the yardstick of tests/test_gpu_actor_tail_reference.py) against the oracle's own action
values; the error bound of tests/actor_tail_cases.py against an fp32 restatement of the kernels' arithmetic in their order of additions (which must use
at most a quarter of it, at every case the GPU tests run) and against five wrong computations (each of which it must reject); and the share of envs whose
greedy action the bound leaves undecided."""
import dataclasses

import numpy as np
import pytest
import torch

import actor_tail_cases as C
import recipe
from oracle import nets
from util import action_values64, assert_close, greedy_check, head_from_slabs64, qhead64, round_bf16

RT, AT = 2e-5, 2e-6             # the oracle's fp32 against float64: the tolerances tests/test_oracle_golden.py holds it to
SPARE = 4.0


def _small(name, **kw):
    return dataclasses.replace(recipe.SPECS[name], obs_shape=(4, 36, 36), **kw)


def _params(spec, seed):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in recipe.make_state_dict(spec, seed).items()}


def _slabs_of(x64, W64, nslab):
    """x W^T as nslab partial products over consecutive k ranges, float64 [nslab][rows][N]."""
    K = x64.shape[1]
    edges = [(K * z) // nslab for z in range(nslab + 1)]
    return np.stack([x64[:, a:b] @ W64[:, a:b].T for a, b in zip(edges[:-1], edges[1:])])


def _head_wb(p, spec):
    W, b = [p["head.q_head.weight"]], [p["head.q_head.bias"]]
    if spec.dueling:
        W.append(p["head.value_head.weight"])
        b.append(p["head.value_head.bias"])
    return torch.cat(W).double().numpy(), torch.cat(b).double().numpy()


# c51_duel: SPECS has the dueling c51 head only with NoisyNet on top (c51_duel_noisy); the noise is switched off here, the head is the same
@pytest.mark.parametrize("name,kw", [("dqn_duel", {}), ("c51_duel_noisy", {"noisy": False}), ("qr", {}), ("iqn", {}), ("fqf", {})])
def test_float64_helpers_match_the_oracle_action_values(name, kw):
    spec = _small(name, **kw)
    p = _params(spec, 21)
    B, A = 5, spec.action_dim
    g = recipe.gen(22)
    feat = torch.from_numpy(np.maximum(g.standard_normal((B, spec.feat_dim)), 0).astype(np.float32))
    W1, b1 = p["head.first_dense.weight"].double().numpy(), p["head.first_dense.bias"].double().numpy()
    W2, b2 = _head_wb(p, spec)
    if spec.algo == "dqn":
        want = nets.qval_from_feat(p, spec, feat)
        got, scale = qhead64(feat.numpy(), W1, b1, W2, b2, A, spec.dueling)
        assert_close(got, want, RT, AT, "q")
        assert (scale >= np.abs(got)).all()
        return
    if spec.algo in ("c51", "qr"):
        T, mode = spec.num_atoms, (2 if spec.algo == "c51" else 1)
        h = np.maximum(feat.double().numpy() @ W1.T + b1, 0)
        slabs = _slabs_of(h, W2, 3)
        q, qs = head_from_slabs64(slabs, b2, A, T, spec.dueling, 0)
        assert_close(q, nets.head_dist(p, spec, feat), RT, AT, "head")
        aux = nets.c51_atoms(spec).numpy() if mode == 2 else None
        want = nets.qval_from_feat(p, spec, feat)
    else:
        if spec.algo == "iqn":
            T, mode = 32, 1
            taus = torch.from_numpy(g.random((B, T, 1)).astype(np.float32))
            aux = None
            want = nets.qval_from_feat(p, spec, feat, taus)
        else:
            T, mode = spec.F, 3
            t, taus, _ = nets.fqf_prop_taus(p, spec, feat)
            aux = t[:, :, 0].numpy()
            want = nets.qval_from_feat(p, spec, feat)
        x = nets.cos_features(p, spec, feat, taus).double().numpy()
        h = np.maximum(x @ W1.T + b1, 0)
        slabs = _slabs_of(h, W2, 5)
        q, qs = head_from_slabs64(slabs, b2, A, T, spec.dueling, 1)
        assert_close(q.transpose(0, 2, 1), nets.head_iqn(p, spec, feat, taus), RT, AT, "head")
    got, scale = action_values64(q, mode, aux, qs)
    assert_close(got, want, RT, AT, "qval")
    assert (qs >= np.abs(q)).all() and (scale >= np.abs(got) * (1 - 1e-12)).all()
    assert want.shape == (B, A)


def _judge(values32, ref_values, tol, tie, tied, what, spare=SPARE, degenerate=False):
    """An fp32 evaluation inside a quarter of the bound, element by element, and its first maxima accepted by greedy_check at the whole bound."""
    err = np.abs(values32.astype(np.float64) - ref_values)
    worst = float((err / tol).max())
    assert worst * spare <= 1.0, f"{what}: the fp32 restatement uses {worst:.3f} of the bound"
    a, qm = C.first_max(values32)
    share = greedy_check(ref_values, tol, a, qm, what, exclude=tied, tie=tie, allow_empty=len(tied) == 1 or ref_values.shape[1] == 2 or degenerate)
    assert share <= C.MAX_UNDECIDED, f"{what}: {share:.1%} of the envs undecided"
    assert (a[tied] == ref_values.argmax(1)[tied]).all()          # the first of the equal maxima (the pair's lower index unless an earlier action equals it too)
    return worst


@pytest.mark.parametrize("kt,case", [(0, c) for c in C.DIST_CASES] + [(1, c) for c in C.QUANTILE_CASES], ids=lambda v: C.case_id(v) if isinstance(v, tuple) else f"kt{v}")
def test_fp32_restatement_of_the_tails_stays_inside_the_bound(kt, case):
    A, T, dueling, mode = case[:4]
    r = C.tail_reference(case, kt)
    q32 = C.head_from_slabs32(r["slabs"], r["bias"], A, T, dueling, kt)
    _judge(C.action_values32(q32, mode, r["aux"]), r["values"], r["tol"], r["tie"], r["tied"], C.case_id(case))


@pytest.mark.parametrize("E", C.QHEAD_ES)
@pytest.mark.parametrize("A,dueling", C.QHEAD_HEADS)
def test_fp32_restatement_of_the_scalar_head_stays_inside_the_bound(A, dueling, E):
    r = C.qhead_reference(E, C.QHEAD_K, A, dueling)
    for ns in C.QHEAD_SPLITS:
        v32 = C.qhead32(r["feat"], r["W1"], r["b1"], r["W2"], r["b2"], A, dueling, ns)
        _judge(v32, r["values"], C.qhead_tol(ns, A, dueling, r["vscale"]), r["tie"], r["tied"], f"qhead A={A} E={E} splits={ns}")


@pytest.mark.parametrize("A,dueling,E", C.QHEAD_ENV_CASES)
def test_fp32_restatement_of_the_merged_scalar_head_stays_inside_the_bound(A, dueling, E):
    r = C.qhead_reference(E, C.QHEAD_ENV_K, A, dueling)
    ns = C.fc1_splits(E, C.QHEAD_ENV_K)
    v32 = C.qhead32(r["feat"], r["W1"], r["b1"], r["W2"], r["b2"], A, dueling, ns)
    _judge(v32, r["values"], C.qhead_tol(ns, A, dueling, r["vscale"]), r["tie"], r["tied"], f"qhead A={A} E={E} K={C.QHEAD_ENV_K}")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("B", C.SELECT_BS)
@pytest.mark.parametrize("A,T", C.SELECT_SHAPES)
def test_fp32_restatement_of_select_action_stays_inside_the_bound(A, T, B, transposed):
    for mode in range(4):
        _, _, q, aux = C.select_inputs(A, T, B, mode, transposed, 3000 + mode)
        v, vs = action_values64(q, mode, aux)
        tol = C.values_tol(mode, T, 0, np.abs(q.astype(np.float64)), vs)
        tie = C.tie_pair(A)
        tied = (v[:, tie[0]] == v.max(1)) & (v[:, tie[0]] == v[:, tie[1]])
        assert tied[0]
        degenerate = mode == 2 and T == 1           # the expectation over a single atom is that atom, whatever the logit: every action ties
        if not degenerate:
            C.check_spread(v, tied, A, f"select mode {mode} A={A} T={T} B={B}")
        v32 = C.action_values32(q, mode, aux)
        if mode == 0:
            assert np.array_equal(v32.astype(np.float64), v)
            a, qm = C.first_max(v32)
            assert greedy_check(v, tol, a, qm, "mode 0", exclude=tied, tie=tie, allow_empty=B == 1) <= C.MAX_UNDECIDED
        else:
            # inputs without roundings of their own: the bound is the eight to ten roundings of the reduction itself and leaves no fixed factor to spare
            _judge(v32, v, tol, tie, tied, f"select mode {mode} A={A} T={T} B={B}", spare=1.0, degenerate=degenerate)


@pytest.mark.parametrize("E", C.MEAN_ROWS_ES)
def test_fp32_restatement_of_mean_rows_stays_inside_the_bound(E):
    x = recipe.gen(4000 + E).standard_normal((3, E)).astype(np.float32)
    n = (E + 255) // 256 * 256
    part = np.zeros((3, n), np.float32)
    part[:, :E] = x
    part = part.reshape(3, -1, 256)
    red = np.zeros((3, 256), np.float32)
    for k in range(part.shape[1]):
        red = (red + part[:, k]).astype(np.float32)
    o = 128
    while o:
        red[:, :o] = (red[:, :o] + red[:, o:2 * o]).astype(np.float32)
        o >>= 1
    got = (red[:, 0] / np.float32(E)).astype(np.float64)
    x64 = x.astype(np.float64)
    assert (np.abs(got - x64.mean(1)) * SPARE <= C.mean_rows_tol(E, np.abs(x64).mean(1))).all()


def _rejected(values, r, tol, what):
    err = np.abs(np.asarray(values, np.float64) - r["values"])
    assert (err > tol).any(), f"negative control {what}: the bound does not reject it (worst {float((err / tol).max()):.3f} of it)"


def test_the_bound_rejects_wrong_computations():
    # one slab left out; the dueling mean divided by A + 1 — at every dueling case; a mean over T divided by 64 ceil(T / 64) — at every mode-1 case
    # whose T is no multiple of 64
    for kt, cases in ((0, C.DIST_CASES), (1, C.QUANTILE_CASES)):
        for case in cases:
            A, T, dueling, mode, ld, nslab, E = case[:7]
            r = C.tail_reference(case, kt)
            if nslab > 1:
                q, _ = head_from_slabs64(r["slabs"][:-1], r["bias"], A, T, dueling, kt)
                _rejected(action_values64(q, mode, r["aux"])[0], r, r["tol"], f"{C.case_id(case)} without the last slab")
                q, _ = head_from_slabs64(r["slabs"][1:], r["bias"], A, T, dueling, kt)
                _rejected(action_values64(q, mode, r["aux"])[0], r, r["tol"], f"{C.case_id(case)} without the first slab")
            if dueling:
                raw, _ = head_from_slabs64(r["slabs"], r["bias"], A + 1, T, False, kt)          # the A + 1 raw streams, no combine
                q = raw[:, A:A + 1] + (raw[:, :A] - raw[:, :A].sum(1, keepdims=True) / (A + 1))
                _rejected(action_values64(q, mode, r["aux"])[0], r, r["tol"], f"{C.case_id(case)} dueling mean over A + 1")
            if mode == 1 and T % 64:
                _rejected(r["values"] * T / (64.0 * C.trips(T)), r, r["tol"], f"{C.case_id(case)} mean over the padded wave")
            # the last of two tied actions instead of the first
            a, qm = C.first_max(r["values"])
            greedy_check(r["values"], r["tol"], a, qm, tie=r["tie"])
            a[0] = r["tie"][1]
            with pytest.raises(AssertionError, match="the later one was chosen"):
                greedy_check(r["values"], r["tol"], a, qm, tie=r["tie"])
    # fc1 computed on single bf16 terms of both operands; one slab of fc1 left out (a k range of 32 of 544)
    for A, dueling in C.QHEAD_HEADS:
        E = 9
        r = C.qhead_reference(E, C.QHEAD_K, A, dueling)
        tol = C.qhead_tol(17, A, dueling, r["vscale"])
        if A > 2:               # two identical actions under the combine leave the value stream alone: one head row, whose bf16 error reaches 0.75 of the bound here
            lost, _ = qhead64(round_bf16(torch.from_numpy(r["feat"])).numpy(), round_bf16(torch.from_numpy(r["W1"])).numpy(), r["b1"], r["W2"], r["b2"], A, dueling)
            _rejected(lost, r, tol, f"qhead A={A}: fc1 on single bf16 terms")
        cut, _ = qhead64(r["feat"][:, 32:], r["W1"][:, 32:], r["b1"], r["W2"], r["b2"], A, dueling)
        _rejected(cut, r, tol, f"qhead A={A}: fc1 without its first slab")
        a, qm = C.first_max(r["values"])
        a[0] = r["tie"][1]
        with pytest.raises(AssertionError, match="the later one was chosen"):
            greedy_check(r["values"], tol, a, qm, tie=r["tie"])


def test_greedy_check_judges_decided_and_undecided_envs():
    v = np.array([[1.0, 2.0, 0.0], [1.0, 1.0 + 1e-9, 0.0], [3.0, 0.0, 3.0]])
    tol = np.full_like(v, 1e-6)
    assert greedy_check(v, tol, [1, 0, 0], [2.0, 1.0, 3.0], tie=(0, 2)) == pytest.approx(2 / 3)
    assert greedy_check(v, tol, [1, 1, 0], [2.0, 1.0, 3.0], exclude=[False, False, True]) == pytest.approx(1 / 2)
    with pytest.raises(AssertionError):
        greedy_check(v, tol, [0, 0, 0], [1.0, 1.0, 3.0])                      # a decided env with another action
    with pytest.raises(AssertionError):
        greedy_check(v, tol, [1, 2, 0], [2.0, 0.0, 3.0])                      # an undecided env with a non-candidate
    with pytest.raises(AssertionError):
        greedy_check(v, tol, [1, 0, 0], [2.0, 1.0 + 1e-5, 3.0])               # max-Q outside the bound
    with pytest.raises(AssertionError):
        greedy_check(v, tol, [1, 0, 2], [2.0, 1.0, 3.0], tie=(0, 2))          # the later of two equal actions


def test_the_draw_offsets_take_both_branches():
    for E, A in sorted({(c[6], c[0]) for c in C.DIST_CASES + C.QUANTILE_CASES} | {(E, A) for E in C.QHEAD_ES for A, _ in C.QHEAD_HEADS}):
        seen = set()
        for lone_greedy in (False, True):
            off_a, off_u = C.draw_offsets(E, A, lone_greedy)
            _, keep = C.egreedy_expected(C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, C.EPS, A, np.zeros(E, np.int64))
            seen |= set(keep.tolist())
            assert E == 1 or seen == {False, True}
        assert seen == {False, True}
