"""GPU (MI355X): the actor's action-selection kernels against float64 at the edges of their work splits.

Kernels: the distributional tails (actor_dist_tail: a0_actor_dist_tail_kernel, four envs per workgroup, 256-column trips; actor_dist_tail_env_step /
_env_step_enc: a0_actor_dist_tail_wave0 with its 16-byte and scalar slab sums), the quantile tails (actor_quantile_tail / _env_step / _env_step_enc: the same
wave with the (env, quantile) row layout), the scalar head (actor_qhead_n / actor_qhead / actor_qhead_env_step / _env_step_enc: a0_qhead_wave's 8-, 4- and
1-slab trips), select_action on both layouts its callers use, and mean_rows.  Cases, inputs and bounds: tests/actor_tail_cases.py; references:
tests/util.py; both checked on the CPU by tests/test_actor_tail_reference_helpers.py, where an fp32 restatement of the kernels' arithmetic uses at most a
quarter of the bound and five wrong computations are rejected by it.

The bound.  An fp32 addition, multiplication, division or fused multiply-add moves its result by at most 2^-24 of the magnitude it works at, and every
magnitude on the way to an element is at most that element's SCALE, the same computation on absolute values.  So an element is held to
c 2^-24 scale, c the number of roundings on its longest path, counted from the source:
  head output       nslab + 1      slab sum in slab order (the first addition to zero included) and the bias
  dueling combine   A + 3          A - 1 additions, the division by A, the subtraction and the addition (one spare)
  mode 1 (mean)     ceil(T/64) + 7 the lane's strided sum, six butterfly stages, the division by T
  mode 3 (fqf)      ceil(T/64) + 8 the fraction's width, its product with q, the strided sum, the butterfly
  mode 2 (c51)      a logit error delta moves sum_t p_t z_t by at most 2 delta sum_t p_t |z_t|; delta = (c_head + 2) 2^-24 max_t scale_t (the head's roundings and
                    the subtraction of the maximum on |q| + |max|); on top, relative to sum_t p_t |z_t|: twice expf's relative error (numerator and
                    denominator) and 2 ceil(T/64) + 14 roundings (product, two strided sums, two butterflies, the division)
  scalar head       fc1 is a split-operand GEMM: 2e-6 of its accumulated magnitude (the bound of tests/test_gpu_gemm.py and tests/test_gpu_conv_reference.py,
                    measured worst 5e-7), then nslab + 1 for a0_qhead_wave's slab sum and bias; the head row: 8 fused multiply-adds per lane, six
                    butterfly stages, the bias (15); the combine (A + 3); all on fc1's magnitude carried through |W2| (util.qhead64)
  mean_rows         ceil(E/256) + 9  the thread's strided sum, eight tree levels, the division
expf's relative error is not documented for this device: test_expf_error_stays_within_the_recorded_figure measures it through select_action (mode 2 on the
logits (0, a), atoms (0, 1): exp(a) / (1 + exp(a)), two roundings on top of expf, none for a < -17) on 1e5 arguments in [-40, 0]; the bound takes twice
the recorded worst (actor_tail_cases.EXPF_MEASURED = 9.1e-8, measured 9.07e-8 below -17 and 1.71e-7 with the two roundings above it;
profiles/r11_actor_tail_accuracy.md) and the test keeps the record honest.

An env is DECIDED when one action alone lies within the two bounds of the float64 maximum; there the device's greedy action must be the float64 argmax,
elsewhere one of the candidates; max-Q must be the value of the action chosen, within its bound (util.greedy_check).  Every case plants one exact tie — two
actions bit-identical in every input, not adjacent where the action set allows, lifted to the best of env 0 — where the lower index must win; envs whose best
is that pair are left out of the undecided share, which must stay within 2 %.  action is prefilled with -1, max-Q with NaN, both followed by 64 sentinels
(the surplus waves of the four-env workgroups).  Epsilon-greedy: the oracle's Philox draws at offset + e, by value and through the control block."""
import numpy as np
import pytest
import torch

import actor_tail_cases as C
import recipe
from util import action_values64, greedy_check, record_stats

pytestmark = pytest.mark.gpu

GUARD = 64
SENT_F, SENT_I = -1.25e38, 0x5A5A5A5A


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


_NET = {}


def _enc(hip):
    """Encoder weights for the merged steps that go on to encode the next observation."""
    if not _NET:
        from agent0_amd.deepq.engine import DeviceNet
        from agent0_amd.deepq.layout import NetLayout
        spec = recipe.NetSpec("dqn", 4, obs_shape=(4, 84, 84))
        net = DeviceNet(hip, NetLayout.from_spec(spec), hip.net(4, 84, 84))
        net.load_state_dict(recipe.make_state_dict(spec, 11))
        _NET["net"] = net
    return _NET["net"]


def _dev(hip, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)


def _outputs(hip, n, m=None):
    """action [n] = -1 and max-Q [m or n] = NaN, each followed by GUARD sentinels."""
    m = n if m is None else m
    act = hip.empty(n + GUARD, dtype=torch.int32)
    act[:n].fill_(-1)
    act[n:].fill_(SENT_I)
    q = hip.empty(m + GUARD)
    q[:m].fill_(float("nan"))
    q[m:].fill_(SENT_F)
    return act, q


def _collect(act, q, n, what, m=None):
    m = n if m is None else m
    torch.cuda.synchronize()
    assert bool((act[n:] == SENT_I).all()) and bool((q[m:] == SENT_F).all()), f"{what}: write past the end"
    a, v = act[:n].cpu().numpy(), q[:m].cpu().numpy()
    assert np.isfinite(v).all(), f"{what}: max-Q unwritten or not finite"
    return a, v


def _throwaway_env(hip, E):
    """The synthetic env's arguments of a merged step whose env work nobody reads (test_actor_step_encoder_against_float64's)."""
    z = lambda n, dt=torch.float32: hip.zeros(n, dtype=dt)
    obs_in = _dev(hip, recipe.gen(77).integers(0, 256, E * 4 * 84 * 84, dtype=np.uint8))
    return (4321, 0, 1, obs_in, z(E * 4 * 84 * 84, torch.uint8), z(E), z(E), z(E), 1, 0, 0.99, z(E, torch.int32), z(E), z(E), obs_in,
            z(E * 8 * 84 * 84, torch.uint8), E, 0, z(E, torch.int32), z(E), z(E))


def _ctrl(hip, da, du):
    ctrl = hip.zeros(8, dtype=torch.int64)
    ctrl[2], ctrl[3] = da, du                       # A0_CTRL_RNG_ACTION, A0_CTRL_RNG_UNIFORM
    return ctrl


def _judge_forms(hip, forms, values, tol_of, tie, tied, E, A, what):
    """``forms``: name -> launch(eps, off_a, off_u, ctrl, eps_ptr, action, qmax).  Every form's greedy pass (eps = -1: u > eps always) against float64, its
    epsilon-greedy passes (by value; through the control block) against the oracle's draws, and all forms bit-equal in action and max-Q."""
    stats, first = {}, None
    eps_ptr = _dev(hip, np.array([C.EPS], np.float32))
    offs = [C.draw_offsets(E, A, False), C.draw_offsets(E, A, True)]
    seen = set()
    for name, launch in forms.items():
        tol = tol_of(name)
        act, q = _outputs(hip, E)
        launch(-1.0, 0, 0, None, None, act, q)
        a_g, q_g = _collect(act, q, E, f"{what} {name} greedy")
        share = greedy_check(values, tol, a_g, q_g, f"{what} {name}", exclude=tied, tie=tie, allow_empty=E == 1 or A == 2)
        assert share <= C.MAX_UNDECIDED, f"{what} {name}: {share:.1%} of the envs undecided"
        assert (a_g[tied] == values.argmax(1)[tied]).all(), f"{what} {name}: the first of the equal maxima must win: {a_g[tied]}"
        rows = np.arange(E)
        stats[name] = {"worst_over_bound": float((np.abs(q_g.astype(np.float64) - values[rows, a_g]) / tol[rows, a_g]).max()), "undecided": share}
        print(f"{what} {name}: {stats[name]}")
        runs = [(a_g, q_g)]
        for (off_a, off_u), through_ctrl in zip(offs, (False, True)):
            want, keep = C.egreedy_expected(C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, C.EPS, A, a_g)
            seen |= set(keep.tolist())
            act, q = _outputs(hip, E)
            if through_ctrl:
                launch(0.9, off_a - 8, off_u - 20, _ctrl(hip, 8, 20), eps_ptr, act, q)
            else:
                launch(C.EPS, off_a, off_u, None, None, act, q)
            a_e, q_e = _collect(act, q, E, f"{what} {name} eps")
            assert np.array_equal(a_e, want), f"{what} {name} (ctrl={through_ctrl}): {a_e} vs the oracle's draws {want}"
            assert np.array_equal(q_e.view(np.int32), q_g.view(np.int32)), f"{what} {name}: max-Q is the greedy value whatever is drawn"
            runs.append((a_e, q_e))
        if first is None:
            first = (name, runs)
        else:
            for (a0, q0), (a1, q1) in zip(first[1], runs):
                assert np.array_equal(a0, a1) and np.array_equal(q0.view(np.int32), q1.view(np.int32)), f"{what}: {name} differs from {first[0]}"
    assert seen == {False, True}, "the oracle's draws take both branches"
    return stats


# ------------------------------------------------------------------------------------------------ expf
def test_expf_error_stays_within_the_recorded_figure(hip):
    B = 100000
    g = recipe.gen(9)
    a = np.concatenate((-40.0 * g.random(B - 2), [-40.0, 0.0])).astype(np.float32)
    x = np.stack((np.zeros(B, np.float32), a), 1)
    qsel = hip.empty(B)
    hip.select_action(_dev(hip, x.reshape(-1)), 2, 2, 1, B, 1, 2, 2, _dev(hip, np.array([0.0, 1.0], np.float32)), None, qsel, None)
    torch.cuda.synchronize()
    got = qsel.cpu().numpy().astype(np.float64)
    e = np.exp(a.astype(np.float64))
    rel = np.abs(got - e / (1.0 + e)) / (e / (1.0 + e))
    alone = a < -17.0                                   # 1 + exp(a) rounds to 1: the quotient is expf(a) itself
    fig = {"worst": float(rel.max()), "worst_expf_alone": float(rel[alone].max()), "at": float(a[rel.argmax()]), "n": B, "recorded": C.EXPF_MEASURED}
    print("expf:", fig)
    record_stats("actor_tail_expf", fig)
    assert fig["worst_expf_alone"] <= C.EXPF_MEASURED and fig["worst"] <= C.EXPF_MEASURED + 2 * C.U, fig


# ------------------------------------------------------------------------------------------------ distributional and quantile tails
def _tail_case(hip, case, kt):
    A, T, dueling, mode, ld, nslab, E, offset = case
    r = C.tail_reference(case, kt)
    buf = hip.empty(r["slabs"].size + 4)
    assert buf.data_ptr() % 16 == 0
    slabs = buf[offset:offset + r["slabs"].size]
    slabs.copy_(_dev(hip, r["slabs"].reshape(-1)))
    assert slabs.data_ptr() % 16 == 4 * offset
    bias = _dev(hip, r["bias"])
    aux = None if r["aux"] is None else _dev(hip, r["aux"].reshape(-1))
    env = _throwaway_env(hip, E)
    net = _enc(hip)
    enc = dict(task=0, wt=net.wt, enc_w=net.encoder_weights(), act3_next=hip.empty(E * 3136))
    fn = (("actor_dist_tail", "actor_dist_tail_env_step", "actor_dist_tail_env_step_enc"),
          ("actor_quantile_tail", "actor_quantile_tail_env_step", "actor_quantile_tail_env_step_enc"))[kt]

    def form(k):
        f = getattr(hip, fn[k])

        def launch(eps, off_a, off_u, ctrl, eps_ptr, act, q):
            args = (slabs, nslab, bias, ld, A, T, dueling, mode, aux, E, C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
            if k == 0:
                f(*args)
            elif k == 1:
                f(*args, *env)
            else:
                f(*args, *env, **enc)
        return launch

    what = ("dist ", "quantile ")[kt] + C.case_id(case)
    stats = _judge_forms(hip, {fn[k]: form(k) for k in range(3)}, r["values"], lambda name: r["tol"], r["tie"], r["tied"], E, A, what)
    record_stats("actor_tail_" + ("dist_", "quantile_")[kt] + C.case_id(case), stats)


@pytest.mark.parametrize("case", C.DIST_CASES, ids=C.case_id)
def test_distributional_tails_against_float64(hip, case):
    _tail_case(hip, case, 0)


@pytest.mark.parametrize("case", C.QUANTILE_CASES, ids=C.case_id)
def test_quantile_tails_against_float64(hip, case):
    _tail_case(hip, case, 1)


# ------------------------------------------------------------------------------------------------ scalar head
def _qhead_dev(hip, r):
    return tuple(_dev(hip, r[k].reshape(-1)) for k in ("feat", "W1", "b1", "W2", "b2"))


@pytest.mark.parametrize("E", C.QHEAD_ES)
@pytest.mark.parametrize("A,dueling", C.QHEAD_HEADS)
def test_scalar_head_against_float64_at_every_slab_trip_combination(hip, A, dueling, E):
    """actor_qhead_n at K = 544 with 1 ... 17 splits (every combination of a0_qhead_wave's 8-, 4- and 1-slab trips), and actor_qhead at its own split count,
    bit-equal to actor_qhead_n with that count."""
    K = C.QHEAD_K
    r = C.qhead_reference(E, K, A, dueling)
    feat, W1, b1, W2, b2 = _qhead_dev(hip, r)
    own = C.fc1_splits(E, K)
    assert hip.actor_qhead_scratch(E, K) == own * E * 512 and own in C.QHEAD_SPLITS
    forms, ns_of = {}, {}
    for ns in C.QHEAD_SPLITS:
        def launch(eps, off_a, off_u, ctrl, eps_ptr, act, q, ns=ns):
            hip.actor_qhead_n(feat, E, K, ns, W1, b1, W2, b2, A, dueling, hip.empty(ns * E * 512), C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
        forms[f"actor_qhead_n[{ns}]"], ns_of[f"actor_qhead_n[{ns}]"] = launch, ns
    stats = {}
    for name, launch in forms.items():          # one form at a time: different split counts are different sums, not bit-equal
        stats.update(_judge_forms(hip, {name: launch}, r["values"], lambda n: C.qhead_tol(ns_of[n], A, dueling, r["vscale"]), r["tie"], r["tied"], E, A,
                                  f"qhead A={A} duel={dueling} E={E}"))

    def launch_own(eps, off_a, off_u, ctrl, eps_ptr, act, q):
        hip.actor_qhead(feat, E, K, W1, b1, W2, b2, A, dueling, hip.empty(own * E * 512), C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
    stats.update(_judge_forms(hip, {f"actor_qhead_n[{own}]": forms[f"actor_qhead_n[{own}]"], "actor_qhead": launch_own}, r["values"],
                              lambda n: C.qhead_tol(own, A, dueling, r["vscale"]), r["tie"], r["tied"], E, A, f"qhead A={A} duel={dueling} E={E}"))
    record_stats(f"actor_tail_qhead_A{A}_{'duel' if dueling else 'plain'}_E{E}", stats)


@pytest.mark.parametrize("A,dueling,E", C.QHEAD_ENV_CASES)
def test_merged_scalar_head_steps_against_float64(hip, A, dueling, E):
    """actor_qhead, actor_qhead_env_step and actor_qhead_env_step_enc at K = 3136 and the split count they choose: the same slabs, the same bytes."""
    K = C.QHEAD_ENV_K
    r = C.qhead_reference(E, K, A, dueling)
    feat, W1, b1, W2, b2 = _qhead_dev(hip, r)
    ns = C.fc1_splits(E, K)
    need = hip.actor_qhead_scratch(E, K)
    assert need == ns * E * 512
    env = _throwaway_env(hip, E)
    net = _enc(hip)
    enc = dict(task=0, wt=net.wt, enc_w=net.encoder_weights(), act3_next=hip.empty(E * K))

    def form(k):
        def launch(eps, off_a, off_u, ctrl, eps_ptr, act, q):
            args = (feat, E, K, W1, b1, W2, b2, A, dueling, hip.empty(need), C.RNG_SEED, C.STREAM_A, C.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
            if k == 0:
                hip.actor_qhead(*args)
            elif k == 1:
                hip.actor_qhead_env_step(*args, *env)
            else:
                hip.actor_qhead_env_step_enc(*args, *env, **enc)
        return launch

    names = ("actor_qhead", "actor_qhead_env_step", "actor_qhead_env_step_enc")
    stats = _judge_forms(hip, {n: form(k) for k, n in enumerate(names)}, r["values"], lambda n: C.qhead_tol(ns, A, dueling, r["vscale"]), r["tie"], r["tied"], E, A,
                         f"qhead K={K} A={A} duel={dueling} E={E}")
    record_stats(f"actor_tail_qhead_env_A{A}_{'duel' if dueling else 'plain'}_E{E}", stats)


# ------------------------------------------------------------------------------------------------ select_action, mean_rows
@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("B", C.SELECT_BS)
@pytest.mark.parametrize("A,T", C.SELECT_SHAPES)
def test_select_action_against_float64_on_both_layouts(hip, A, T, B, transposed):
    stats = {}
    for mode in range(4):
        x, (sb, sa, st), q, aux = C.select_inputs(A, T, B, mode, transposed, 3000 + mode)
        v, vs = action_values64(q, mode, aux)
        tol = C.values_tol(mode, T, 0, np.abs(q.astype(np.float64)), vs)
        tie = C.tie_pair(A)
        tied = (v[:, tie[0]] == v.max(1)) & (v[:, tie[0]] == v[:, tie[1]])
        assert tied[0]
        degenerate = mode == 2 and T == 1           # the expectation over a single atom is that atom, whatever the logit: every action ties
        if not degenerate:
            C.check_spread(v, tied, A, f"select mode {mode} A={A} T={T} B={B}")
        a_star, qmax = _outputs(hip, B)
        _, qsel = _outputs(hip, 1, B * A)
        hip.select_action(_dev(hip, x), sb, sa, st, B, A, T, mode, None if aux is None else _dev(hip, aux.reshape(-1)), a_star, qsel, qmax)
        what = f"select mode {mode} A={A} T={T} B={B} {'transposed' if transposed else 'contiguous'}"
        a, qm = _collect(a_star, qmax, B, what)
        _, qs = _collect(a_star, qsel, B, what, B * A)
        err = np.abs(qs.astype(np.float64).reshape(B, A) - v)
        assert (err <= tol).all(), f"{what}: qsel off by {float((err / np.maximum(tol, 1e-300)).max()):.3f} of the bound"
        share = greedy_check(v, tol, a, qm, what, exclude=tied, tie=tie, allow_empty=B == 1 or degenerate)
        assert share <= C.MAX_UNDECIDED, f"{what}: {share:.1%} undecided"
        assert (a[tied] == v.argmax(1)[tied]).all(), f"{what}: the first of the equal maxima must win"
        assert np.array_equal(qm.view(np.int32), qs.reshape(B, A)[np.arange(B), a].view(np.int32)), f"{what}: qmax is qsel at a_star"
        stats[f"mode{mode}"] = {"worst_over_bound": float((err[tol > 0] / tol[tol > 0]).max()) if mode else float(err.max()), "undecided": share}
    print(stats)
    record_stats(f"actor_tail_select_A{A}_T{T}_B{B}_{'transposed' if transposed else 'contiguous'}", stats)


@pytest.mark.parametrize("E", C.MEAN_ROWS_ES)
def test_mean_rows_against_float64(hip, E):
    T = 3
    x = recipe.gen(4000 + E).standard_normal((T, E)).astype(np.float32)
    _, out = _outputs(hip, 1, T)
    hip.mean_rows(_dev(hip, x.reshape(-1)), T, E, out)
    torch.cuda.synchronize()
    assert bool((out[T:] == SENT_F).all())
    got = out[:T].cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    tol = C.mean_rows_tol(E, np.abs(x64).mean(1))
    err = np.abs(got - x64.mean(1))
    record_stats(f"actor_tail_mean_rows_E{E}", {"worst_over_bound": float((err / tol).max())})
    assert (err <= tol).all(), f"E={E}: {float((err / tol).max()):.3f} of the bound"
