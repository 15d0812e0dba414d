"""GPU (MI355X): the feature rank (``learner.rank_freq`` / ``learner.rank_delta``): a0_feature_rank and everything that issues it, against the numpy restatement
tests/feature_rank_ref.py on the input set that file defines (tests/test_feature_rank_config.py shows on the CPU that the set keeps every cumulative share away
from 1 - delta and that the Gram route agrees with a singular value decomposition on it).

1. the Gram launch against a Gram matrix accumulated in extended precision: every element within rows * 2^-53 * sum_r |x_ri x_rj| (the bound of a double summation
   in any order; the products are exact), and bitwise symmetric.   2. the eigenvalue stage against numpy on the DEVICE's Gram matrix read back: sigma^2 within
   512 * 2^-53 * lambda_1 (half the floor), the same number of singular values above the floor.   3. the rank for delta = 0.01 and 0.1, after the margin condition.
4. the self-deciding gate with guard bands.   5. determinism and the argument checks.   6. DeviceLearner and the a0_learner handle beside a twin without the
setting.   7. the Trainer on both loops, a snapshot between two evaluations, the data-parallel path on one rank, every setting at once.

Work split of the kernels (csrc/feature_rank.hip): a workgroup owns a 64 x 64 tile of G and stages 16 rows per step, an MFMA consumes 4 — the row counts 1, 3, 4, 5
(the MFMA's k edge), 63, 511, 512, 513 (the 16-row step's edge; fewer rows than columns: hundreds of eigenvalues at the floor) and 2051 (128 steps and a tail)."""
import math

import numpy as np
import pytest
import torch

import feature_rank_ref as FR

pytestmark = pytest.mark.gpu

GUARD = 16
NN = 512 * 512


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "feature_rank")
    return ops


class _Out:
    """gram, spectrum and result, each between two guard bands of a value the kernels never write."""

    def __init__(self, hip):
        dev = hip.device
        self.gb = torch.full((2 * NN + 2 * GUARD,), -7.25, dtype=torch.float64, device=dev)
        self.sb = torch.full((512 + 2 * GUARD,), -7.25, dtype=torch.float64, device=dev)
        self.rb = torch.full((8 + 2 * GUARD,), -5, dtype=torch.int32, device=dev)
        self.gram, self.spectrum, self.result = self.gb[GUARD:GUARD + 2 * NN], self.sb[GUARD:GUARD + 512], self.rb[GUARD:GUARD + 8]
        self.result[2] = -1

    def guards_intact(self):
        return all(bool((b[:GUARD] == v).all()) and bool((b[-GUARD:] == v).all()) for b, v in ((self.gb, -7.25), (self.sb, -7.25), (self.rb, -5)))

    def untouched(self):
        return self.guards_intact() and bool((self.gram == -7.25).all()) and bool((self.spectrum == -7.25).all()) and self.result.tolist() == [-5, -5, -1, -5, -5, -5, -5, -5]


_DEV = {}


def _device(hip, case):
    """The device's evaluation of a case with ``force``, once per delta: (G, {delta: (sigma, result)}); cached and shared by the tests below."""
    if case not in _DEV:
        X = FR.make(case)
        x = torch.from_numpy(X).to(hip.device).reshape(-1)
        per, G = {}, None
        for delta in FR.DELTAS:
            o = _Out(hip)
            hip.feature_rank(x, X.shape[0], delta, None, 0, True, o.gram, o.spectrum, o.result)
            torch.cuda.synchronize()
            assert o.guards_intact()
            g = o.gram[:NN].cpu().numpy().reshape(512, 512)
            assert G is None or np.array_equal(g.view(np.int64), G.view(np.int64)), "the Gram matrix does not depend on delta"
            G = g
            per[delta] = (o.spectrum.cpu().numpy(), o.result.tolist())
        _DEV[case] = (G, per)
    return _DEV[case]


FINITE = [c for c in FR.CASES if c[0] != "inf-row"]


# ------------------------------------------------------------------------------------------------ 1. the Gram launch
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_gram_against_extended_precision(hip, case):
    X = FR.make(case)
    G, _ = _device(hip, case)
    assert np.array_equal(G.view(np.int64), G.T.view(np.int64)), "bitwise symmetric"
    if case[0] == "inf-row":
        assert np.isinf(np.diag(G)).all()
        return
    ref = FR.reference(case)[0]
    bound = X.shape[0] * 2.0 ** -53 * FR.abs_gram(X)
    err = np.abs(G - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"RECORD gram {FR.case_id(case)}: worst error over its bound {worst:.4f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 2. the spectrum
@pytest.mark.parametrize("case", FINITE, ids=FR.case_id)
def test_spectrum_against_numpy_on_the_devices_gram(hip, case):
    G, per = _device(hip, case)
    lam = FR.eigenvalues(G)
    want = FR.floor_of(lam)
    tol = FR.EIG_TOL * lam[0]
    for delta in FR.DELTAS:
        sigma, result = per[delta]
        assert np.array_equal(sigma.view(np.int64), per[FR.DELTAS[0]][0].view(np.int64)), "the spectrum does not depend on delta"
        assert (sigma >= 0).all() and (np.diff(sigma) <= 0).all(), "descending"
        err = np.abs(sigma * sigma - want * want).max()
        print(f"RECORD eig {FR.case_id(case)}: worst eigenvalue error over 512 * 2^-53 * lambda_1: {err / tol if tol > 0 else 0.0:.4f}; above the floor {result[1]}")
        assert err <= tol
        assert result[1] == int((want > 0).sum()) == int((sigma > 0).sum())
        assert result[2] == 0 and result[3:] == [-5] * 5, "a NULL state counts as update 0; the spare words are not written"


# ------------------------------------------------------------------------------------------------ 3. the rank
@pytest.mark.parametrize("delta", FR.DELTAS)
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_rank_equals_the_restatement(hip, case, delta):
    G, per = _device(hip, case)
    sigma, result = per[delta]
    if case[0] == "inf-row":
        assert result[:3] == [-1, 0, 0] and not sigma.any(), "a diagonal element that is not finite"
        return
    lam = FR.eigenvalues(G)
    want = FR.floor_of(lam)
    need, have = 2 * FR.ratio_error_bound(lam, FR.EIG_TOL), FR.margin(want, delta)
    print(f"RECORD margin {FR.case_id(case)} delta={delta}: srank {FR.srank(want, delta)}, margin {have:.3e} over the required {need:.3e}: {have / need if need > 0 else math.inf:.3g}")
    assert have > need, "the case keeps every cumulative share away from 1 - delta"
    assert result[0] == FR.srank(want, delta)
    fixed = {"zeros": {0.01: 0, 0.1: 0}, "one-element": {0.01: 1, 0.1: 1}, "identity": {0.01: 507, 0.1: 461}}
    if case[0] in fixed:
        assert result[0] == fixed[case[0]][delta]


# ------------------------------------------------------------------------------------------------ 4. the gate
@pytest.mark.parametrize("state,freq", [([0, 4, 0, 0, 0, 0, 4, 0], 3), ([0, 3, 1, 1, 0, 0, 3, 0], 3), ([0, 0, 0, 0, 0, 0, 0, 0], 3), ([0, 3, 0, 0, 0, 0, 3, 0], 0)],
                         ids=["freq-mismatch", "nan-skipped", "no-update-yet", "freq-zero"])
def test_the_launches_decide_for_themselves(hip, state, freq):
    X = FR.make(("mix", 63, 7, 0.01))
    x = torch.from_numpy(X).to(hip.device).reshape(-1)
    o = _Out(hip)
    st = torch.tensor(state, dtype=torch.int32, device=hip.device)
    hip.feature_rank(x, 63, 0.01, st, freq, False, o.gram, o.spectrum, o.result)
    torch.cuda.synchronize()
    assert o.untouched() and st.tolist() == state


def test_the_launches_fire_on_a_multiple_of_the_period(hip):
    case = ("mix", 63, 7, 0.01)
    x = torch.from_numpy(FR.make(case)).to(hip.device).reshape(-1)
    o = _Out(hip)
    state = [0, 6, 0, 0, 0, 0, 6, 0]
    st = torch.tensor(state, dtype=torch.int32, device=hip.device)
    hip.feature_rank(x, 63, 0.01, st, 3, False, o.gram, o.spectrum, o.result)
    torch.cuda.synchronize()
    G, per = _device(hip, case)
    sigma, result = per[0.01]
    assert o.guards_intact() and st.tolist() == state
    assert np.array_equal(o.gram[:NN].cpu().numpy().view(np.int64), G.reshape(-1).view(np.int64)) and np.array_equal(o.spectrum.cpu().numpy().view(np.int64), sigma.view(np.int64))
    assert o.result.tolist() == result[:2] + [6] + [-5] * 5, "result[2] is the evaluation's update count"


# ------------------------------------------------------------------------------------------------ 5. determinism, arguments
@pytest.mark.parametrize("case", [("mix", 513, 64, 0.05), ("mix", 5, 1, 0.0), ("graded", 0, 0, 0.0)], ids=FR.case_id)
def test_two_runs_give_the_same_bytes(hip, case):
    X = FR.make(case)
    x = torch.from_numpy(X).to(hip.device).reshape(-1)
    runs = []
    for _ in range(2):
        o = _Out(hip)
        hip.feature_rank(x, X.shape[0], 0.01, None, 0, True, o.gram, o.spectrum, o.result)
        torch.cuda.synchronize()
        runs.append((o.gram.view(torch.int64).clone(), o.spectrum.view(torch.int64).clone(), o.result.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    G, per = _device(hip, case)
    assert np.array_equal(runs[0][0][:NN].cpu().numpy(), G.reshape(-1).view(np.int64))


def test_argument_checks(hip):
    from agent0_amd._abi import A0Error
    x = hip.zeros(4 * 512 + 4)
    o = _Out(hip)
    st = hip.zeros(8, dtype=torch.int32)
    good = dict(fc1=x[:4 * 512], rows=4, delta=0.01, state=st, freq=3, force=True, gram=o.gram, spectrum=o.spectrum, result=o.result)

    def call(**kw):
        a = dict(good, **kw)
        hip.feature_rank(a["fc1"], a["rows"], a["delta"], a["state"], a["freq"], a["force"], a["gram"], a["spectrum"], a["result"])

    for bad, word in ((dict(rows=0), "rows < 1"), (dict(rows=-2), "rows < 1"), (dict(freq=-1), "freq < 0"), (dict(fc1=x[1:4 * 512 + 1]), "fc1 must be 16-byte aligned"),
                      (dict(delta=0.0), "delta = 0 "), (dict(delta=1.0), "delta = 1 "), (dict(delta=float("nan")), "delta = nan"), (dict(delta=-0.5), "delta = -0.5")):
        with pytest.raises(A0Error, match="a0_feature_rank") as e:
            call(**bad)
        assert word in str(e.value), (bad, str(e.value))
    torch.cuda.synchronize()
    assert o.untouched(), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 6. learners
B = 8
FAR = 10 ** 6
N_RANK = 3


def _rd():
    import test_gpu_redo as RDT
    return RDT


def _peek_fc1(nat):
    import ctypes as C
    ptr, cnt = C.c_void_p(), C.c_longlong()
    assert nat.lib.a0_learner_peek(nat.h, 4, C.addressof(ptr), C.addressof(cnt)) == 0
    view = type("_Peek", (), {"__cuda_array_interface__": {"shape": (int(cnt.value),), "typestr": "<f4", "data": (int(ptr.value), False), "version": 3}})()
    return torch.as_tensor(view, device="cuda").cpu().numpy().reshape(-1, 512)


def _restated(X, delta):
    """(srank, sigma, above the floor) of activations through the restatement, after the margin condition."""
    G = FR.gram(X)
    lam = FR.eigenvalues(G)
    sigma = FR.floor_of(lam)
    assert FR.margin(sigma, delta) > 2 * FR.ratio_error_bound(lam, FR.EIG_TOL), "the activations keep every cumulative share away from 1 - delta"
    return FR.srank(sigma, delta), sigma, int((sigma > 0).sum())


def _check_evaluation(X, delta, spectrum, result, steps):
    want, sigma, pos = _restated(X, delta)
    got = spectrum.cpu().numpy()
    assert np.abs(got * got - sigma * sigma).max() <= 2 * FR.EIG_TOL * sigma[0] ** 2, "the device's Gram matrix and eigenvalues against numpy's: twice the eigenvalue tolerance"
    assert result.tolist()[:3] == [want, pos, steps]
    return want


def test_learner_table_is_the_redo_tests():
    assert list(_rd().LEARNERS) == ["dqn", "c51-duel", "iqn", "fqf-fraction-clip"] and _rd().B == B


@pytest.mark.parametrize("name", ["dqn", "c51-duel", "iqn", "fqf-fraction-clip"])
def test_learner_evaluates_at_the_right_updates_and_moves_nothing(hip, name):
    """rank_freq = 3 beside a twin without the setting and the a0_learner handle.  Evaluations after updates 3 and 6 and not between; the update in front of which the
    NaN flag is raised leaves the count at 3 and does not evaluate; after 2 N + 1 = 7 counted updates the whole learner state is the twin's, byte for byte."""
    RDT = _rd()
    T = RDT._tt()
    cs = RDT._case(hip, name)
    L, delta = cs.L, 0.1
    auto, twin = RDT._engine(cs, rank_freq=N_RANK, rank_delta=delta), RDT._engine(cs)
    nat = T._handle(cs, auto, FAR)
    nat.set_feature_rank(N_RANK, delta)
    assert twin.rank_result is None and twin.rank_gram is None and twin.feature_spectrum() is None and auto.rank_result.tolist() == [0, 0, -1, 0, 0, 0, 0, 0]
    assert auto.feature_spectrum() is None, "None before the first evaluation"
    sp, rs = nat.feature_rank_buffers()
    assert rs.tolist() == [0, 0, -1, 0, 0, 0, 0, 0] and sp.dtype == torch.float64 and sp.numel() == 512
    rows = B * (cs.N if L.algo == "iqn" else L.F) if L.quantile else B

    def handle_equals(dev, what):
        o, t, m, v, st = nat.get()
        T._same(dict(online=o, target=t, moment1=m, moment2=v), {k: T._all_of(dev)[k] for k in ("online", "target", "moment1", "moment2")}, what)

    def step(s, nan=False, handle=True):
        for dev in (auto, twin):
            if nan:
                dev.state[0] = 1
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        if handle:
            nat.update(*cs.batch(s))
        torch.cuda.synchronize()
        T._same(T._all_of(auto), T._all_of(twin), f"{name}: call {s + 1}")

    ranks = {}
    for s in range(2):
        step(s)
        assert auto.rank_result.tolist()[2] == -1 and nat.feature_rank_buffers()[1].tolist()[2] == -1, "no evaluation yet"
    step(2)
    X = auto.ws_o.h.cpu().numpy().reshape(-1, 512)
    assert X.shape[0] == rows and np.array_equal(X, _peek_fc1(nat)) and np.array_equal(X, twin.ws_o.h.cpu().numpy().reshape(-1, 512)), "iqn / fqf: the B * N rows of the differentiated pass"
    ranks[3] = _check_evaluation(X, delta, auto.rank_spectrum, auto.rank_result, 3)
    sp, rs = nat.feature_rank_buffers()
    assert torch.equal(sp.view(torch.int64), auto.rank_spectrum.view(torch.int64)) and torch.equal(rs, auto.rank_result), "the handle: the same evaluation"
    assert np.array_equal(auto.feature_spectrum(), auto.rank_spectrum.cpu().numpy())
    handle_equals(auto, f"{name}: handle, update 3")
    # a NaN-skipped call: the count stays at 3, a multiple of the period, and nothing is evaluated.  The engines only — a handle's flag is not the caller's to raise —
    # so from here on the handle is a run of its own (the skipped call consumed the engines' quantile draws) and is checked against its own activations.
    auto.rank_result[0] = -77
    step(3, nan=True, handle=False)
    assert auto.state.tolist()[1] == 3 and auto.state.tolist()[3] == 1 and auto.rank_result.tolist()[0] == -77
    for s in (4, 5):
        step(s)
        assert auto.rank_result.tolist()[0] == -77 and auto.rank_result.tolist()[2] == 3 and nat.feature_rank_buffers()[1].tolist()[2] == 3, "not between"
    step(6)
    assert auto.state.tolist()[1] == 6
    X = auto.ws_o.h.cpu().numpy().reshape(-1, 512)
    ranks[6] = _check_evaluation(X, delta, auto.rank_spectrum, auto.rank_result, 6)
    sp, rs = nat.feature_rank_buffers()
    _check_evaluation(_peek_fc1(nat), delta, sp, rs, 6)
    step(7)
    assert auto.state.tolist()[1] == 7 == 2 * N_RANK + 1 and auto.rank_result.tolist()[2] == 6 and nat.feature_rank_buffers()[1].tolist()[2] == 6
    if "frac" in L.blocks:
        assert torch.equal(auto.rms_sq, twin.rms_sq)
    print(f"{name}: {rows} rows, srank_{delta} after updates 3 and 6: {ranks}")
    with pytest.raises(Exception, match="has run an update"):
        nat.set_feature_rank(5, delta)
    nat.close()


def test_handle_refusals(hip):
    RDT = _rd()
    T = RDT._tt()
    cs = RDT._case(hip, "dqn")
    nat = T._handle(cs, RDT._engine(cs), FAR)
    with pytest.raises(Exception, match="freq < 0"):
        nat.set_feature_rank(-1, 0.01)
    for delta, shown in ((0.0, "delta = 0 "), (1.0, "delta = 1 "), (float("nan"), "delta = nan")):
        with pytest.raises(Exception, match="a0_learner_set_feature_rank") as e:
            nat.set_feature_rank(3, delta)
        assert shown in str(e.value)
    nat.set_feature_rank(0, 0.5)
    assert nat.feature_rank_buffers() is None, "off: nothing allocated"
    nat.close()


def test_freq_zero_is_the_learner_without_the_argument(hip, monkeypatch):
    RDT = _rd()
    T = RDT._tt()
    cs = RDT._case(hip, "dqn")
    from collections import Counter

    class Counting:
        def __init__(self, lib):
            self._lib, self.seen = lib, Counter()

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("a0_"):
                return fn

            def call(*a, **k):
                self.seen[name] += 1
                return fn(*a, **k)
            return call

    off, none, on = RDT._engine(cs, rank_freq=0, rank_delta=0.5), T._engine(cs, FAR), RDT._engine(cs, rank_freq=2)
    assert off.rank_gram is None and off.rank_spectrum is None and off.rank_result is None
    counting = Counting(hip.lib)
    monkeypatch.setattr(hip, "lib", counting)
    seen = {}
    for s in range(3):
        for tag, dev in (("off", off), ("none", none), ("on", on)):
            counting.seen = Counter()
            dev.update(*cs.batch(s), rand=cs.draws(dev))
            seen[tag] = counting.seen
        assert seen["off"] == seen["none"] and sum(seen["off"].values()) > 5 and not any("feature_rank" in k for k in seen["off"]), f"update {s + 1}: {seen}"
        assert seen["on"] - seen["off"] == Counter({"a0_feature_rank": 1}), "on: one call more, nothing else"
    torch.cuda.synchronize()
    T._same(T._all_of(off), T._all_of(none), "off")
    T._same(T._all_of(on), T._all_of(none), "on")
    import gc
    del on
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = RDT._engine(cs, rank_freq=0)
    used_off = torch.cuda.memory_allocated() - mem
    del more
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = T._engine(cs, FAR)
    assert torch.cuda.memory_allocated() - mem == used_off, "no extra allocation"


# ------------------------------------------------------------------------------------------------ 7. the Trainer
ON = ["learner.rank_freq=3", "learner.rank_delta=0.1"]


def _nr():
    import test_gpu_net_reset as NR
    return NR


def _without_rank(results):
    return [{k: v for k, v in r.items() if k != "feature_rank"} for r in results]


def _assert_same_run(a, b):
    _rd()._assert_same_run(a, b)


@pytest.mark.parametrize("native", [False, True], ids=["python-classes", "handles"])
def test_the_statistic_is_the_restatements(native, tmp_path, monkeypatch):
    """rank_freq = 3 = learner_steps: every evaluation falls on an iteration's last update, whose activations are still there when the iteration returns.  The result,
    progress.csv and msg.log carry the column; feature_spectrum() returns the evaluation's singular values on both hosts."""
    import csv
    NR = _nr()
    tr = NR._trainer(tmp_path, monkeypatch, native, "dqn", ON, False, "run", freq=0)
    seen = 0
    for i in range(4):
        res = tr.run_iteration()
        tr.logging(res)
        assert list(res)[-2:] == ["feature_rank", "fps"]
        eng = tr.learner.engine
        steps = eng.state[1].item()
        if steps == 0:
            assert math.isnan(res["feature_rank"]) and eng.feature_spectrum() is None, "NaN until the first evaluation"
            continue
        assert steps % 3 == 0
        torch.cuda.synchronize()
        if native:
            import ctypes as C
            ptr, cnt = C.c_void_p(), C.c_longlong()
            assert tr._nl.lib.a0_learner_peek(tr._nl.learner, 4, C.addressof(ptr), C.addressof(cnt)) == 0
            view = type("_Peek", (), {"__cuda_array_interface__": {"shape": (int(cnt.value),), "typestr": "<f4", "data": (int(ptr.value), False), "version": 3}})()
            X = torch.as_tensor(view, device="cuda").cpu().numpy().reshape(-1, 512)
        else:
            X = eng.ws_o.h.cpu().numpy().reshape(-1, 512)
        assert X.shape[0] == eng.B
        want, sigma, pos = _restated(X, 0.1)
        assert res["feature_rank"] == float(want), f"iteration {i}"
        got = eng.feature_spectrum()
        assert got.shape == (512,) and np.abs(got * got - sigma * sigma).max() <= 2 * FR.EIG_TOL * sigma[0] ** 2 and int((got > 0).sum()) == pos
        seen += 1
    assert seen >= 2 and (tr._nl is not False) == native
    NR._el()._close(tr)
    with open(tmp_path / "run" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0][-1] == "feature_rank" and len(rows) == 5 and float(rows[-1][-1]) == res["feature_rank"]
    assert "feature_rank: " in open(tmp_path / "run" / "msg.log").read()


def test_handles_python_classes_and_the_plain_run_end_on_the_same_state(tmp_path, monkeypatch):
    """Six iterations of three updates once training has started; the Python classes run their first updates eagerly and the rest from a hipGraph, which holds the two
    launches like every other of the update.  The setting writes nothing the run uses: the state and every other statistic are the plain run's."""
    NR = _nr()
    a = NR._run(tmp_path, monkeypatch, False, "dqn", ON, False, "py", freq=0)
    b = NR._run(tmp_path, monkeypatch, True, "dqn", ON, False, "nat", freq=0)
    _assert_same_run(a, b)
    assert a[0][4][1].item() >= 6 and a[1][-1]["feature_rank"] >= 1
    for native, tag in ((True, "plain-nat"), (False, "plain-py")):
        plain = NR._run(tmp_path, monkeypatch, native, "dqn", [], False, tag, freq=0)
        assert not any("feature_rank" in r for r in plain[1])
        _assert_same_run((a[0], _without_rank(a[1])) + a[2:], plain)
    zero = NR._run(tmp_path, monkeypatch, True, "dqn", ["learner.rank_freq=0", "learner.rank_delta=0.3"], False, "zero", freq=0)
    _assert_same_run(zero, plain)
    assert [list(r) for r in zero[1]] == [list(r) for r in plain[1]], "freq = 0: the same keys"


@pytest.mark.parametrize("save_native,load_native", [(True, True), (False, True)], ids=["handles", "python-to-handles"])
def test_a_snapshot_between_two_evaluations_resumes_with_nan(save_native, load_native, tmp_path, monkeypatch):
    NR = _nr()
    on = ["learner.rank_freq=4", "learner.rank_delta=0.1"]          # period 4 against three updates per iteration: the snapshot falls between two evaluations
    want = NR._run(tmp_path, monkeypatch, load_native, "dqn", on, False, "a", freq=0)
    tr = NR._trainer(tmp_path, monkeypatch, save_native, "dqn", on, False, "b", freq=0)
    for _ in range(4):
        last = tr.run_iteration()
    at = tr.learner.engine.state[1].item()
    assert at >= 4 and at % 4 != 0 and not math.isnan(last["feature_rank"]), "behind an evaluation, in front of the next"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    NR._el()._close(tr)
    tr = NR._trainer(tmp_path, monkeypatch, load_native, "dqn", on, False, "c", freq=0, seed=7)
    tr.load_snapshot(snap_dir)
    assert math.isnan(tr._result()["feature_rank"]), "nothing of the evaluation is in a snapshot"
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = NR._state(tr)
    assert tr.learner.engine.state[1].item() // 4 > at // 4, "an evaluation happened after the snapshot"
    NR._el()._close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    _rd()._same_results(res[-1:], want[1][-1:])
    assert not math.isnan(res[-1]["feature_rank"])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_the_data_parallel_path_on_one_rank_gives_the_plain_runs_value(tmp_path, monkeypatch):
    """A one-rank RCCL group (A0_DP_FORCE=1): the setting is allowed, and the statistic is the plain run's (verified on one rank only)."""
    import torch.distributed as dist
    NR = _nr()
    plain = NR._run(tmp_path, monkeypatch, True, "dqn", ON, False, "plain", freq=0)
    NR._el()._one_rank_group(monkeypatch)
    try:
        a = NR._run(tmp_path, monkeypatch, False, "dqn", ON, False, "dp-py", freq=0, dp=True)
        b = NR._run(tmp_path, monkeypatch, True, "dqn", ON, False, "dp-nat", freq=0, dp=True)
    finally:
        dist.destroy_process_group()
    _assert_same_run(a, b)
    ranks = [r["feature_rank"] for r in plain[1]]
    for run in (a, b):
        got = [r["feature_rank"] for r in run[1]]
        assert all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(got, ranks)) and not math.isnan(got[-1]), (got, ranks)


def test_every_learner_setting_at_once(tmp_path, monkeypatch):
    """clip_grad_norm, target_tau, weight_decay, aug_shift, redo_freq = 3 and net_reset_freq = 6 beside rank_freq = 3: the feature-rank launches stand in front of the
    recycle and the reset, so they see the activations those leave alone; the run's state is the same run's without rank_freq."""
    NR = _nr()
    others = ["learner.redo_freq=3", "learner.redo_tau=0.5", "learner.clip_grad_norm=5.0", "learner.target_tau=0.25", "learner.weight_decay=0.01", "learner.aug_shift=4"]
    a = NR._run(tmp_path, monkeypatch, False, "dqn", ON + others, False, "py", freq=6)
    b = NR._run(tmp_path, monkeypatch, True, "dqn", ON + others, False, "nat", freq=6)
    _assert_same_run(a, b)
    state = a[0][4]
    assert state[1].item() >= 9 and state[7].item() == state[1].item() // 6 * 6 and a[1][-1]["net_resets"] >= 1 and not math.isnan(a[1][-1]["dormant_frac"])
    assert a[1][-1]["feature_rank"] >= 1 and list(a[1][-1])[-1] == "feature_rank"
    without = NR._run(tmp_path, monkeypatch, True, "dqn", others, False, "without", freq=6)
    _assert_same_run((a[0], _without_rank(a[1])) + a[2:], without)
