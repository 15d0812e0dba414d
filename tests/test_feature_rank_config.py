"""CPU: the host side of ``learner.rank_freq`` / ``learner.rank_delta`` — the config keys, the value helper and its refusals, the numpy restatement
tests/feature_rank_ref.py checked against a singular value decomposition on the input set the GPU tests use, the declarations in the binding table, the library's
argument checks (made in front of any launch), and the statistic's column, which appears only with the setting on.  The GPU side is tests/test_gpu_feature_rank.py."""
import csv
import ctypes as C
import inspect
import logging
import math
import types

import numpy as np
import pytest
import torch

import feature_rank_ref as FR


# ----------------------------------------------------------------------------------------------------------- settings
def test_config_keys_parse_and_round_trip():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    lc = parse_overrides([]).learner
    assert lc.rank_freq == 0 and isinstance(lc.rank_freq, int) and lc.rank_delta == 0.01 and isinstance(lc.rank_delta, float)
    cfg = parse_overrides(["learner.rank_freq=1000", "learner.rank_delta=0.1"])
    assert cfg.learner.rank_freq == 1000 and cfg.learner.rank_delta == 0.1
    for bad in ("learner.rank_freq=often", "learner.rank_delta=small"):
        with pytest.raises(Exception):
            parse_overrides([bad])
    d = to_dict(cfg)
    assert d["learner"]["rank_freq"] == 1000 and d["learner"]["rank_delta"] == 0.1
    back = from_dict(d)
    assert (back.learner.rank_freq, back.learner.rank_delta) == (1000, 0.1) and to_dict(back) == d
    old = from_dict({"learner": {"algo": "dqn"}}).learner
    assert (old.rank_freq, old.rank_delta) == (0, 0.01), "a dictionary written before the keys existed"
    from agent0.deepq import config as alias
    assert alias.LearnerConfig().rank_freq == 0 and alias.parse_overrides(["learner.rank_freq=7"]).learner.rank_freq == 7
    doc = " ".join(config.__doc__.split())
    for words in ("learner.rank_freq", "learner.rank_delta", "Kumar et al. 2021", "feature_rank", "512 * 2^-52", "verified on one rank only", "feature_spectrum"):
        assert words in doc, words


@pytest.mark.parametrize("args,want", [((0,), (0, 0.01)), ((None, None), (0, 0.01)), ((3, 0.1), (3, 0.1)), ((5.0, 0.5), (5, 0.5)), ((1, 0.999999), (1, 0.999999)),
                                       ((2, 1e-300), (2, 1e-300))])
def test_the_value_helper(args, want):
    from agent0_amd.deepq import engine
    got = engine.rank_value(*args)
    assert got == want and isinstance(got[0], int) and isinstance(got[1], float)
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["rank_freq"].default == 0 and p["rank_delta"].default == 0.01


@pytest.mark.parametrize("freq", [-1, -1000, 2.5, True])
def test_a_bad_period_is_refused_by_name(freq):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.rank_freq"):
        engine.rank_value(freq, 0.01)


@pytest.mark.parametrize("delta", [0.0, -0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("freq", [0, 3])
def test_a_bad_delta_is_refused_with_the_number_named(freq, delta):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.rank_delta") as e:
        engine.rank_value(freq, delta)
    assert repr(delta) in str(e.value)


def test_delta_is_inert_without_the_period_and_data_parallel_is_allowed(monkeypatch):
    """rank_delta alone switches nothing on; and unlike learner.redo_freq the setting is not refused under the data-parallel path: it writes nothing."""
    from agent0_amd.deepq import engine
    assert engine.rank_value(0, 0.3) == (0, 0.3) and engine.rank_value(None, 0.3)[0] == 0
    monkeypatch.setenv("A0_DP_FORCE", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert engine.rank_value(3, 0.01) == (3, 0.01)
    # off: the launch site issues nothing and touches no buffer
    eng = types.SimpleNamespace(rank_freq=0)
    assert engine.DeviceLearner._feature_rank(eng) is None and engine.DeviceLearner.feature_spectrum(eng) is None


def test_the_emulation_backend_is_refused_by_name():
    """DeviceLearner asks its backend for feature_rank; the CPU emulation (tests/cpu_ops.py) has none, and builds the learner without the setting as before."""
    import cpu_ops
    import recipe
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    ops = cpu_ops.CpuOps()
    assert not hasattr(ops, "feature_rank")
    L = NetLayout.from_spec(recipe.NetSpec("dqn", 4))
    with pytest.raises(ValueError, match=r"learner\.rank_freq=3: needs a backend with feature_rank"):
        DeviceLearner(ops, L, 4, rank_freq=3)
    dev = DeviceLearner(ops, L, 4, rank_freq=0, rank_delta=0.2)
    assert dev.rank_freq == 0 and dev.rank_gram is None and dev.rank_spectrum is None and dev.rank_result is None and dev.feature_spectrum() is None


# ----------------------------------------------------------------------------------------------------------- the restatement
def test_the_restatement_on_hand_made_spectra():
    s = np.zeros(512)
    assert FR.srank(s, 0.01) == 0 and FR.margin(s, 0.01) == np.inf and FR.ratio_error_bound(s, FR.EIG_TOL) == 0.0
    s[:4] = [4.0, 3.0, 2.0, 1.0]
    assert FR.srank(s, 0.5) == 2 and FR.srank(s, 0.31) == 2 and FR.srank(s, 0.29) == 3 and FR.srank(s, 0.01) == 4
    assert FR.margin(s, 0.25) == pytest.approx(0.05)
    assert FR.srank(np.ones(512), 0.01) == 507, "the identity"
    lam = np.array([1.0, FR.FLOOR * 1.0001, FR.FLOOR, FR.FLOOR / 2, 0.0, -1e-20] + [0.0] * 506)
    sig = FR.floor_of(lam)
    assert sig[0] == 1.0 and sig[1] > 0 and not sig[2:].any(), "at or under the floor: 0"
    # two equal eigenvalues moved by t: the share 1/2 moves by t / 4 to first order
    lam = np.array([1.0, 1.0] + [0.0] * 510)
    assert FR.ratio_error_bound(lam, 1e-6) == pytest.approx(1e-6 / 4, rel=1e-9)
    g = np.random.default_rng(5)
    X = g.standard_normal((40, 512)).astype(np.float32)
    G = FR.gram(X)
    assert G.dtype == np.float64 and np.array_equal(G, G.T) and np.allclose(G, X.astype(np.float64).T @ X.astype(np.float64), rtol=1e-13, atol=1e-12)
    assert (np.abs(G) <= FR.abs_gram(X) * (1 + 1e-15)).all()


@pytest.mark.parametrize("case", [c for c in FR.CASES if c[0] != "inf-row"], ids=FR.case_id)
def test_the_gram_route_agrees_with_the_svd_on_the_input_set(case):
    """srank through gram + eigvalsh equals srank through the singular values of X, and no cumulative share lies within twice the first-order error bound of 1 -
    delta — the condition the GPU test asserts again before it compares."""
    X = FR.make(case)
    G, lam, sigma = FR.reference(case)
    sv = np.zeros(512)
    s = np.linalg.svd(X.astype(np.float64), compute_uv=False)
    sv[:min(s.size, 512)] = s[:512]
    sv[sv * sv <= FR.FLOOR * sv[0] * sv[0]] = 0.0
    bound = FR.ratio_error_bound(lam, FR.EIG_TOL)
    diff = np.abs(np.sort(sv * sv)[::-1] - np.where(sigma > 0, lam, 0.0)).max() / (FR.EIG_TOL * lam[0]) if lam[0] > 0 else 0.0
    for delta in FR.DELTAS:
        m = FR.margin(sigma, delta)
        print(f"{FR.case_id(case)} delta={delta}: srank {FR.srank(sigma, delta)}, margin {m:.3e}, required {2 * bound:.3e}, routes differ by {diff:.4f} of the tolerance")
        assert m > 2 * bound
        assert FR.srank(sigma, delta) == FR.srank(sv, delta)
    assert int((sigma > 0).sum()) == int((sv > 0).sum())
    if case[0] == "zeros":
        assert FR.srank(sigma, 0.01) == 0
    if case[0] == "one-element":
        assert FR.srank(sigma, 0.01) == 1 and sigma[0] == 3.0
    if case[0] == "identity":
        assert FR.srank(sigma, 0.01) == 507
    if case[0] == "graded":
        assert int((sigma > 0).sum()) == 172, "2^(-i/4) above 2^-43"


# ----------------------------------------------------------------------------------------------------------- the binding table and the library's checks
def test_declarations():
    from agent0_amd import _abi, ops
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_feature_rank"] == ("int", ["ptr", "long long", "double", "ptr", "int", "int", "ptr", "ptr", "ptr", "ptr"])
    assert protos["a0_learner_set_feature_rank"] == ("int", ["ptr", "int", "double"]) and protos["a0_learner_feature_rank_buffers"] == ("int", ["ptr"] * 3)
    assert len(protos["a0_redo_score"][1]) == 17 and protos["a0_learner_set_redo"] == ("int", ["ptr", "int", "double", "int", "unsigned long long"]), "existing exports are what they were"
    lib = _abi.load()
    assert lib.a0_abi_version() == 1
    assert lib.a0_learner_set_feature_rank.argtypes == [C.c_void_p, C.c_int, C.c_double]
    assert ops.HipOps.RANK_FEATURES == 512 and ops.HipOps.RANK_GRAM_DOUBLES == 2 * 512 * 512
    header = open(_abi.HEADER).read()
    assert "#define A0_RANK_GRAM_DOUBLES (2 * A0_RANK_FEATURES * A0_RANK_FEATURES)" in header and "#define A0_RANK_FEATURES 512" in header
    assert hasattr(ops.HipOps, "feature_rank") and hasattr(ops.NativeLearner, "set_feature_rank") and hasattr(ops.NativeLearner, "feature_rank_buffers")


def test_arguments_are_checked_before_any_launch():
    """Every refusal returns A0_EINVAL with a message that names the argument, before a pointer is used (the pointers here are never dereferenced on the device)."""
    from agent0_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    q = [p + 1024 * i for i in range(8)]

    def rank(**kw):
        a = dict(fc1=q[0], rows=1, delta=0.01, state=q[1], freq=3, force=1, gram=q[2], spectrum=q[3], result=q[4])
        a.update(kw)
        return lib.a0_feature_rank(a["fc1"], a["rows"], a["delta"], a["state"], a["freq"], a["force"], a["gram"], a["spectrum"], a["result"], None)

    for bad, word in ((dict(fc1=None), "fc1"), (dict(gram=None), "gram"), (dict(spectrum=None), "spectrum"), (dict(result=None), "result"), (dict(state=None, force=0), "state"),
                      (dict(rows=0), "rows"), (dict(rows=-3), "rows"), (dict(freq=-1), "freq"), (dict(fc1=q[0] + 4), "fc1"), (dict(gram=q[2] + 4), "gram"),
                      (dict(spectrum=q[3] + 4), "spectrum"), (dict(result=q[4] + 2), "result"), (dict(state=q[1] + 1), "state")):
        assert rank(**bad) == -1, bad
        err = _abi.last_error()
        assert err.startswith("a0_feature_rank: ") and word in err, (bad, err)
    for delta, shown in ((0.0, "0"), (1.0, "1"), (-0.25, "-0.25"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf")):
        assert rank(delta=delta) == -1
        err = _abi.last_error()
        assert "delta" in err and f"= {shown}" in err and "(0, 1)" in err, (delta, err)
    assert lib.a0_learner_set_feature_rank(None, 3, 0.01) == -1 and "a0_learner_set_feature_rank" in _abi.last_error()
    assert lib.a0_learner_feature_rank_buffers(None, None, None) == -1 and "a0_learner_feature_rank_buffers" in _abi.last_error()


# ----------------------------------------------------------------------------------------------------------- the statistic
TODAYS_HEADER = ["frames", "fraction_loss", "loss", "return_train", "return_train_max", "qmax", "fps"]
REDO_KEYS = ["dormant_frac", "dormant_frac_conv1", "dormant_frac_conv2", "dormant_frac_conv3", "dormant_frac_fc1"]


def _stub_trainer(tmp_path, tag, **eng):
    from agent0_amd.deepq.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    e = dict(gnorm_ring=None, net_reset_freq=0, wd_partials=None, redo_freq=0, redo_counts=None, rank_freq=0, rank_result=None,
             state=torch.tensor([0, 6, 0, 0, 0, 0, 6, 0], dtype=torch.int32))
    e.update(eng)
    tr.learner = types.SimpleNamespace(engine=types.SimpleNamespace(**e))
    tr.cfg = types.SimpleNamespace(logdir=str(tmp_path / tag))
    (tmp_path / tag).mkdir()
    tr.frame_count, tr.Ls, tr.FLs, tr.Rs, tr.Qs, tr.GNs, tr.PN, tr._nl = 64, [0.5], [], [1.0], [2.0], [], None, False
    tr.primary, tr.writer, tr._wandb = True, None, None
    tr.logger = logging.getLogger(f"rank-test-{tag}")
    tr.logger.setLevel(logging.INFO)
    tr.logger.addHandler(logging.FileHandler(tmp_path / tag / "msg.log"))
    return tr


def _logged(tr, tmp_path, tag):
    res = dict(tr._result(), fps=100.0)
    tr.logging(res)
    for h in tr.logger.handlers:
        h.flush()
    with open(tmp_path / tag / "progress.csv") as f:
        rows = list(csv.reader(f))
    return res, rows, open(tmp_path / tag / "msg.log").read()


def test_the_statistic_appears_only_with_the_setting_on(tmp_path):
    res, rows, log = _logged(_stub_trainer(tmp_path, "off"), tmp_path, "off")
    assert list(res) == TODAYS_HEADER and rows[0] == TODAYS_HEADER and "feature_rank" not in log

    result = torch.tensor([0, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int32)
    tr = _stub_trainer(tmp_path, "on", rank_freq=3, rank_result=result)
    res, rows, log = _logged(tr, tmp_path, "on")
    assert list(res) == TODAYS_HEADER[:-1] + ["feature_rank", "fps"] and math.isnan(res["feature_rank"]), "NaN until the first evaluation"
    assert rows[0] == TODAYS_HEADER + ["feature_rank"]
    result.copy_(torch.tensor([187, 498, 6, 0, 0, 0, 0, 0], dtype=torch.int32))
    res, rows, log = _logged(tr, tmp_path, "on")
    assert res["feature_rank"] == 187.0 and len(rows) == 3 and float(rows[2][-1]) == 187.0 and "feature_rank: 187 | " in log
    result.copy_(torch.tensor([-1, 0, 9, 0, 0, 0, 0, 0], dtype=torch.int32))
    res, rows, log = _logged(tr, tmp_path, "on")
    assert math.isnan(res["feature_rank"]), "an activation that was not finite: reported as NaN"
    result.copy_(torch.tensor([0, 0, 12, 0, 0, 0, 0, 0], dtype=torch.int32))
    assert _logged(tr, tmp_path, "on")[0]["feature_rank"] == 0.0, "all activations zero: rank 0 is a value"

    # behind the other optional columns
    counts = torch.tensor([2, 16, 0, 128, 146, 6, 0, 0], dtype=torch.int32)
    tr = _stub_trainer(tmp_path, "all", rank_freq=3, rank_result=result, redo_freq=3, redo_counts=counts, net_reset_freq=3, wd_partials=torch.zeros(1), gnorm_ring=torch.zeros(1))
    res, rows, log = _logged(tr, tmp_path, "all")
    assert rows[0] == TODAYS_HEADER + ["grad_norm", "net_resets", "param_norm"] + REDO_KEYS + ["feature_rank"]
