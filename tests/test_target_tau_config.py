"""CPU: the host side of ``learner.target_tau`` — the config key, the value helper, the float64 reference against itself, and the two new exports in the binding
table (declared, exported, bound, their arguments checked in front of any launch).  The GPU side is tests/test_gpu_target_tau.py."""
import numpy as np
import pytest

import target_tau_ref as R


def test_config_key_parses_and_round_trips():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.target_tau == 0.0 and isinstance(cfg.learner.target_tau, float) and cfg.learner.target_update_freq == 500
    cfg = parse_overrides(["learner.target_tau=0.005", "learner.target_update_freq=1"])
    assert cfg.learner.target_tau == 0.005 and isinstance(cfg.learner.target_tau, float) and cfg.learner.target_update_freq == 1
    assert parse_overrides(["learner.target_tau=5e-3"]).learner.target_tau == 0.005
    with pytest.raises(Exception):
        parse_overrides(["learner.target_tau=slow"])
    d = to_dict(cfg)
    assert d["learner"]["target_tau"] == 0.005
    back = from_dict(d)
    assert back.learner.target_tau == 0.005 and to_dict(back) == d
    assert from_dict({"learner": {"algo": "dqn"}}).learner.target_tau == 0.0, "a dictionary written before the key existed"
    doc = config.__doc__
    assert "learner.target_tau" in doc and "target_update_freq=1 learner.target_tau=0.005" in doc and "hard copy" in doc


@pytest.mark.parametrize("value,want", [(0.0, 0.0), (-0.0, 0.0), (-1.0, 0.0), (-5, 0.0), (None, 0.0), (0.005, 0.005), (0.5, 0.5), (0.999, 0.999)])
def test_the_value_helper(value, want):
    import inspect
    from agent0_amd.deepq import engine
    got = engine.target_tau_value(value)
    assert isinstance(got, float) and got == want
    assert inspect.signature(engine.DeviceLearner.__init__).parameters["target_tau"].default == 0.0


@pytest.mark.parametrize("value", [1, 1.0, 1.5, 1e9, float("inf")])
def test_the_value_helper_refuses_the_hard_copy(value):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.target_tau"):
        engine.target_tau_value(value)


def test_reference_rounds_tau_once_and_keeps_fixed_points():
    # tau32 is the double rounded to fp32 once: 0.005 is not a float, and rounding through fp16 or twice would give another number
    assert R.tau32(0.005) == np.float32(0.005) and float(R.tau32(0.005)) != 0.005
    assert R.tau32(0.005).dtype == np.float32 and R.tau32(np.float64(0.999)) == np.float32(0.999)
    g = np.random.default_rng(3)
    t = g.standard_normal(4096).astype(np.float32)
    p = g.standard_normal(4096).astype(np.float32)
    for tau in (0.005, 0.5, 0.999):
        # fixed points: p == t gives t, exactly, whatever tau is
        assert np.array_equal(R.blend_nearest(t, t, tau), t) and np.array_equal(R.blend_f64(t, t, tau), t.astype(np.float64))
        # the reference uses tau32, not the double: with the double the float64 values differ
        a, x = R.blend_terms(t, p, tau)
        d = (p - t).astype(np.float64)
        assert np.array_equal(x, np.float64(np.float32(tau)) * d)
        if float(np.float32(tau)) != tau:
            assert not np.array_equal(x, tau * d)
        # the result lies between t and p (up to one rounding)
        out = R.blend_nearest(t, p, tau)
        assert bool(((out >= np.minimum(t, p)) & (out <= np.maximum(t, p))).all())
        assert int(R.double_rounding_suspects(t, p, tau).sum()) <= 2
    # a difference that underflows against t: one ulp apart, tau below a half -> t; above -> p
    q = np.nextafter(t, np.float32(np.inf)).astype(np.float32)
    assert np.array_equal(R.blend_nearest(t, q, 0.005), t) and np.array_equal(R.blend_nearest(t, q, 0.999), q)
    assert np.array_equal(R.ulp_distance(t, q), np.ones(t.size, np.int64)) and int(R.ulp_distance(np.float32(0.0), np.float32(-0.0))) == 0


def test_the_header_declares_and_the_binding_matches():
    from agent0_amd import _abi
    protos = {n: (r, t) for r, n, t in _abi.parse_header()}
    assert protos["a0_target_blend"] == ("int", ["ptr", "ptr", "long long", "double", "ptr", "int", "int", "ptr", "int", "ptr", "ptr"])
    assert protos["a0_learner_set_target_tau"] == ("int", ["ptr", "double"])
    # the existing exports are what they were
    assert protos["a0_target_sync"] == ("int", ["ptr", "ptr", "long long", "ptr", "int", "ptr"]) and len(protos["a0_adam_step_sync"][1]) == 16
    assert len(protos["a0_adam_step_sync_wt"][1]) == 24 and len(protos["a0_update_tail"][1]) == 22 and protos["a0_learner_set_grad_clip"] == ("int", ["ptr", "double", "ptr", "int"])
    assert "state[4] stays 0 while tau is on" in " ".join(open(_abi.HEADER).read().split()).replace("* ", "")
    lib = _abi.load()
    for name in ("a0_target_blend", "a0_learner_set_target_tau"):
        assert len(getattr(lib, name).argtypes) == len(protos[name][1]), name
    from agent0_amd.ops import HipOps, NativeLearner
    assert callable(HipOps.target_blend) and callable(NativeLearner.set_target_tau)


def test_arguments_are_checked_before_any_launch():
    """Validation happens in front of every HIP call, so it runs here."""
    import ctypes as C
    from agent0_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 80000)()
    p = (C.addressof(buf) + 15) // 16 * 16
    q = p + 4 * 40000
    ok_args = lambda **kw: dict(dict(target=p, online=q, n=64, tau=0.5, state=q, freq=1, force=1, w=None, C=0, wt=None), **kw)
    call = lambda a: lib.a0_target_blend(a["target"], a["online"], a["n"], a["tau"], a["state"], a["freq"], a["force"], a["w"], a["C"], a["wt"], None)
    for bad in (dict(target=None), dict(online=None), dict(n=0), dict(state=None, force=0), dict(target=p + 2)):
        assert call(ok_args(**bad)) == -1 and "a0_target_blend" in _abi.last_error(), bad
    for tau in (1.0, 1.5, 0.0, -0.5, float("nan"), 1.0 - 2.0 ** -30):      # the last one rounds to 1.0f
        assert call(ok_args(tau=tau)) == -1 and "tau" in _abi.last_error(), tau
    # weight copies: the target's encoder weights, C and an aligned buffer
    ew = _abi.EncoderWeights(p, p, p, p, p, p)
    assert call(ok_args(wt=q, w=None, C=4)) == -1 and call(ok_args(wt=q, w=C.addressof(ew), C=0)) == -1
    assert call(ok_args(wt=q + 4, w=C.addressof(ew), C=4, n=80000)) == -1 and "16-byte aligned" in _abi.last_error()
    assert call(ok_args(wt=q, w=C.addressof(ew), C=4, n=64)) == -1 and "inside target" in _abi.last_error()
    assert lib.a0_learner_set_target_tau(None, 0.5) == -1 and "a0_learner_set_target_tau" in _abi.last_error()
