"""CPU: the host side of ``learner.iqn.munchausen`` — the config key, the validation function and its messages, the declarations in the binding table and the
library's argument checks (which need no device).  The GPU side is tests/test_gpu_miqn.py; the reference is held by tests/test_miqn_reference_helpers.py."""
import ctypes as C
import inspect
import math
import os

import pytest


def test_config_key_parses_and_round_trips():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.iqn.munchausen is False, "the default is off"
    assert (cfg.learner.mdqn.tau, cfg.learner.mdqn.alpha, cfg.learner.mdqn.lo) == (0.03, 0.9, -1)
    for raw, want in (("true", True), ("1", True), ("false", False), ("off", False)):
        assert parse_overrides([f"learner.iqn.munchausen={raw}"]).learner.iqn.munchausen is want
    with pytest.raises(Exception):
        parse_overrides(["learner.iqn.munchausen=maybe"])
    cfg = parse_overrides(["learner.algo=iqn", "learner.iqn.munchausen=true", "learner.mdqn.alpha=0.5", "learner.mdqn.tau=0.1", "learner.mdqn.lo=-2"])
    assert cfg.learner.iqn.munchausen is True and (cfg.learner.mdqn.alpha, cfg.learner.mdqn.tau, cfg.learner.mdqn.lo) == (0.5, 0.1, -2.0)
    d = to_dict(cfg)
    assert d["learner"]["iqn"]["munchausen"] is True
    back = from_dict(d)
    assert back.learner.iqn.munchausen is True and to_dict(back) == d
    assert from_dict({"learner": {"algo": "iqn", "iqn": {"K": 8}}}).learner.iqn.munchausen is False, "a dictionary written before the key existed"
    from agent0.deepq import config as alias
    assert alias.IQNConfig().munchausen is False and alias.parse_overrides(["learner.iqn.munchausen=true"]).learner.iqn.munchausen is True
    doc = config.__doc__
    assert "learner.iqn.munchausen" in doc and "learner.mdqn.alpha" in doc and "still unused by ``learner.algo=mdqn``" in doc and "Q17" in doc


def test_the_validation_function():
    from agent0_amd.deepq import engine
    assert engine.munchausen_value(False) == (False, 0.03, 0.9, -1.0)
    assert engine.munchausen_value(None) == (False, 0.03, 0.9, -1.0)
    assert engine.munchausen_value(True, pipeline_target=False) == (True, 0.03, 0.9, -1.0)
    assert engine.munchausen_value(True, 1, 0, 0, pipeline_target=False) == (True, 1.0, 0.0, 0.0), "alpha = 0 and lo = 0 are allowed: no bonus"
    assert engine.munchausen_value(False, algo="dqn", double_q=True, pipeline_target=True)[0] is False, "off is off whatever else is set"
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["munchausen"].default is False and p["mdqn_alpha"].default == 0.9


@pytest.mark.parametrize("key,kw", [("tau", dict(tau=0.0)), ("tau", dict(tau=-0.03)), ("tau", dict(tau=math.nan)), ("tau", dict(tau=math.inf)), ("tau", dict(tau=1e-60)),
                                    ("tau", dict(tau=1e60)), ("alpha", dict(alpha=-0.1)), ("alpha", dict(alpha=math.nan)), ("alpha", dict(alpha=math.inf)),
                                    ("lo", dict(lo=0.5)), ("lo", dict(lo=math.nan)), ("lo", dict(lo=-math.inf))])
@pytest.mark.parametrize("on", [True, False])
def test_bad_numbers_are_refused_with_the_setting_and_the_number_named(key, kw, on):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=rf"learner\.iqn\.munchausen.*learner\.mdqn\.{key}=") as e:
        engine.munchausen_value(on, pipeline_target=False, **kw)
    assert repr(list(kw.values())[0]) in str(e.value)


def test_other_settings_are_refused_by_name(monkeypatch):
    from agent0_amd.deepq import engine
    for algo in ("dqn", "c51", "qr", "fqf", "mdqn"):
        with pytest.raises(ValueError, match=rf"learner\.iqn\.munchausen.*learner\.algo={algo}"):
            engine.munchausen_value(True, algo=algo, pipeline_target=False)
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*learner\.double_q"):
        engine.munchausen_value(True, double_q=True, pipeline_target=False)
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*A0_PIPELINE_TARGET"):
        engine.munchausen_value(True, pipeline_target=True)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*A0_PIPELINE_TARGET"):
        engine.munchausen_value(True)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "0")
    assert engine.munchausen_value(True)[0] is True


def test_a_backend_without_the_kernel_is_refused():
    """The engine composes kernels through ``ops``; the host emulation has no miqn_target, and a missing kernel is an error, not a fall-back."""
    import cpu_ops
    import recipe
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    ops = cpu_ops.CpuOps()
    assert not hasattr(ops, "miqn_target")
    L = NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="iqn"))
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*miqn_target"):
        DeviceLearner(ops, L, 4, K=2, N=2, N_dash=2, munchausen=True)
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*learner\.algo=dqn"):
        DeviceLearner(ops, NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="dqn")), 4, munchausen=True)
    dev = DeviceLearner(ops, L, 4, K=2, N=2, N_dash=2)
    assert dev.munchausen is False and dev.ws_m is None, "off: no buffer"


def test_declarations():
    from agent0_amd import _abi, ops
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_miqn_target"] == ("int", ["ptr", "ptr", "long long", "long long", "long long", "ptr", "ptr", "ptr", "float", "float", "float", "float", "int", "int",
                                                "int", "ptr", "ptr"])
    assert protos["a0_learner_set_munchausen"] == ("int", ["ptr", "int", "double", "double", "double"])
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_learner_set_munchausen.argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double] and lib.a0_miqn_target.restype == C.c_int
    assert hasattr(ops.HipOps, "miqn_target") and hasattr(ops.NativeLearner, "set_munchausen")


def test_argument_checks_are_made_in_front_of_any_launch():
    """Every refusal returns A0_EINVAL under the entry point's name before a pointer is used (the pointers here are never dereferenced)."""
    from agent0_amd import _abi
    lib = _abi.load()
    fake, EINVAL = 1 << 20, -1
    ok = dict(q_next=fake, q_cur=fake, act=fake, rew=fake, done=fake, tau=0.03, alpha=0.9, lo=-1.0, B=2, Nd=8, A=4, y=fake)
    call = lambda **kw: (lambda a: lib.a0_miqn_target(a["q_next"], a["q_cur"], 32, 4, 1, a["act"], a["rew"], a["done"], 0.99, a["tau"], a["alpha"], a["lo"], a["B"], a["Nd"],
                                                      a["A"], a["y"], None))({**ok, **kw})
    bad = [dict(q_next=None), dict(q_cur=None), dict(act=None), dict(rew=None), dict(done=None), dict(y=None), dict(B=0), dict(Nd=0), dict(Nd=8193), dict(A=0), dict(A=33),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=math.nan), dict(tau=math.inf), dict(alpha=-0.5), dict(alpha=math.nan), dict(alpha=math.inf), dict(lo=0.25),
           dict(lo=math.nan), dict(lo=-math.inf)]
    for kw in bad:
        assert call(**kw) == EINVAL and _abi.last_error().startswith("a0_miqn_target"), kw
    assert lib.a0_learner_set_munchausen(None, 1, 0.03, 0.9, -1.0) == EINVAL and "a0_learner_set_munchausen" in _abi.last_error()
