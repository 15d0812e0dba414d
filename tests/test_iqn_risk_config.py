"""CPU: the host side of ``learner.iqn.risk`` — the two config keys, the validation function and its messages, the declarations in the binding table and the
library's argument checks (which need no device).  The GPU side is tests/test_gpu_iqn_risk.py; the reference is held by tests/test_iqn_risk_reference_helpers.py."""
import ctypes as C
import inspect
import math
import os

import pytest


def test_config_keys_parse_and_round_trip():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.iqn.risk == "neutral" and cfg.learner.iqn.risk_eta == 0.0, "the defaults"
    cfg = parse_overrides(["learner.algo=iqn", "learner.iqn.risk=cvar", "learner.iqn.risk_eta=0.25"])      # KeyError before the keys existed
    assert cfg.learner.iqn.risk == "cvar" and cfg.learner.iqn.risk_eta == 0.25
    assert parse_overrides(["learner.iqn.risk=WANG", "learner.iqn.risk_eta=-0.75"]).learner.iqn.risk_eta == -0.75
    with pytest.raises(ValueError):
        parse_overrides(["learner.iqn.risk_eta=much"])
    d = to_dict(cfg)
    assert d["learner"]["iqn"]["risk"] == "cvar" and d["learner"]["iqn"]["risk_eta"] == 0.25
    back = from_dict(d)
    assert back.learner.iqn.risk == "cvar" and to_dict(back) == d
    old = from_dict({"learner": {"algo": "iqn", "iqn": {"K": 8}}})
    assert old.learner.iqn.risk == "neutral" and old.learner.iqn.risk_eta == 0.0, "a dictionary written before the keys existed"
    from agent0.deepq import config as alias
    assert alias.IQNConfig().risk == "neutral" and alias.parse_overrides(["learner.iqn.risk=pow"]).learner.iqn.risk == "pow"
    doc = config.__doc__
    assert "learner.iqn.risk " in doc and "learner.iqn.risk_eta" in doc and "neutral | cvar | pow | cpw | wang" in doc and "Dabney" in doc


def test_the_validation_function():
    from agent0_amd.deepq import engine
    from agent0_amd.ops import RISK_KINDS
    assert RISK_KINDS == {"neutral": 0, "cvar": 1, "pow": 2, "cpw": 3, "wang": 4}
    assert engine.risk_value("neutral") == (0, 0.0) and engine.risk_value(None) == (0, 0.0)
    assert engine.risk_value("neutral", math.nan, algo="dqn", munchausen=True) == (0, 0.0), "neutral ignores eta and everything else"
    assert engine.risk_value("CVaR", 0.25) == (1, 0.25) and engine.risk_value(" cvar ", 1) == (1, 1.0)
    assert engine.risk_value("pow", -2) == (2, -2.0) and engine.risk_value("pow", 0.0) == (2, 0.0) and engine.risk_value("pow", 64) == (2, 64.0)
    assert engine.risk_value("cpw", 0.71) == (3, 0.71) and engine.risk_value("Wang", -0.75) == (4, -0.75) and engine.risk_value("wang", 8.0) == (4, 8.0)
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["risk"].default == "neutral" and p["risk_eta"].default == 0.0


@pytest.mark.parametrize("name", ["norm", "cvar2", "", "0.25"])
def test_an_unknown_name_is_refused(name):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=.*neutral \| cvar \| pow \| cpw \| wang") as e:
        engine.risk_value(name, 0.5)
    assert repr(name) in str(e.value)


@pytest.mark.parametrize("kind,eta", [("cvar", -0.1), ("cvar", 1.5), ("cvar", math.nan), ("cvar", math.inf), ("cvar", 1e-60), ("cpw", -0.71), ("cpw", 1.01),
                                      ("cpw", math.nan), ("pow", 64.5), ("pow", -65.0), ("pow", math.nan), ("pow", math.inf), ("wang", 8.5), ("wang", -9.0),
                                      ("wang", math.nan), ("wang", -math.inf)])
def test_a_bad_eta_is_refused_with_the_setting_and_the_number_named(kind, eta):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=rf"learner\.iqn\.risk={kind}: learner\.iqn\.risk_eta=.*the paper uses") as e:
        engine.risk_value(kind, eta)
    assert repr(eta) in str(e.value)


@pytest.mark.parametrize("kind,paper", [("cvar", "0.25"), ("cpw", "0.71")])
def test_the_default_eta_names_the_papers_value(kind, paper):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=rf"learner\.iqn\.risk={kind}: learner\.iqn\.risk_eta=0\.0 must be 0 < eta <= 1 \(the default 0 is not a {kind} parameter; the paper uses {paper}"):
        engine.risk_value(kind, 0.0)


def test_other_settings_are_refused_by_name():
    from agent0_amd.deepq import engine
    for algo in ("dqn", "c51", "qr", "fqf", "mdqn"):
        with pytest.raises(ValueError, match=rf"learner\.iqn\.risk=wang.*learner\.algo={algo}"):
            engine.risk_value("wang", 0.75, algo=algo)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cvar.*learner\.iqn\.munchausen"):
        engine.risk_value("cvar", 0.25, munchausen=True)


def test_a_staged_target_pass_needs_no_refusal(monkeypatch):
    """A0_PIPELINE_TARGET=1 is allowed: an iqn learner has no separately staged target pass, with or without the setting (and where one exists it ends at the fc1
    slabs, in front of every fraction)."""
    import cpu_ops
    import recipe
    from agent0_amd.deepq import engine
    from agent0_amd.deepq.layout import NetLayout
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    assert engine.risk_value("cvar", 0.25) == (1, 0.25)
    L = NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="iqn"))
    assert engine.DeviceLearner(cpu_ops.CpuOps(), L, 4, K=2, N=2, N_dash=2).target_stage_supported is False


def test_the_engine_refuses_through_its_constructor_and_its_setter():
    """The engine composes kernels through ``ops``; the host emulation has no risk_distort, and a missing kernel is an error, not a fall-back."""
    import cpu_ops
    import recipe
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    ops = cpu_ops.CpuOps()
    assert not hasattr(ops, "risk_distort")
    L = NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="iqn"))
    mk = lambda **kw: DeviceLearner(ops, L, 4, K=2, N=2, N_dash=2, **kw)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cvar.*risk_distort"):
        mk(risk="cvar", risk_eta=0.25)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cvar: learner\.iqn\.risk_eta=0\.0"):
        mk(risk="cvar")
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk='norm'"):
        mk(risk="norm")
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=pow.*learner\.algo=dqn"):
        DeviceLearner(ops, NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="dqn")), 4, risk="pow", risk_eta=-2)
    dev = mk()
    assert (dev.risk_kind, dev.risk_eta, dev.t_risk) == (0, 0.0, None), "off: no buffer"
    dev.set_risk("neutral", 7.0)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=wang: learner\.iqn\.risk_eta=9"):
        dev.set_risk("wang", 9)
    dev._risk_fixed = True      # what the first forward_dense leaves
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk.*fixed once the learner has run an update"):
        dev.set_risk("neutral")


def test_declarations():
    from agent0_amd import _abi, ops
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_risk_distort"] == ("int", ["ptr", "ptr", "long long", "int", "double", "ptr"])
    assert protos["a0_tau_cos_features_risk"] == ("int", protos["a0_tau_cos_features"][1][:-1] + ["int", "double", "ptr"])
    assert protos["a0_learner_set_risk"] == ("int", ["ptr", "int", "double"]) and protos["a0_actor_set_risk"] == ("int", ["ptr", "int", "double"])
    header = open(_abi.HEADER).read()
    for k, (name, v) in enumerate(ops.RISK_KINDS.items()):
        assert v == k and f"#define A0_RISK_{name.upper()} {v}\n" in header
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_learner_set_risk.argtypes == [C.c_void_p, C.c_int, C.c_double] and lib.a0_risk_distort.restype == C.c_int
    assert protos["a0_actor_fractions"] == ("int", ["ptr", "ptr"])
    for name in ("risk_distort", "tau_cos_features_risk", "actor_set_risk", "actor_fractions"):
        assert hasattr(ops.HipOps, name)
    assert hasattr(ops.NativeLearner, "set_risk")


def test_argument_checks_are_made_in_front_of_any_launch():
    """Every refusal returns A0_EINVAL under the entry point's name, with the setting and the number, before a pointer is used (the pointers here are never dereferenced)."""
    from agent0_amd import _abi
    lib = _abi.load()
    fake, EINVAL = 1 << 20, -1
    bad_eta = [(1, 0.0), (1, -0.25), (1, 1.5), (1, math.nan), (1, math.inf), (1, 1e-60), (2, 64.5), (2, -70.0), (2, math.nan), (2, -math.inf), (3, 0.0), (3, 1.25),
               (3, math.nan), (4, 8.5), (4, -8.5), (4, math.nan), (4, math.inf)]
    for kind, eta in bad_eta:
        assert lib.a0_risk_distort(fake, fake, 8, kind, eta, None) == EINVAL
        msg = _abi.last_error()
        assert msg.startswith("a0_risk_distort: learner.iqn.risk_eta = ") and "the paper" in msg, (kind, eta, msg)
        assert lib.a0_tau_cos_features_risk(1, 3, 0, None, 0, fake, fake, 4, 64, kind, eta, None) == EINVAL and _abi.last_error().startswith("a0_tau_cos_features_risk: learner.iqn.risk_eta")
    assert "0.25" in (lib.a0_risk_distort(fake, fake, 8, 1, 0.0, None), _abi.last_error())[1] and "0.71" in (lib.a0_risk_distort(fake, fake, 8, 3, 0.0, None), _abi.last_error())[1]
    for kind in (-1, 5, 99):
        assert lib.a0_risk_distort(fake, fake, 8, kind, 0.5, None) == EINVAL and _abi.last_error().startswith(f"a0_risk_distort: learner.iqn.risk = {kind}")
        assert lib.a0_tau_cos_features_risk(1, 3, 0, None, 0, fake, fake, 4, 64, kind, 0.5, None) == EINVAL and "learner.iqn.risk = " in _abi.last_error()
    for args in ((None, fake, 8), (fake, None, 8), (fake, fake, 0), (fake, fake, -3)):
        assert lib.a0_risk_distort(*args, 1, 0.25, None) == EINVAL and _abi.last_error().startswith("a0_risk_distort")
    for taus, out, R, D, ctrl, idx in ((None, fake, 4, 64, None, 0), (fake, None, 4, 64, None, 0), (fake, fake, 0, 64, None, 0), (fake, fake, 4, 0, None, 0),
                                       (fake, fake, 4, 64, fake, -1), (fake, fake, 4, 64, fake, 8)):
        assert lib.a0_tau_cos_features_risk(1, 3, 0, ctrl, idx, taus, out, R, D, 1, 0.25, None) == EINVAL and _abi.last_error().startswith("a0_tau_cos_features_risk")
    assert lib.a0_learner_set_risk(None, 1, 0.25) == EINVAL and "a0_learner_set_risk" in _abi.last_error()
    assert lib.a0_actor_set_risk(None, 1, 0.25) == EINVAL and "a0_actor_set_risk" in _abi.last_error()
