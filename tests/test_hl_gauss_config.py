"""CPU: the host side of ``learner.c51.hl_gauss`` — the config key, the validation function and its messages, the declarations in the binding table and the
library's argument checks (which need no device).  The GPU side is tests/test_gpu_hl_gauss.py; the reference is held by tests/test_hl_gauss_reference_helpers.py."""
import ctypes as C
import inspect
import math
import os

import pytest


def test_config_key_parses_and_round_trips():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    assert parse_overrides([]).learner.c51.hl_gauss == 0.0, "the default is off"
    cfg = parse_overrides(["learner.c51.hl_gauss=0.75"])
    assert cfg.learner.c51.hl_gauss == 0.75 and isinstance(cfg.learner.c51.hl_gauss, float)
    assert (cfg.learner.c51.num_atoms, cfg.learner.c51.vmin, cfg.learner.c51.vmax) == (51, -10, 10)
    assert parse_overrides(["learner.c51.hl_gauss=-1"]).learner.c51.hl_gauss == -1.0
    d = to_dict(cfg)
    assert d["learner"]["c51"]["hl_gauss"] == 0.75
    back = from_dict(d)
    assert back.learner.c51.hl_gauss == 0.75 and to_dict(back) == d
    assert from_dict({"learner": {"algo": "c51", "c51": {"num_atoms": 11}}}).learner.c51.hl_gauss == 0.0, "a dictionary written before the key existed"
    from agent0.deepq import config as alias
    assert alias.C51Config().hl_gauss == 0.0 and alias.parse_overrides(["learner.c51.hl_gauss=0.5"]).learner.c51.hl_gauss == 0.5
    doc = config.__doc__
    assert "learner.c51.hl_gauss" in doc and "Farebrother" in doc and "A0_PIPELINE_TARGET=1`` is allowed" in doc


def test_the_validation_function():
    from agent0_amd.deepq import engine
    rho, sigma = engine.hl_gauss_value(0.75)
    assert rho == 0.75 and sigma == 0.75 * (20.0 / 50), "sigma = rho * Delta, formed in double"
    assert engine.hl_gauss_value(0.75, -1.0, 1.0, 2) == (0.75, 1.5)
    assert engine.hl_gauss_value(51.0) == (51.0, 51.0 * (20.0 / 50)), "rho = num_atoms is the limit, and allowed"
    assert engine.hl_gauss_value(0.1, 0.1, 0.7, 3)[1] == 0.1 * ((float.fromhex("0x1.666666p-1") - float.fromhex("0x1.99999ap-4")) / 2), "Delta of the fp32 vmin and vmax, as the kernels get them"
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["hl_gauss"].default == 0.0


@pytest.mark.parametrize("algo", ["dqn", "c51", "qr", "iqn", "fqf", "mdqn"])
@pytest.mark.parametrize("value", [0, 0.0, -1, -0.5, None])
def test_off_values_validate_for_every_algo(algo, value, monkeypatch):
    from agent0_amd.deepq import engine
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    assert engine.hl_gauss_value(value, algo=algo) == (0.0, 0.0)
    assert engine.hl_gauss_value(value, 0.0, 0.0, 1, algo=algo, pipeline_target=True) == (0.0, 0.0), "off is off whatever else is set"


@pytest.mark.parametrize("value,kw", [(math.nan, {}), (math.inf, {}), (-math.inf, {}), (51.5, {}), (2.25, dict(num_atoms=2)), (1e60, dict(num_atoms=64)),
                                      (0.75, dict(vmin=0.0, vmax=1e-40)), (0.75, dict(vmin=3.0, vmax=3.0)), (0.75, dict(vmin=1.0, vmax=-1.0)), (1e-45, dict(vmin=-1e-3, vmax=1e-3)),
                                      (1.0, dict(vmin=-3e38, vmax=3e38, num_atoms=2)), (0.75, dict(vmax=math.nan))])
@pytest.mark.parametrize("algo", ["c51", "dqn"])
def test_bad_numbers_are_refused_with_the_setting_and_the_number_named(value, kw, algo):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.c51\.hl_gauss=") as e:
        engine.hl_gauss_value(value, algo=algo, **kw)
    assert repr(float(value)) in str(e.value), "the number is named"
    if algo == "c51" and math.isfinite(value):
        assert ("num_atoms" in str(e.value)) or ("normal fp32" in str(e.value))


def test_other_algos_are_refused_by_name():
    from agent0_amd.deepq import engine
    for algo in ("dqn", "qr", "iqn", "fqf", "mdqn"):
        with pytest.raises(ValueError, match=rf"learner\.c51\.hl_gauss=0\.75.*learner\.algo={algo}"):
            engine.hl_gauss_value(0.75, algo=algo)


def test_a_staged_target_pass_is_allowed(monkeypatch):
    """c51's separately staged target pass (A0_PIPELINE_TARGET=1, tstage) ends at the target's fc1 slabs; the loss kernel reads them as it does without the stage,
    so the setting has nothing to refuse there (aug_shift and net_reset refuse it because THEY change what that stage reads)."""
    from agent0_amd.deepq import engine
    assert engine.hl_gauss_value(0.75, pipeline_target=True) == engine.hl_gauss_value(0.75, pipeline_target=False) == (0.75, 0.75 * 0.4)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    assert engine.hl_gauss_value(0.75)[0] == 0.75
    assert "ALLOWED" in engine.hl_gauss_value.__doc__


def test_a_backend_without_the_kernel_is_refused():
    """The engine composes kernels through ``ops``; the host emulation has no c51_hl_gauss_head_loss_slabs, and a missing kernel is an error, not a fall-back."""
    import cpu_ops
    import recipe
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    ops = cpu_ops.CpuOps()
    assert not hasattr(ops, "c51_hl_gauss_head_loss_slabs")
    L = NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="c51"))
    with pytest.raises(ValueError, match=r"learner\.c51\.hl_gauss=0\.75.*c51_hl_gauss_head_loss_slabs"):
        DeviceLearner(ops, L, 4, hl_gauss=0.75)
    with pytest.raises(ValueError, match=r"learner\.c51\.hl_gauss=0\.75.*learner\.algo=dqn"):
        DeviceLearner(ops, NetLayout.from_spec(recipe.NetSpec(action_dim=4, obs_shape=(4, 84, 84), algo="dqn")), 4, hl_gauss=0.75)
    with pytest.raises(ValueError, match=r"learner\.c51\.hl_gauss=nan"):
        DeviceLearner(ops, L, 4, hl_gauss=math.nan)
    for off in (0.0, -2.0):
        dev = DeviceLearner(ops, L, 4, hl_gauss=off)
        assert dev.hl_gauss == 0.0 and dev.hl_gauss_sigma == 0.0


def test_declarations():
    from agent0_amd import _abi, ops
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    c51 = protos["a0_loss_c51"][1]
    assert protos["a0_loss_c51_hl_gauss"] == ("int", c51[:13] + ["double"] + c51[13:]), "a0_loss_c51's arguments plus sigma, a double, behind vmax"
    slabs = protos["a0_c51_head_loss_slabs"][1]
    assert protos["a0_c51_hl_gauss_head_loss_slabs"] == ("int", slabs[:22] + ["double"] + slabs[22:])
    assert slabs[19:23] == ["float", "float", "float", "int"] and c51[10:14] == ["float", "float", "float", "int"], "gamma_n, vmin, vmax, B: the signatures stay"
    assert protos["a0_learner_set_hl_gauss"] == ("int", ["ptr", "double"])
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_learner_set_hl_gauss.argtypes == [C.c_void_p, C.c_double] and lib.a0_loss_c51_hl_gauss.restype == C.c_int
    assert hasattr(ops.HipOps, "loss_c51_hl_gauss") and hasattr(ops.HipOps, "c51_hl_gauss_head_loss_slabs") and hasattr(ops.NativeLearner, "set_hl_gauss")


def test_argument_checks_are_made_in_front_of_any_launch():
    """Every refusal returns A0_EINVAL under the entry point's name before a pointer is used (the pointers here are never dereferenced)."""
    from agent0_amd import _abi
    lib = _abi.load()
    fake, EINVAL = 1 << 20, -1
    T = 51
    ok = dict(sigma=0.3, T=T, vmin=-10.0, vmax=10.0, B=2, logits=fake)
    alone = lambda **kw: (lambda a: lib.a0_loss_c51_hl_gauss(a["logits"], fake, 4, a["T"], fake, fake, fake, fake, fake, fake, 0.99, a["vmin"], a["vmax"], a["sigma"], a["B"],
                                                             fake, fake, None, fake, None))({**ok, **kw})
    fused = lambda **kw: (lambda a: lib.a0_c51_hl_gauss_head_loss_slabs(a["logits"], 2 * 256, 1, 2, fake, 2 * 256, 1, -1, fake, fake, 256, 4, a["T"], 0, fake, fake, fake, fake, fake,
                                                                        0.99, a["vmin"], a["vmax"], a["sigma"], a["B"], fake, fake, None, None, None, None, fake, None))({**ok, **kw})
    bad = [dict(sigma=math.nan), dict(sigma=math.inf), dict(sigma=0.0), dict(sigma=-0.3), dict(sigma=1e-40), dict(sigma=1e39), dict(sigma=0.4 * T * 1.001),
           dict(vmin=1.0, vmax=1.0), dict(vmin=1.0, vmax=-1.0)]
    for name, call in (("a0_loss_c51_hl_gauss", alone), ("a0_c51_hl_gauss_head_loss_slabs", fused)):
        for kw in bad:
            assert call(**kw) == EINVAL, (name, kw)
            err = _abi.last_error()
            assert err.startswith(name) and "learner.c51.hl_gauss" in err and "sigma = " in err, (name, kw, err)
        for kw in (dict(logits=None), dict(T=1), dict(T=65), dict(B=0)):
            assert call(**kw) == EINVAL and _abi.last_error().startswith(name), (name, kw)
    assert lib.a0_learner_set_hl_gauss(None, 0.75) == EINVAL and "a0_learner_set_hl_gauss" in _abi.last_error()
