"""CPU: the host side of ``learner.weight_decay`` — the config key and its docstring entry, the value helper with its refusals, the numpy restatement against
itself, the new exports in the binding table and their argument checks (which run in front of any launch).  The GPU side is tests/test_gpu_weight_decay.py."""
import math

import numpy as np
import pytest

import weight_decay_ref as R


def test_config_key_parses_and_round_trips():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.weight_decay == 0.0 and isinstance(cfg.learner.weight_decay, float)
    cfg = parse_overrides(["learner.weight_decay=0.1"])
    assert cfg.learner.weight_decay == 0.1 and isinstance(cfg.learner.weight_decay, float)
    assert parse_overrides(["learner.weight_decay=1e-1"]).learner.weight_decay == 0.1
    with pytest.raises(Exception):
        parse_overrides(["learner.weight_decay=heavy"])
    d = to_dict(cfg)
    assert d["learner"]["weight_decay"] == 0.1
    back = from_dict(d)
    assert back.learner.weight_decay == 0.1 and to_dict(back) == d
    assert from_dict({"learner": {"algo": "dqn"}}).learner.weight_decay == 0.0, "a dictionary written before the key existed"
    doc = " ".join(config.__doc__.split())
    for words in ("learner.weight_decay", "torch.optim.AdamW", "param_norm", "2^-24", "not the fqf fraction net", "Masks that exempt biases or sigmas are not offered"):
        assert words in doc, words


@pytest.mark.parametrize("value", [0.0, -0.0, -1.0, -5, None, float("-inf")])
def test_the_off_values(value):
    import inspect
    from agent0_amd.deepq import engine
    got = engine.weight_decay_value(value, 5e-4)
    assert isinstance(got, float) and got == 0.0
    assert inspect.signature(engine.DeviceLearner.__init__).parameters["weight_decay"].default == 0.0


@pytest.mark.parametrize("lam,lr", [(0.1, 5e-4), (1e-2, 1e-4), (20.0, 5e-4), (1999.0, 5e-4), (2.0 ** -24 / 5e-4 * 1.001, 5e-4), (0.5, 1.0)])
def test_the_value_helper_gives_the_fp32_coefficient(lam, lr):
    from agent0_amd.deepq import engine
    c = engine.weight_decay_value(lam, lr)
    assert isinstance(c, float) and c == float(np.float32(lr * lam)) == float(R.coef32(lr, lam)) and R.C_MIN <= c < 1.0


def test_the_value_helper_refuses_with_the_numbers_named():
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.weight_decay=nan"):
        engine.weight_decay_value(float("nan"), 5e-4)
    for lam in (2000.0, 1e9, float("inf"), 2000.0 * (1 - 2.0 ** -30)):      # the last product rounds to 1.0f
        with pytest.raises(ValueError, match=r"learner\.weight_decay") as e:
            engine.weight_decay_value(lam, 5e-4)
        assert "0.0005" in str(e.value) and repr(lam) in str(e.value) and "below 1" in str(e.value)
    for lam in (1e-4, 1e-30, 5e-324):
        with pytest.raises(ValueError, match=r"learner\.weight_decay") as e:
            engine.weight_decay_value(lam, 5e-4)
        assert "0.0005" in str(e.value) and repr(lam) in str(e.value) and "2^-24" in str(e.value) and repr(2.0 ** -24) in str(e.value)
    assert engine.weight_decay_value(2.0 ** -24, 1.0) == 2.0 ** -24, "the smallest coefficient that is accepted"


def test_reference_arithmetic():
    # c is rounded once: 5e-5 is not a float
    assert R.coef32(5e-4, 0.1).dtype == np.float32 and float(R.coef32(5e-4, 0.1)) != 5e-4 * 0.1
    g = np.random.default_rng(5)
    p = g.standard_normal(4099).astype(np.float32)
    p[:8] = [0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38, 1.0]
    for c in (2.0 ** -24, 5e-5, 0.5):
        out = R.decay(p, c)
        assert out.dtype == np.float32
        # zeros stay zero (-0 - (-0) is +0 under round-to-nearest, on the device as here), nothing grows, nothing changes sign
        assert np.array_equal(out[:2].view(np.uint32), np.zeros(2, np.uint32))
        assert bool((np.abs(out) <= np.abs(p)).all()) and bool((np.signbit(out) == np.signbit(p))[p != 0].all())
        # two roundings, not one: where they differ from the single rounding of p * (1 - c) it is by one ulp at the most
        one = (p.astype(np.float64) * (1.0 - float(np.float32(c)))).astype(np.float32)
        assert int(np.abs(out.view(np.int32).astype(np.int64) - one.view(np.int32).astype(np.int64))[p != 0].max()) <= 1
    assert np.array_equal(R.decay(p, 0.5), (p - np.float32(0.5) * p).astype(np.float32))
    # 2^-24 still moves a float: 1.0 loses half an ulp, which rounds to even (stays), its odd neighbour moves
    x = np.array([1.0, np.nextafter(np.float32(1.0), np.float32(2.0))], np.float32)
    assert R.decay(x, 2.0 ** -24)[1] == np.float32(1.0)
    # the partial sums: the split, the zeros behind the data, the norm
    for n in (5, 1025, 77824 + 37):
        ch = R.chunk_of(n)
        assert ch % 4 == 0 and ch * R.P >= n and (ch - 4) * R.P < n
        q = g.standard_normal(n).astype(np.float32)
        parts = R.partials_f64(q)
        used = (n + ch - 1) // ch
        assert parts.shape == (R.P,) and bool((parts[used:] == 0.0).all()) and bool((parts[:used] > 0.0).all())
        want = math.sqrt(math.fsum((q.astype(np.float64) ** 2).tolist()))
        assert abs(R.norm_of(parts) - want) <= n * 2.0 ** -53 * want


def test_the_header_declares_and_the_binding_matches():
    from agent0_amd import _abi
    protos = {n: (r, t) for r, n, t in _abi.parse_header()}
    assert protos["a0_weight_decay"] == ("int", ["ptr", "long long", "double", "ptr", "ptr", "ptr", "ptr"])
    assert protos["a0_learner_set_weight_decay"] == ("int", ["ptr", "double", "ptr"])
    assert protos["a0_learner_weight_decay_partials"] == ("int", ["ptr", "ptr"])
    # the existing exports are what they were
    assert protos["a0_grad_norm_partials"] == ("int", ["ptr", "long long", "ptr", "ptr"]) and len(protos["a0_adam_step_sync"][1]) == 16
    assert len(protos["a0_adam_step_sync_wt"][1]) == 24 and len(protos["a0_update_tail"][1]) == 22 and protos["a0_learner_set_target_tau"] == ("int", ["ptr", "double"])
    lib = _abi.load()
    for name in ("a0_weight_decay", "a0_learner_set_weight_decay", "a0_learner_weight_decay_partials"):
        assert len(getattr(lib, name).argtypes) == len(protos[name][1]), name
    from agent0_amd.ops import HipOps, NativeLearner
    assert callable(HipOps.weight_decay) and callable(NativeLearner.set_weight_decay)


def test_arguments_are_checked_before_any_launch():
    """Validation happens in front of every HIP call, so it runs here."""
    import ctypes as C
    from agent0_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    st, parts = p + 4 * 1024, p + 4 * 2048
    ok_args = lambda **kw: dict(dict(params=p, n=64, c=0.5, state=st, flag=None, partials=parts), **kw)
    call = lambda a: lib.a0_weight_decay(a["params"], a["n"], a["c"], a["state"], a["flag"], a["partials"], None)
    for bad in (dict(params=None), dict(state=None), dict(partials=None), dict(n=0), dict(n=-3), dict(params=p + 2), dict(partials=parts + 4)):
        assert call(ok_args(**bad)) == -1 and "a0_weight_decay" in _abi.last_error(), bad
    for c in (1.0, 1.5, 0.0, -0.5, float("nan"), float("inf"), 1.0 - 2.0 ** -30, 2.0 ** -25, 2.0 ** -24 * (1 - 2.0 ** -20)):
        assert call(ok_args(c=c)) == -1 and "a0_weight_decay" in _abi.last_error() and "2^-24" in _abi.last_error(), c
    assert lib.a0_learner_set_weight_decay(None, 0.1, None) == -1 and "a0_learner_set_weight_decay" in _abi.last_error()
    assert lib.a0_learner_weight_decay_partials(None, None) == -1 and "a0_learner_weight_decay_partials" in _abi.last_error()
