"""CPU: the ``actor.eps_ladder`` setting, the C-ABI's declarations for it, and the float64 restatement the GPU tests compare the kernels with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eps_ladder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setting_parses_defaults_to_off_and_round_trips():
    from agent0_amd.deepq import config as cfgmod
    assert cfgmod.ExpConfig().actor.eps_ladder == 0.0
    cfg = cfgmod.parse_overrides(["actor.eps_ladder=7", "actor.min_eps=0.4"])
    assert cfg.actor.eps_ladder == 7.0 and isinstance(cfg.actor.eps_ladder, float) and cfg.actor.min_eps == 0.4
    d = cfgmod.to_dict(cfg)
    assert d["actor"]["eps_ladder"] == 7.0
    assert cfgmod.from_dict(d).actor.eps_ladder == 7.0
    # the alias package follows
    from agent0.deepq import config as alias
    assert alias.parse_overrides(["actor.eps_ladder=0.5"]).actor.eps_ladder == 0.5 and alias.ActorConfig().eps_ladder == 0.0


def test_header_declares_the_sentinel_and_the_two_functions():
    from agent0_amd import _abi
    text = open(_abi.HEADER).read()
    m = re.search(r"#define\s+A0_EPS_PER_ENV\s+\((-?[0-9.]+)f\)", text)
    assert m and float(m.group(1)) == -1.0
    from agent0_amd import ops
    assert ops.EPS_PER_ENV == float(m.group(1))
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_eps_ladder"] == ("int", ["float", "ptr", "float", "int", "long long", "long long", "ptr", "ptr"])
    assert protos["a0_actor_set_eps_ladder"] == ("int", ["ptr", "float", "long long", "long long"])
    # every entry point that takes eps_ptr is still declared with the argument list it had
    for name in ("a0_actor_qhead", "a0_actor_qhead_n", "a0_actor_dist_tail", "a0_actor_quantile_tail", "a0_actor_egreedy_rng"):
        assert "float" in protos[name][1] and protos[name][0] == "int"


def test_ctypes_signatures_agree_with_the_header():
    from agent0_amd import _abi
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_eps_ladder.argtypes == [C.c_float, C.c_void_p, C.c_float, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    assert lib.a0_actor_set_eps_ladder.argtypes == [C.c_void_p, C.c_float, C.c_longlong, C.c_longlong]
    assert lib.a0_eps_ladder.restype == C.c_int and lib.a0_actor_set_eps_ladder.restype == C.c_int


def test_restatement_gives_the_apex_ladder():
    """eps = 0.4, alpha = 7, N = 8: the exponent of env i is 1 + i."""
    got = ref.ladder64(0.4, 7, 0, 8, 8)
    want = np.float64(np.float32(0.4)) ** np.arange(1, 9)
    assert np.allclose(got, want, rtol=1e-15, atol=0)
    # against the decimal figures: 0.4 reaches the kernel as fp32, within 2^-25 of 0.4 relatively, and the k-th power carries k times that
    decimal = np.array([0.4, 0.16, 0.064, 0.0256, 0.01024, 0.004096, 0.0016384, 0.00065536])
    assert (np.abs(got / decimal - 1.0) <= np.arange(1, 9) * 2.0 ** -25 * 1.001).all()
    # a slice of the whole is the whole's slice
    assert np.array_equal(ref.ladder64(0.4, 7, 3, 5, 300), ref.ladder64(0.4, 7, 0, 300, 300)[3:8])


@pytest.mark.parametrize("alpha", [0.5, 7.0])
@pytest.mark.parametrize("eps", [1e-3, 0.01, 0.4, 1 - 2.0 ** -24])
def test_restatement_does_not_increase_with_the_env_index(eps, alpha):
    for N in (2, 5, 65, 300):
        v = ref.ladder64(eps, alpha, 0, N, N)
        assert (np.diff(v) <= 0).all() and (np.diff(ref.ladder32(eps, alpha, 0, N, N)) <= 0).all()
        assert v[0] == np.float64(np.float32(eps)) and 0 < v[-1] <= v[0]


def test_restatement_obeys_the_three_edges():
    for alpha in (0.5, 7.0):
        for eps in (1.0, 1.01, 1.4, float("inf")):                    # eps >= 1: eps itself, bit for bit
            assert np.array_equal(ref.ladder32(eps, alpha, 0, 9, 9), np.full(9, np.float32(eps)))
        for eps in (0.0, -0.25, -1.0):                                # eps <= 0: zero
            assert np.array_equal(ref.ladder32(eps, alpha, 0, 9, 9), np.zeros(9, np.float32))
        for eps in (1e-3, 0.4, 1 - 2.0 ** -24):                       # env 0, and a lone env, keep eps
            assert ref.ladder32(eps, alpha, 0, 4, 300)[0] == np.float32(eps)
            assert ref.ladder32(eps, alpha, 0, 1, 1)[0] == np.float32(eps)


def test_span_over_the_job(monkeypatch):
    from agent0_amd.deepq.dist import eps_ladder_span
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert eps_ladder_span(0, 256) == (0, 256)
    monkeypatch.setenv("WORLD_SIZE", "8")
    assert eps_ladder_span(3, 256) == (768, 2048)
    with pytest.raises(ValueError):
        eps_ladder_span(8, 256)
