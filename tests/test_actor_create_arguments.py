"""CPU: a0_actor_create refuses a null pointer or a bad description with A0_EINVAL and a fixed message before any HIP call (csrc/runtime.hip), so every case here runs
without a GPU: nothing is allocated, `out` stays untouched.

Check order: null desc / out, then every field of the description under one message: E, T, A and n_step at least 1, reset_noise_freq at least 0 (0 = NoisyNet's
default of 4), a positive discount, env_task one of the three synthetic tasks, and the chase task with at least four actions."""
import ctypes as C

import pytest

EINVAL = -1
TASK_STREAM, TASK_CHASE = 0, 2

NULL = "a0_actor_create: null argument"
BAD = "a0_actor_create: bad description"

VALID = dict(E=4, T=8, A=6, dueling=0, n_step=1, discount=0.99, seed=7, rank=0, env_task=TASK_STREAM, reset_noise_freq=0)


@pytest.fixture(scope="module")
def lib():
    from agent0_amd import _abi
    return _abi.load()


def _refused(lib, null=None, **bad):
    """Calls a0_actor_create with the valid description overridden by `bad` (`null` = "desc" / "out" passes that pointer as NULL); asserts A0_EINVAL and an untouched
    `out`, and returns the message."""
    from agent0_amd import _abi
    from agent0_amd.deepq.native_loop import _ActorDesc
    assert set(bad) <= set(VALID), bad
    assert [n for n, _ in _ActorDesc._fields_] == list(VALID)
    desc = _ActorDesc(**dict(VALID, **bad))
    out = C.c_void_p(0x5A5A)
    assert lib.a0_actor_create(None if null == "desc" else C.addressof(desc), None if null == "out" else C.addressof(out)) == EINVAL, (null, bad)
    assert out.value == 0x5A5A
    return _abi.last_error()


@pytest.mark.parametrize("null", ["desc", "out"])
def test_null_arguments(lib, null):
    assert _refused(lib, null=null) == NULL


FIELDS = [dict(E=0), dict(T=0), dict(A=0), dict(n_step=0), dict(reset_noise_freq=-1), dict(discount=0.0), dict(discount=-0.5), dict(discount=float("nan")),
          dict(env_task=TASK_STREAM - 1), dict(env_task=TASK_CHASE + 1), dict(env_task=TASK_CHASE, A=3)]


@pytest.mark.parametrize("bad", FIELDS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_description_fields(lib, bad):
    assert _refused(lib, **bad) == BAD


def test_a_null_pointer_is_reported_before_the_description(lib):
    assert _refused(lib, null="out", E=0) == NULL
