"""CPU: a0_learner_create and a0_learner_create_on refuse a bad description with A0_EINVAL and a fixed message before any HIP call (csrc/learner.hip,
a0_learner_desc_check), so every case here runs without a GPU: nothing is allocated, `out` stays untouched.

Check order: null desc / out; the caller's loss ring (create_on only); the fields every learner shares (A, B, n_step, discount, lr, target_update_freq, algo) under one
message; then the one check of the description's own algo.  Three descriptions with two faults each pin that order."""
import ctypes as C

import pytest

EINVAL = -1
ALGO = {"dqn": 0, "c51": 1, "iqn": 2, "fqf": 3, "qr": 4, "mdqn": 5}
CREATORS = ["a0_learner_create", "a0_learner_create_on"]

NULL = "a0_learner_create: null argument"
RING = "a0_learner_create_on: loss_ring_cap"
BAD = "a0_learner_create: bad description"
QR = "a0_learner_create: qr needs 1 <= num_atoms <= 1024"
MDQN = "a0_learner_create: mdqn needs tau > 0"
FQF = "a0_learner_create: fqf needs 2 <= F <= 32, A + dueling <= 32"
IQN = "a0_learner_create: iqn needs K, N, N' >= 1, A + dueling <= 32"
DQN = "a0_learner_create: the dqn handle covers scalar heads with A + dueling <= 24 actions"
C51 = "a0_learner_create: c51 needs 2 <= num_atoms <= 64 and vmin < vmax"

VALID = dict(A=6, dueling=0, double_q=0, B=32, n_step=1, discount=0.99, lr=5e-4, adam_eps=0.0, target_update_freq=500, algo=0, num_atoms=51, vmin=-10.0, vmax=10.0, noisy=0,
             seed=7, iqn_K=32, iqn_N=64, iqn_N_dash=64, fqf_F=32, mdqn_tau=0.03, mdqn_lo=-1.0, max_grad_norm=-1.0)


@pytest.fixture(scope="module")
def lib():
    from agent0_amd import _abi
    return _abi.load()


def _refused(lib, fn, algo, ring_cap=None, null=None, **bad):
    """Calls `fn` with a valid `algo` description overridden by `bad` (create_on: over a caller's loss ring of `ring_cap` floats when given; `null` = "desc" / "out"
    passes that pointer as NULL); asserts A0_EINVAL and an untouched `out`, and returns the message."""
    from agent0_amd import _abi
    from agent0_amd.deepq.native_loop import _LearnerBuffers
    assert set(bad) <= set(VALID), bad
    desc = _abi.LearnerDesc(**dict(VALID, algo=ALGO.get(algo, algo), **bad))
    out = C.c_void_p(0x5A5A)
    args = [None if null == "desc" else C.addressof(desc)]
    if fn == "a0_learner_create_on":
        bufs = _LearnerBuffers(loss_ring=0x10000, loss_ring_cap=ring_cap) if ring_cap is not None else None      # a stand-in pointer that nothing may read
        args.append(C.addressof(bufs) if bufs is not None else None)
    args.append(None if null == "out" else C.addressof(out))
    assert getattr(lib, fn)(*args) == EINVAL, (fn, algo, bad)
    assert out.value == 0x5A5A
    return _abi.last_error()


def _id(v):
    return v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items())


@pytest.mark.parametrize("null", ["desc", "out"])
@pytest.mark.parametrize("fn", CREATORS)
def test_null_arguments(lib, fn, null):
    assert _refused(lib, fn, "dqn", null=null) == NULL


@pytest.mark.parametrize("cap", [0, -1])
def test_a_callers_loss_ring_needs_a_capacity(lib, cap):
    assert _refused(lib, "a0_learner_create_on", "dqn", ring_cap=cap) == RING


SHARED = [dict(A=0), dict(B=0), dict(n_step=0), dict(discount=0.0), dict(discount=-0.5), dict(discount=float("nan")), dict(lr=-1e-4), dict(lr=float("nan")),
          dict(target_update_freq=0)]


@pytest.mark.parametrize("bad", SHARED, ids=_id)
@pytest.mark.parametrize("algo", list(ALGO))
@pytest.mark.parametrize("fn", CREATORS)
def test_shared_fields(lib, fn, algo, bad):
    assert _refused(lib, fn, algo, **bad) == BAD


@pytest.mark.parametrize("algo", [-1, 6])
@pytest.mark.parametrize("fn", CREATORS)
def test_unknown_algo(lib, fn, algo):
    assert _refused(lib, fn, algo) == BAD


PER_ALGO = [("qr", dict(num_atoms=0), QR), ("qr", dict(num_atoms=1025), QR),
            ("mdqn", dict(mdqn_tau=0.0), MDQN), ("mdqn", dict(mdqn_tau=float("nan")), MDQN),
            ("fqf", dict(fqf_F=1), FQF), ("fqf", dict(fqf_F=33), FQF), ("fqf", dict(A=33), FQF), ("fqf", dict(A=32, dueling=1), FQF),
            ("iqn", dict(iqn_K=0), IQN), ("iqn", dict(iqn_N=0), IQN), ("iqn", dict(iqn_N_dash=0), IQN), ("iqn", dict(A=33), IQN), ("iqn", dict(A=32, dueling=1), IQN),
            ("dqn", dict(A=25), DQN), ("dqn", dict(A=24, dueling=1), DQN),
            ("c51", dict(num_atoms=1), C51), ("c51", dict(num_atoms=65), C51), ("c51", dict(vmin=10.0, vmax=10.0), C51), ("c51", dict(vmin=10.0, vmax=-10.0), C51),
            ("c51", dict(vmax=float("nan")), C51)]


@pytest.mark.parametrize("algo,bad,msg", PER_ALGO, ids=[f"{a}-{_id(b)}" for a, b, _ in PER_ALGO])
@pytest.mark.parametrize("fn", CREATORS)
def test_the_algos_own_check(lib, fn, algo, bad, msg):
    assert _refused(lib, fn, algo, **bad) == msg


@pytest.mark.parametrize("fn", CREATORS)
def test_a_null_pointer_is_reported_before_the_description(lib, fn):
    assert _refused(lib, fn, "dqn", null="out", A=0) == NULL


def test_the_loss_ring_is_reported_before_the_description(lib):
    assert _refused(lib, "a0_learner_create_on", "dqn", ring_cap=0, B=0) == RING


@pytest.mark.parametrize("fn", CREATORS)
def test_a_shared_field_is_reported_before_the_algos_own_check(lib, fn):
    assert _refused(lib, fn, "c51", n_step=0, num_atoms=1) == BAD
