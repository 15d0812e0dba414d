"""GPU (MI355X): a0_actor_rollout refuses handles that do not fit together, and heads its tail kernels do not cover, with A0_EINVAL and a fixed message
(csrc/runtime.hip).  E = 16 envs, rollouts of 4 steps, a ring of 64 rows; every call here is refused on the host.

Check order: a null handle; actor, learner and replay of different shapes (the learner's A or dueling flag, a ring smaller than E); then what no step of the rollout
could run: a scalar head (dqn / mdqn) with A + dueling > 24, a c51 / qr head wider than the tail kernel's 160 KiB of LDS (4 envs x (A * T + T) floats).  A refused
rollout leaves the actor's state and the ring's rows as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1
E, T, SIZE, B, OBS = 16, 4, 64, 32, 4 * 84 * 84

NULL = "a0_actor_rollout: null argument"
SHAPES = "a0_actor_rollout: actor, learner and replay were created for different shapes"
SCALAR = "a0_actor_rollout: scalar heads with A + dueling <= 24 actions"
WIDE = "a0_actor_rollout: head too wide for the distributional tail kernel"


@pytest.fixture(scope="module")
def lib():
    from agent0_amd import _abi
    from agent0_amd.ops import HipOps
    assert "gfx950" in HipOps().device_info()[2]
    return _abi.load()


class Handles:
    """Creates handles through the C-ABI and destroys them when the module's tests are done."""

    def __init__(self, lib):
        self.lib, self.made = lib, []

    def learner(self, A, dueling=0, algo="dqn", num_atoms=51):
        from agent0_amd.ops import NativeLearner
        nat = NativeLearner(self.lib, A=A, dueling=dueling, double_q=False, B=B, algo=algo, num_atoms=num_atoms, seed=7)
        self.made.append(nat.close)
        return nat.h

    def actor(self, A, dueling=0):
        from agent0_amd import _abi
        from agent0_amd.deepq.native_loop import _ActorDesc
        d, h = _ActorDesc(E, T, A, dueling, 1, 0.99, 7, 0, 0, 0), C.c_void_p()
        _abi.check(self.lib.a0_actor_create(C.addressof(d), C.addressof(h)), "a0_actor_create")
        self.made.append(lambda: self.lib.a0_actor_destroy(h))
        return h

    def ring(self, size):
        from agent0_amd import _abi
        from agent0_amd.deepq.native_loop import _RbufDesc
        d, h = _RbufDesc(size, OBS, min(B, size), 0, 0.5, 0.01, 0.4, 1000, 11), C.c_void_p()
        _abi.check(self.lib.a0_rbuf_create(C.addressof(d), C.addressof(h)), "a0_rbuf_create")
        self.made.append(lambda: self.lib.a0_rbuf_destroy(h))
        return h


@pytest.fixture(scope="module")
def make(lib):
    m = Handles(lib)
    yield m
    torch.cuda.synchronize()
    for close in reversed(m.made):
        close()


@pytest.fixture(scope="module")
def base(make):
    """a dqn learner and an actor of A = 6 without dueling, and the ring"""
    return make.learner(6), make.actor(6), make.ring(SIZE)


def _refused(lib, actor, learner, ring):
    from agent0_amd import _abi
    st = torch.cuda.current_stream().cuda_stream
    assert lib.a0_actor_rollout(actor, learner, ring, C.c_float(0.5), st) == EINVAL
    return _abi.last_error()


def _actor_state(lib, actor):
    n = int(lib.a0_actor_state_size(actor))
    blob = np.zeros(n, np.uint8)
    assert lib.a0_actor_state_save(actor, blob.ctypes.data, n, torch.cuda.current_stream().cuda_stream) == 0
    return blob


def _ring_rows(lib, ring):
    dev = torch.device("cuda", torch.cuda.current_device())
    frames = torch.empty(SIZE * 2 * OBS, dtype=torch.uint8, device=dev)
    act, rew, done = torch.empty(SIZE, dtype=torch.int32, device=dev), torch.empty(SIZE, device=dev), torch.empty(SIZE, device=dev)
    assert lib.a0_rbuf_read(ring, SIZE, frames.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return [t.cpu() for t in (frames, act, rew, done)]


@pytest.mark.parametrize("which", ["actor", "learner", "replay"])
def test_a_null_handle(lib, base, which):
    learner, actor, ring = base
    assert _refused(lib, None if which == "actor" else actor, None if which == "learner" else learner, None if which == "replay" else ring) == NULL


def test_a_learner_of_another_action_count(lib, make, base):
    _, actor, ring = base
    assert _refused(lib, actor, make.learner(7), ring) == SHAPES


def test_a_learner_whose_dueling_flag_differs(lib, make, base):
    _, actor, ring = base
    assert _refused(lib, actor, make.learner(6, dueling=1), ring) == SHAPES


def test_a_ring_smaller_than_the_env_count(lib, make, base):
    learner, actor, _ = base
    assert _refused(lib, actor, learner, make.ring(E - 1)) == SHAPES


@pytest.mark.parametrize("A,dueling", [(25, 0), (24, 1)])
def test_a_scalar_head_with_more_than_24_rows(lib, make, A, dueling):
    """An mdqn learner may be that wide (it then runs layer by layer); the actor's scalar tail stages A + dueling head rows in LDS and covers 24.  The refusal leaves
    the actor where it was (step count 0, every word and buffer of its state blob) and the ring's rows as they were."""
    learner, actor, ring = make.learner(A, dueling=dueling, algo="mdqn"), make.actor(A, dueling=dueling), make.ring(SIZE)
    state0, rows0 = _actor_state(lib, actor), _ring_rows(lib, ring)
    assert _refused(lib, actor, learner, ring) == SCALAR
    torch.cuda.synchronize()
    state1, rows1 = _actor_state(lib, actor), _ring_rows(lib, ring)
    assert state1[:8 * 32].view(np.int64)[13] == 0, "the actor's step count (word 13 of the blob's header)"
    assert np.array_equal(state0, state1), "the actor's state blob"
    assert all(torch.equal(x, y) for x, y in zip(rows0, rows1)), "the ring's rows"
    assert lib.a0_rbuf_len(ring) == 0 and lib.a0_rbuf_write_cursor(ring) == 0


def test_a_distributional_head_wider_than_the_tail_kernels_lds(lib, make):
    """qr with A = 10 and 1024 quantiles: A * T + T = 11 264 floats per env, above the 10 240 that four envs' rows may take of 160 KiB"""
    learner, actor, ring = make.learner(10, algo="qr", num_atoms=1024), make.actor(10), make.ring(SIZE)
    assert _refused(lib, actor, learner, ring) == WIDE
    torch.cuda.synchronize()
