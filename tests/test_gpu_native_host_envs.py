"""GPU (MI355X): host-environment rollouts through the library's actor handle (a0_actor_attach_pool).  A main-schedule Trainer over one HostEnvPool with worker
processes is taken by the handles, and every number of the run — parameters, replay rows, losses, train and test returns, qmax, frame count — equals the
Python classes' run of the same configuration (A0_NATIVE_LOOP=0).  Host envs are the oracle's CPU twin of the synthetic env (tests/host_slices.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _host_atari_slice(env_id, episode_life, seed):
    import host_slices
    return host_slices.synth_slice(seed, 0)


class _DyingSlice:
    """A slice whose step raises at its third step: worker_main stores -1 into its done word and exits."""

    def __init__(self, seed, e0, k):
        import host_slices
        self.env, self.t = host_slices.synth_slice(seed, 0)(e0, k), 0

    def reset(self, **kw):
        return self.env.reset(**kw)

    def step(self, a):
        self.t += 1
        if self.t == 3:
            raise RuntimeError("scripted worker failure")
        return self.env.step(a)

    def close(self):
        pass


def _dying_atari_slice(env_id, episode_life, seed):
    import functools
    return functools.partial(_DyingSlice, seed)


def _trainer(tmp_path, monkeypatch, native, algo="dqn", E=16, extra=(), use_lp=False, slice_fn=_host_atari_slice, tag=""):
    from agent0_amd.common import atari_wrappers
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setattr(atari_wrappers, "real_atari_available", lambda: True)
    monkeypatch.setattr(atari_wrappers, "AtariSlice", slice_fn)
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    logdir = tmp_path / f"{algo}{E}{int(native)}{tag}"
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.num_envs={E}", "actor.sample_steps=12", "learner.batch_size=32", "learner.learner_steps=3",
                           "replay.size=500" if E < 64 else "replay.size=8000", "trainer.training_start_steps=100", "learner.target_update_freq=4",
                           "trainer.test_episodes=2", "wandb=false", "tb=false", f"logdir={logdir}"] + list(extra))
    return Trainer(cfg, use_lp=use_lp), logdir


def test_a_host_pool_trainer_is_taken_by_the_handles(tmp_path, monkeypatch):
    from agent0_amd.common.env_pool import HostEnvPool
    from agent0_amd.deepq.native_loop import NativeLoop
    tr, _ = _trainer(tmp_path, monkeypatch, True)
    try:
        assert isinstance(tr.actors[1].envs, HostEnvPool) and tr.actors[1].envs.W >= 1
        tr.run_iteration()
        assert getattr(tr, "native_loop_reason", None) is None
        assert isinstance(tr._nl, NativeLoop) and tr._nl.pool is tr.actors[1].envs
    finally:
        tr.final(save=False)
    for what, kw, env, reason in (("groups", dict(extra=["actor.env_groups=2"]), {}, "groups"), ("calls", {}, {"A0_ENV_POOL_CALLS": "0"}, "A0_ENV_POOL_CALLS=0"),
                                  ("launch", dict(use_lp=True), {}, "launch schedule")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr, _ = _trainer(tmp_path, monkeypatch, True, tag=what, **kw)
        try:
            tr.run_iteration()
            assert tr._nl is False and reason in tr.native_loop_reason, (what, tr.native_loop_reason)
        finally:
            tr.final(save=False)
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("algo,E,extra", [("dqn", 16, []), ("mdqn", 16, []), ("qr", 16, []), ("c51", 16, ["learner.noisy_net=true", "learner.n_step_q=3"]),
                                          ("iqn", 16, ["replay.policy=prioritize"]), ("fqf", 16, ["learner.dueling_head=true"]), ("dqn", 256, [])])
def test_handle_driven_host_pool_equals_the_python_classes(algo, E, extra, tmp_path, monkeypatch):
    """Six training iterations, then Trainer.final (the test rollouts on the test actor's own pool and a checkpoint): the same bytes and numbers both ways."""
    from agent0_amd.deepq.native_loop import NativeLoop
    res = []
    for native in (True, False):
        tr, logdir = _trainer(tmp_path, monkeypatch, native, algo, E, extra)
        out = [tr.run_iteration(prefetch=(i % 2 == 0)) for i in range(6)]
        assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
        pool = tr.actors[1].envs
        seq, full = pool.seq, pool.full_uploads
        tr.final()
        assert os.path.exists(os.path.join(str(logdir), "final.pth"))
        torch.cuda.synchronize()
        res.append((tr.learner.engine.online.flat.clone(), tr.replay.frames.clone(), tr.replay.act.clone(), tr.replay.rew.clone(), tr.replay.done.clone(),
                    [o["loss"] for o in out], [o["return_train"] for o in out], [o["qmax"] for o in out], list(tr.RTs), tr.frame_count, seq, full))
    a, b = res
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert a[5:] == b[5:]
    assert a[5][-1] is not None, "updates ran"


def test_host_pool_rows_stay_the_pools_own_after_a_python_reset(tmp_path, monkeypatch):
    """Hand-back: after a native rollout the pool's sequence number and current half are the handle's; a host-side reset in between is picked up by the next one."""
    tr, _ = _trainer(tmp_path, monkeypatch, True)
    try:
        pool = tr.actors[1].envs
        s0 = pool.seq
        tr.run_iteration()
        assert pool.seq == s0 + 12 and tr.actors[1].obs.data_ptr() == pool._obs[pool.seq & 1].data_ptr()
        obs, _ = pool.reset()
        tr.actors[1].obs = obs
        s1 = pool.seq
        tr.run_iteration()
        assert pool.seq == s1 + 12 and tr.actors[1].obs.data_ptr() == pool._obs[pool.seq & 1].data_ptr()
    finally:
        tr.final(save=False)


def test_a_dead_worker_fails_the_rollout(tmp_path, monkeypatch):
    """A worker whose env raises stores -1 into its done word and exits: the handle's wait returns an error (RuntimeError here), it does not hang."""
    import time
    tr, _ = _trainer(tmp_path, monkeypatch, True, slice_fn=_dying_atari_slice, tag="dying")
    try:
        t0 = time.time()
        with pytest.raises(RuntimeError, match="worker"):
            tr.run_iteration()
        assert time.time() - t0 < 60
    finally:
        torch.cuda.synchronize()
        tr.actors[1].envs.close()
