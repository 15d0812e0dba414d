"""GPU (MI355X): grouped host environments (``actor.env_groups``, env_pool.HostEnvGroups) for every head, NoisyNet and test rollouts, and the quantile heads'
actor tail without the env step (a0_actor_quantile_tail).

A grouped rollout steps one group of envs on the CPU while the GPU infers the other; every env must see exactly what it sees in a one-group rollout.  The
references are the device-resident synthetic env (the oracle's CPU twin of it runs inside the host workers, tests/host_slices.py) and, end to end, the same
Trainer with one group."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu


def make_cfg(algo, E, logdir, **kw):
    from agent0_amd.deepq.config import parse_overrides
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.num_envs={E}", "wandb=false", "tb=false", f"logdir={logdir}"] + [f"{k}={v}" for k, v in kw.items()])
    cfg.obs_shape = (4, 84, 84)
    cfg.action_dim = 4
    return cfg


def _model(cfg, spec):
    from agent0_amd.deepq.model import DeepQNet
    model = DeepQNet(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(spec, 11).items()})
    return model


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("with_ctrl", [False, True])
@pytest.mark.parametrize("algo,dueling", [("iqn", False), ("iqn", True), ("fqf", False), ("fqf", True)])
def test_quantile_tail_equals_the_merged_step_and_the_four_launch_chain(algo, dueling, with_ctrl, tmp_path):
    """a0_actor_quantile_tail on the head GEMM's slabs: the action and max-Q of a0_actor_quantile_tail_env_step on the same slabs, and of the chain it replaces in the
    actor (head with its reduction -> a0_select_action -> a0_actor_egreedy_rng), for iqn (mode 1) and fqf (mode 3), with and without dueling, with the
    Philox offsets and epsilon passed by value or through the control block / device scalar (hipGraph replay)."""
    from agent0_amd.deepq.engine import Workspace
    E = 64
    cfg = make_cfg(algo, E, tmp_path, **{"learner.dueling_head": str(dueling).lower()})
    model = _model(cfg, recipe.NetSpec(algo, 4, dueling=dueling))
    ops, dev, L = model.ops, model._dev, model.L
    n_tau = L.F if algo == "fqf" else int(cfg.learner.iqn.K)
    ws = Workspace(ops, L, E, n_tau)
    gen = torch.Generator().manual_seed(3)
    ws.act3.copy_(torch.rand(E * L.feat, generator=gen).to(ops.device))
    if algo == "fqf":
        dev.fqf_taus(ws, E)
        taus, aux, mode = ws.tau_hat, ws.tau_all, 3
    else:
        taus, aux, mode = torch.rand(E * n_tau, generator=gen).to(ops.device), None, 1
    ns = ops.dense_fwd_partial_slabs(E * n_tau, L.Npad, 512)
    slabs = ops.empty(ns * E * n_tau * L.Npad)
    assert dev.head_slabs(ws, E, taus, n_tau, slabs) == ns
    _, bh = dev.wb("head")
    ctrl, eps_ptr = None, None
    if with_ctrl:
        ctrl = ops.zeros(8, dtype=torch.int64)
        ctrl[2], ctrl[3] = 8, 20                               # A0_CTRL_RNG_ACTION, A0_CTRL_RNG_UNIFORM
        eps_ptr = torch.tensor([0.45], device=ops.device)
    seed, sa, su, off_a, off_u, eps = 0x1234_0077, 2, 1, 40, 44, 0.3
    common = (slabs, ns, bh, L.Npad, L.A, n_tau, L.dueling, mode, aux, E, seed, sa, su, off_a, off_u, eps)
    act1, q1 = ops.zeros(E, dtype=torch.int32), ops.zeros(E)
    ops.actor_quantile_tail(*common, act1, q1, ctrl, eps_ptr)
    # the merged kernel with a throwaway env around it
    nb, n = E * 4 * 84 * 84, 1
    u8 = lambda k: ops.zeros(k, dtype=torch.uint8)
    act2, q2 = ops.zeros(E, dtype=torch.int32), ops.zeros(E)
    ops.actor_quantile_tail_env_step(*common, act2, q2, ctrl, eps_ptr, 5, 0, 1, u8(nb), u8(nb), ops.zeros(E), ops.zeros(E), ops.zeros(E), n, 0, 0.99,
                                     ops.zeros(n * E, dtype=torch.int32), ops.zeros(n * E), ops.zeros(n * E), u8(nb), u8(E * 8 * 84 * 84), E, 0,
                                     ops.zeros(E, dtype=torch.int32), ops.zeros(E), ops.zeros(E))
    # the generic chain: head (its own reduction + dueling) -> first-max selection -> epsilon-greedy draw
    greedy, act3, q3 = ops.zeros(E, dtype=torch.int32), ops.zeros(E, dtype=torch.int32), ops.zeros(E)
    dev.head(ws, E, taus, n_tau)
    dev.select(ws, E, n_tau, greedy, qmax=q3)
    ops.actor_egreedy_rng(greedy, seed, sa, su, off_a, off_u, L.A, eps, E, act3, q3, None, ctrl, eps_ptr)
    torch.cuda.synchronize()
    assert torch.equal(act1, act2) and torch.equal(q1, q2)
    assert torch.equal(act1, act3) and torch.equal(q1, q3)
    assert bool((act1 != greedy).any()) and bool((act1 == greedy).any()), "both the greedy and the random branch are taken"


# ------------------------------------------------------------------------------------------------ grouped rollouts == the device env
def _rollouts(logdir, algo, E, groups, workers, n_step, T, rollouts, noisy=False, replay_size=300, extra=None):
    """(replay frames, act, rew, done, episode returns, per-step max-Q) of ``rollouts`` rollouts on the device env and on the grouped host env."""
    import host_slices
    from agent0_amd.common.env_pool import HostEnvGroups
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.replay import ReplayDataset
    spec = recipe.NetSpec(algo, 4, noisy=noisy, num_atoms=200 if algo == "qr" else 51)
    outs = []
    for host in (False, True):
        cfg = make_cfg(algo, E, logdir, **{"learner.n_step_q": n_step, "actor.sample_steps": T, "replay.size": replay_size, "learner.batch_size": 8,
                                   "learner.noisy_net": str(noisy).lower(), "learner.reset_noise_freq": 4, **(extra or {})})
        model = _model(cfg, spec)
        replay = ReplayDataset(cfg, ops=model.ops)
        envs = HostEnvGroups(host_slices.synth_slice(cfg.seed, 0), E, groups=groups, obs_shape=(4, 84, 84), action_dim=4, num_workers=workers, ops=model.ops) if host else None
        actor = Actor(cfg, model, replay=replay, rank=0, envs=envs)
        try:
            assert (actor.groups is not None) == host
            rs_all, qs_all = [], []
            for _ in range(rollouts):
                data, rs, qs = actor.sample(0.3)
                replay.extend(data)
                rs_all += rs
                qs_all += qs
            n = rollouts * T * E
            outs.append((replay.frames[: n * replay.row_bytes].clone(), replay.act[:n].clone(), replay.rew[:n].clone(), replay.done[:n].clone(), rs_all, qs_all))
        finally:
            actor.close()
    return outs


def _assert_same(outs):
    a, b = outs
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("algo,n_step,workers,groups", [("iqn", 1, 4, 2), ("iqn", 3, 0, 3), ("fqf", 3, 6, 3), ("fqf", 1, 2, 2), ("qr", 3, 3, 3), ("mdqn", 1, 4, 2),
                                                        ("dqn-noisy", 1, 2, 2), ("c51-noisy", 3, 4, 2), ("iqn-noisy", 1, 2, 2), ("iqn-noisy", 3, 3, 3)])
def test_grouped_rollouts_match_the_device_env_for_every_head(algo, n_step, workers, groups, tmp_path):
    """Quantile heads in groups (iqn: the step's E K fraction draws reserved once, group g's rows from its own offset; fqf: fractions from the group's features),
    qr and mdqn, NoisyNet (noise redrawn every 4 steps inside 6-step rollouts: once per step, before any group's inference of that step), n-step 1 and 3, uneven
    groups (8 envs in 3) and in-process stepping.  At 8 envs the quantile heads' fc1 already splits differently over a group's rows than over the batch's."""
    name, noisy = algo.split("-")[0], algo.endswith("-noisy")
    outs = _rollouts(tmp_path, name, 8, groups, workers, n_step, 6, 4, noisy=noisy)
    _assert_same(outs)
    assert float(outs[0][3].sum()) > 0, "the run contains done flags (life losses), so the flag path is exercised"


@pytest.mark.parametrize("algo", ["iqn", "c51", "dqn"])
def test_grouped_rollouts_at_full_size_where_split_counts_differ(algo, tmp_path):
    """256 envs in 2 groups of 128, 12 workers: the split-K count of the actor's GEMMs depends on the row count (iqn's head GEMM over 4 096 vs 8 192 rows, the
    c51 / dqn fc1 over 128 vs 256 rows), so each group runs its GEMMs with the full batch's count — the same sums in the same order as the one-group step."""
    from agent0_amd.deepq.model import layout_from_cfg
    from agent0_amd.ops import HipOps
    ops = HipOps()
    E, k = 256, 128
    L = layout_from_cfg(make_cfg(algo, E, tmp_path))
    if algo == "iqn":
        K = int(make_cfg(algo, E, tmp_path).learner.iqn.K)
        assert ops.dense_fwd_partial_slabs(k * K, L.Npad, 512) != ops.dense_fwd_partial_slabs(E * K, L.Npad, 512)
    elif algo == "c51":
        assert ops.dense_fwd_splits(k, 512, L.feat) != ops.dense_fwd_splits(E, 512, L.feat)
    else:
        assert ops.dense_fwd_partial_slabs(k, 512, L.feat) != ops.dense_fwd_partial_slabs(E, 512, L.feat)
    _assert_same(_rollouts(tmp_path, algo, E, 2, 12, 3, 4, 3, replay_size=4 * E * 3))


@pytest.mark.parametrize("algo,groups,workers", [("dqn", 2, 2), ("iqn", 3, 3), ("c51-noisy", 3, 0)])
def test_grouped_test_rollouts_match_the_device_env(algo, groups, workers, tmp_path):
    """Test rollouts (no replay, ``test=True``: Trainer.test / final) on a grouped env: the newest frame of the first four envs per step — gathered over groups 0 and 1
    when group 0 holds fewer than four envs — and the finished episodes' returns in the order of a one-group rollout."""
    import host_slices
    from agent0_amd.common.env_pool import HostEnvGroups
    from agent0_amd.deepq.agent import Actor
    name, noisy = algo.split("-")[0], algo.endswith("-noisy")
    E, T = 8, 20
    outs = []
    for host in (False, True):
        cfg = make_cfg(name, E, tmp_path, **{"actor.sample_steps": T, "learner.noisy_net": str(noisy).lower(), "learner.reset_noise_freq": 4})
        model = _model(cfg, recipe.NetSpec(name, 4, noisy=noisy))
        # rank 1000: the test actor's (Trainer.test); the device env and the host slices draw from the same rank's streams
        envs = HostEnvGroups(host_slices.synth_slice(cfg.seed, 1000), E, groups=groups, obs_shape=(4, 84, 84), action_dim=4, num_workers=workers, ops=model.ops) if host else None
        actor = Actor(cfg, model, replay=None, rank=1000, envs=envs)
        try:
            frames, rets, qs = [], [], []
            for _ in range(4):
                f, r, q = actor.sample(0.05, test=True)
                frames += f
                rets += r
                qs += q
            outs.append((frames, rets, qs))
        finally:
            actor.close()
    (fa, ra, qa), (fb, rb, qb) = outs
    assert len(fa) == len(fb) == 4 * T and all(x.shape == (4, 1, 84, 84) for x in fb)
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert ra == rb and qa == qb


# ------------------------------------------------------------------------------------------------ Trainer end to end through make_atari
def _host_atari_slice(env_id, episode_life, seed):
    import host_slices
    return host_slices.synth_slice(seed, 0)


@pytest.mark.parametrize("use_lp", [False, True])
@pytest.mark.parametrize("algo,extra", [("iqn", ["replay.policy=prioritize"]), ("c51", ["learner.noisy_net=true", "learner.n_step_q=3"])])
def test_trainer_with_env_groups_equals_one_group(algo, extra, use_lp, tmp_path, monkeypatch):
    """``actor.env_groups=2`` through the public surface: make_atari builds HostEnvGroups (host envs steered to the synthetic slices), the Trainer trains on it
    under both schedules, tests and checkpoints through it — parameters, replay contents, losses, train and test returns bit-equal to ``actor.env_groups=1``."""
    import os
    from agent0_amd.common import atari_wrappers
    from agent0_amd.common.env_pool import HostEnvGroups, HostEnvPool
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setattr(atari_wrappers, "real_atari_available", lambda: True)
    monkeypatch.setattr(atari_wrappers, "AtariSlice", _host_atari_slice)
    res = []
    for groups in (1, 2):
        logdir = tmp_path / f"g{groups}"
        cfg = parse_overrides([f"learner.algo={algo}", "actor.num_envs=16", "actor.sample_steps=12", "learner.batch_size=32", "learner.learner_steps=3", "replay.size=500",
                               "trainer.training_start_steps=100", "learner.target_update_freq=4", "trainer.test_episodes=2", f"actor.env_groups={groups}",
                               "wandb=false", "tb=false", f"logdir={logdir}"] + extra)
        tr = Trainer(cfg, use_lp=use_lp)
        assert isinstance(tr.actors[1].envs, HostEnvGroups if groups == 2 else HostEnvPool)
        out = [tr.run_iteration() for _ in range(6)]
        tr.final()
        assert isinstance(tr.actors[0].envs, HostEnvGroups if groups == 2 else HostEnvPool)
        assert os.path.exists(os.path.join(str(logdir), "final.pth"))
        torch.cuda.synchronize()
        res.append((tr.learner.engine.online.flat.clone(), tr.replay.frames.clone(), tr.replay.act.clone(), tr.replay.rew.clone(), tr.replay.done.clone(),
                    [o["loss"] for o in out], [o["return_train"] for o in out], [o["qmax"] for o in out], list(tr.RTs), tr.frame_count))
    a, b = res
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert a[5:] == b[5:]
    assert a[5][-1] is not None, "updates ran"
