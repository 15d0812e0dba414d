"""GPU (MI355X): an unbound actor (``Actor(cfg, model, replay=None).sample(eps)``) leaves in its staged block the rows a bound actor writes into the ring.

Without a ring the rollout goes step by step (``envs.step``, a0_actor_nstep, five copies into the stage) and, over a grouped host env, through the ``bound=False``
branch of ``Actor._rollout_groups``; bound to a ring the same steps are the merged launches (tail + env step + n-step + replay row).  Same seed, rank and weights:
the same observations, actions, n-step rewards and done flags row for row, the same episode returns and the same per-step mean max-Q.  Shapes: 8 envs, 6 steps,
n-step 1 and 3 (an observation window of 3 that wraps twice per rollout), NoisyNet redrawn every 4 steps, so the first rollout has a reset inside it and the second
starts off one."""
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

E, T, ROLLOUTS, RING = 8, 6, 2, 96
# (algo, dueling, noisy)
HEADS = {"dqn": ("dqn", True, False), "c51-noisy": ("c51", False, True), "iqn": ("iqn", False, False), "fqf": ("fqf", False, False)}


def _actor(head, n_step, logdir, bound, groups=0):
    import host_slices
    from agent0_amd.common.env_pool import HostEnvGroups
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.model import DeepQNet
    from agent0_amd.deepq.replay import ReplayDataset
    algo, dueling, noisy = HEADS[head]
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.num_envs={E}", f"actor.sample_steps={T}", f"learner.n_step_q={n_step}", f"replay.size={RING}",
                           "learner.batch_size=8", f"learner.dueling_head={str(dueling).lower()}", f"learner.noisy_net={str(noisy).lower()}",
                           "learner.reset_noise_freq=4", "wandb=false", "tb=false", f"logdir={logdir}"])
    cfg.obs_shape, cfg.action_dim = (4, 84, 84), 4
    model = DeepQNet(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(recipe.NetSpec(algo, 4, dueling=dueling, noisy=noisy), 11).items()})
    replay = ReplayDataset(cfg, ops=model.ops) if bound else None
    envs = HostEnvGroups(host_slices.synth_slice(cfg.seed, 0), E, groups=groups, obs_shape=(4, 84, 84), action_dim=4, num_workers=0, ops=model.ops) if groups else None
    return Actor(cfg, model, replay=replay, rank=0, envs=envs), replay


_BOUND = {}


def _bound(head, n_step, logdir, use_graph):
    """Per rollout: (obs || obs_next rows, act, rew, done) of the ring rows [start, start + T E), then the returns and the per-step max-Q of both rollouts.
    Computed once per case and shared (the grouped test reads the reference of the first)."""
    key = (head, n_step, use_graph)
    if key not in _BOUND:
        _BOUND[key] = _bound_rollouts(head, n_step, logdir, use_graph)
    return _BOUND[key]


def _bound_rollouts(head, n_step, logdir, use_graph):
    actor, replay = _actor(head, n_step, logdir, bound=True)
    actor.use_graph = use_graph
    try:
        blocks, rs_all, qs_all = [], [], []
        for _ in range(ROLLOUTS):
            start = replay.write_cursor()
            data, rs, qs = actor.sample(0.3)
            replay.extend(data)
            assert start + T * E <= replay.size
            sl = slice(start, start + T * E)
            blocks.append((replay.frames.view(replay.size, replay.row_bytes)[sl].clone(), replay.act[sl].clone(), replay.rew[sl].clone(), replay.done[sl].clone()))
            rs_all += rs
            qs_all += qs
        return blocks, rs_all, qs_all
    finally:
        actor.close()


def _unbound(head, n_step, logdir, groups=0):
    actor, _ = _actor(head, n_step, logdir, bound=False, groups=groups)
    try:
        assert (actor.groups is not None) == bool(groups)
        blocks, rs_all, qs_all = [], [], []
        for _ in range(ROLLOUTS):
            data, rs, qs = actor.sample(0.3)
            st = data.staged
            assert data.count == T * E and st is not None
            blocks.append((torch.cat([st["obs"], st["obs_next"]], dim=1).clone(), st["act"].clone(), st["rew"].clone(), st["done"].clone()))
            rs_all += rs
            qs_all += qs
        return blocks, rs_all, qs_all
    finally:
        actor.close()


def _assert_same(want, got, what):
    (bw, rw, qw), (bg, rg, qg) = want, got
    assert len(bw) == len(bg) == ROLLOUTS
    for r, (x, y) in enumerate(zip(bw, bg)):
        for name, a, b in zip(("obs || obs_next", "act", "rew", "done"), x, y):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, r, name)
            assert torch.equal(a, b), (what, r, name)
    assert rw == rg, what
    assert qw == qg and len(qw) == ROLLOUTS * T, what


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("head", list(HEADS))
def test_unbound_rollout_stages_the_rows_a_bound_rollout_writes(head, n_step, tmp_path):
    """Two consecutive rollouts: the unbound actor's staged block against the ring rows of a bound actor, with ``use_graph`` off and on."""
    got = _unbound(head, n_step, tmp_path)
    assert float(sum(b[3].sum() for b in got[0])) > 0, "the run contains done flags, so the flag path is exercised"
    for use_graph in (False, True):
        _assert_same(_bound(head, n_step, tmp_path, use_graph), got, f"use_graph={use_graph}")


@pytest.mark.parametrize("head", ["dqn", "iqn"])
def test_unbound_grouped_rollout_stages_the_rows_of_the_one_group_bound_rollout(head, tmp_path):
    """The same over a two-group in-process host env (``bound=False`` in Actor._rollout_groups): group g's rows of step t at [t E + off_g, ...) of the stage."""
    _assert_same(_bound(head, 3, tmp_path, False), _unbound(head, 3, tmp_path, groups=2), "two groups")
