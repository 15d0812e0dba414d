"""``Actor`` and the six ``<Algo>Learner`` classes with the reference's names and call signatures, running on the device.

Mirrors /root/reference agent0/deepq/agent.py: ``Actor`` (16-93: ``act``, ``reset``, ``sample``, ``close``),
``BaseLearner`` (96-169: Adam(lr, eps=1e-2/B), ``train`` -> {"q_loss","fraction_loss","indices"}), and
``DQNLearner`` / ``MDQNLearner`` / ``C51Learner`` / ``QRLearner`` / ``IQNLearner`` / ``FQFLearner`` (172-388), which
``Trainer`` resolves by name (trainer.py:31-34).  Differences that follow from keeping everything in HBM:
  * ``Actor.sample`` returns a ``TransitionBlock`` (slots already written into the replay ring) instead of a Python
    list of lz4 blobs; episode returns and per-step mean max-Q come back as Python lists after ONE device->host copy;
  * ``Learner.train`` accepts the reference's 6-tuple of tensors, or — on the hot path — ``train_batch`` takes ring
    slots and never touches the host; losses are returned as device tensors (the reference's ``.cpu()`` copies and its
    ``isnan().any()`` sync are gone, quirk Q14; the NaN-skip itself is kept, on the device).
"""
from __future__ import annotations

import os

from dataclasses import dataclass, replace
from typing import NamedTuple, Optional

import numpy as np
import torch

from agent0_amd.common.atari_wrappers import make_atari
from agent0_amd.common.utils import DeviceRng, pinned_copy
from .config import AlgoEnum, ExpConfig
from .dist import eps_ladder_span, graph_capture_kwargs
from .engine import DeviceLearner, Workspace, risk_value
from .model import DeepQNet, layout_from_cfg
from .replay import ReplayDataset, StageRing, TransitionBlock


def _ops_from(cfg, ops=None):
    if cfg.device.value != "cuda":
        raise RuntimeError("agent0_amd runs on MI355X only: set device=cuda (no CPU fallback; see oracle/ for the CPU restatement used in tests)")
    if ops is None:
        from agent0_amd.ops import HipOps
        ops = HipOps()
    return ops


class _Part:
    """Envs [off, off + E) of the batch with the buffers their steps use: the whole batch (``off`` = 0; the actor's own ``ws``, ``action``, ``ring_*`` and ``out_*``
    are these fields), or one group of a grouped host env with its ``pool``.  ``scratch``: a0_actor_qhead's fc1 slabs (scalar heads); ``slabs``: the head GEMM's
    (every other one-kernel tail); ``ring_obs``: the last observations of an n-step window, where the env does not keep them itself."""

    def __init__(self, actor, off, E, action, scratch, slabs, pool=None):
        ops, n = actor.ops, actor.n
        self.off, self.E, self.action, self.scratch, self.slabs, self.pool = off, E, action, scratch, slabs, pool
        self.ws = Workspace(ops, actor.L, E, actor.n_tau)
        self.ring_act, self.ring_rew, self.ring_done = ops.zeros(n * E, dtype=torch.int32), ops.zeros(n * E), ops.zeros(n * E)
        self.out_act, self.out_rew, self.out_done = ops.zeros(E, dtype=torch.int32), ops.zeros(E), ops.zeros(E)
        self.ring_obs = ops.zeros(actor.ring_len * E * actor.obs_bytes, dtype=torch.uint8) if (n > 1 and not actor.env_history) else None


@dataclass
class _Roll:
    """What the stages of one rollout read (the handle's a0_roll, runtime.hip).  ``sample_async`` fills the first block; ``_roll_begin`` decides the second, and a
    context in which it is left off (``act``, host envs, groups, test rollouts) runs every step on the general launches."""
    epsilon: float                               # actor.eps_ladder: the per-env sentinel, with the vector in ``eps_ptr``
    eps_ptr: Optional[torch.Tensor] = None
    ctrl: Optional[torch.Tensor] = None          # a captured rollout: the device control block, and the device scalar epsilon in ``eps_ptr``
    T: int = 1
    start: int = 0                               # the ring's write cursor when the rollout starts
    bound: bool = False
    test: bool = False
    stage: Optional[dict] = None                 # where an unbound rollout leaves its rows, where a test rollout leaves its frames
    frames_out: Optional[list] = None
    splits: Optional[dict] = None                # a grouped env: the full batch's split-K counts (``_split_plan``); None: every GEMM takes its shape's own
    merged: bool = False                         # tail + env step + n-step bookkeeping + replay row in ONE launch (``act_step_commit``)
    step_enc: bool = False                       # ... which also encodes the env's new observation for step t + 1
    planes: bool = False                         # quantile heads: fc1 reads the term planes of ``refresh_fc1_planes``
    fc1p: bool = False                           # scalar and c51 / qr heads: fc1 reads the planes of ``refresh_actor_fc1_planes``


class Pending(NamedTuple):
    """A rollout that has been issued and not yet collected (``sample_async`` -> ``block_of`` / ``stats_async`` / ``sample_finish``)."""
    T: int
    bound: bool                                  # the rows go straight into the actor's replay (or stage) ring, from ``start`` on
    test: bool
    st: Optional[dict]                           # where an unbound rollout leaves its rows
    start: int
    frames_out: list
    done_ev: torch.cuda.Event                    # recorded behind the rollout's last launch


class Actor:
    def __init__(self, cfg: ExpConfig, model: Optional[DeepQNet] = None, replay: Optional[ReplayDataset] = None, ops=None, rank: int = 0, envs=None):
        self.cfg = cfg
        self.ops = ops = model.ops if model is not None else _ops_from(cfg, ops)
        self.rng = DeviceRng(ops, cfg.seed, rank)
        self.envs = envs if envs is not None else make_atari(cfg.env_id, cfg.actor.num_envs, seed=cfg.seed, rank=rank, ops=ops, task=cfg.env_task,
                                                             groups=int(cfg.actor.env_groups))
        self.obs, _ = self.envs.reset()             # a list of per-group observations for a grouped host env (env_pool.HostEnvGroups)
        self.model = model if model is not None else DeepQNet(cfg, ops=ops)
        self.replay = replay
        self.L = self.model.L
        E = self.E = int(cfg.actor.num_envs)
        self.n = int(cfg.learner.n_step_q)
        self.steps = 0
        self.obs_bytes = self.L.C * self.L.H * self.L.W
        n_tau = self.n_tau = self.L.F if self.L.algo == "fqf" else (cfg.learner.iqn.K if self.L.algo == "iqn" else 1)
        self.taus = ops.empty(E * n_tau) if self.L.algo == "iqn" else None
        # learner.iqn.risk: every evaluation of the policy — training and test rollouts, ``act`` — takes its fractions through the distortion, in the launch that draws
        # them (``_roll_head``) or right behind the draw (``_act_device``); neutral (0): both call what they always called
        self.risk_kind, self.risk_eta = risk_value(cfg.learner.iqn.risk, cfg.learner.iqn.risk_eta, algo=self.L.algo, munchausen=cfg.learner.iqn.munchausen)
        if self.risk_kind and not hasattr(ops, "tau_cos_features_risk"):
            raise ValueError(f"learner.iqn.risk={cfg.learner.iqn.risk}: needs a backend with tau_cos_features_risk")
        self.greedy, self.qmax = ops.zeros(E, dtype=torch.int32), ops.zeros(E)
        T = int(cfg.actor.sample_steps)
        self.qs = ops.zeros(T)
        # scalar heads take the fused tail (fc1 slabs -> q -> dueling -> argmax -> epsilon-greedy in one kernel, a0_actor_qhead)
        self.fused_tail = self.L.algo in ("dqn", "mdqn") and self.L.feat % 4 == 0 and self.L.A + (1 if self.L.dueling else 0) <= 24
        # distributional heads (c51, qr): head GEMM slabs -> one tail kernel (bias, dueling, expectation, argmax, epsilon-greedy)
        self.dist_tail = (not self.fused_tail) and self.L.algo in ("c51", "qr") and 4 * (self.L.A * self.L.T + self.L.T) * 4 <= 160 * 1024
        self._head_slabs = ops.empty(ops.dense_fwd_partial_slabs(E, self.L.Npad, 512) * E * self.L.Npad) if self.dist_tail else None
        # quantile heads (iqn, fqf) on the device env: head GEMM slabs -> one kernel for the tail AND the env step (a0_actor_quantile_tail_env_step)
        self.quant_tail = (self.L.algo in ("iqn", "fqf") and hasattr(self.envs, "act_step_commit") and self.obs_bytes == 4 * 84 * 84
                           and ops.dense_fwd_scratch(E * n_tau, self.L.feat, self.L.num_cosines) == 0)
        # quantile heads without the device env's merged step (host envs, test rollouts): head GEMM slabs -> the same tail without the env step (a0_actor_quantile_tail)
        self.quant_slabs = self.L.algo in ("iqn", "fqf") and ops.dense_fwd_scratch(E * n_tau, self.L.feat, self.L.num_cosines) == 0
        if self.quant_slabs:
            self._head_slabs = ops.empty(ops.dense_fwd_partial_slabs(E * n_tau, self.L.Npad, 512) * E * n_tau * self.L.Npad)
        self.one_tail = self.fused_tail or self.dist_tail or self.quant_slabs      # the head has a one-kernel tail (``_roll_head`` / ``_roll_tail``); else the generic chain
        self.qmax_all = ops.zeros(T * E) if self.one_tail else None
        self._qh_scratch = ops.empty(ops.actor_qhead_scratch(E, self.L.feat)) if self.fused_tail else None
        self.stat_mask, self.stat_ret = ops.zeros(T * E), ops.zeros(T * E)
        # observation ring for n-step: holds the last n observations; its length divides sample_steps when possible so that the
        # slot pattern of a rollout repeats (required for hipGraph replay)
        self.ring_len = next((r for r in range(self.n, 2 * self.n + 1) if T % r == 0), self.n)
        # a device env that keeps its own observation history needs no copy at all: n + 1 (or the next divisor of the rollout length) buffers
        self.env_history = self.n > 1 and hasattr(self.envs, "set_history")
        if self.env_history:
            self.envs.set_history(next((r for r in range(self.n + 1, 2 * self.n + 3) if T % r == 0), self.n + 1))
        # the whole batch as a part; the attribute names the loop, the snapshots and the tests read stay
        p = self.whole = _Part(self, 0, E, ops.zeros(E, dtype=torch.int32), self._qh_scratch, self._head_slabs)
        self.ws, self.action, self.ring_obs = p.ws, p.action, p.ring_obs
        self.ring_act, self.ring_rew, self.ring_done, self.out_act, self.out_rew, self.out_done = p.ring_act, p.ring_rew, p.ring_done, p.out_act, p.out_rew, p.out_done
        self.use_graph = True
        self._graph, self._graph_warm = None, 0
        self.ctrl = ops.zeros(8, dtype=torch.int64)
        self.eps_dev = ops.zeros(1)
        self._ctrl_host = torch.zeros(8, dtype=torch.int64).pin_memory()
        self._eps_host = torch.zeros(1).pin_memory()
        # actor.eps_ladder (Ape-X): a training rollout acts with one epsilon per env, eps^(1 + alpha i / (N - 1)), i and N counted over the whole job; the vector lives
        # beside eps_dev and is allocated by the first rollout that fills it (``_eps_ladder``) — off, or on an actor that only tests, nothing is
        self.rank = int(rank)
        self.ladder_alpha = max(float(cfg.actor.eps_ladder), 0.0)
        # training rollouts of scalar and c51 / qr heads run fc1 as a0_actor_fc1_kernel over weights laid out once per rollout (``_roll_layout_planes``; the library's
        # actor handle likewise, native_loop.py); False keeps the general GEMM in every step — the same bytes, for comparisons.  fc1_launches: steps that took the kernel
        self.fc1_planes = True
        self.fc1_launches = 0
        self.eps_vec = None
        self.atoms = self.model.head.atoms.reshape(-1).contiguous() if self.L.algo == "c51" else None
        self._stage = None
        self._stat_host = {}                         # ``stats_async``: its page-locked buffers
        self._host_actions = None                    # ``_rollout_host``: the action buffer and its alternate
        self.fused_commit = hasattr(self.envs, "step_commit") and (self.obs_bytes == 4 * 84 * 84)
        # scalar heads on the synthetic env: the tail and the env step share one launch (a0_actor_qhead_env_step)
        self.tail_env = (self.fused_tail or self.dist_tail) and self.fused_commit and hasattr(self.envs, "act_step_commit") and os.environ.get("A0_TAIL_ENV", "1") != "0"      # 0: tuning aid (same bytes)
        # a host env split into groups (env_pool.HostEnvGroups): per-group workspaces and n-step state; the CPU steps one group while the GPU infers the other
        self.groups, self._splits = None, None
        if hasattr(self.envs, "pools"):
            if not self.one_tail:
                raise ValueError("a grouped host env needs a head with a one-kernel actor tail (scalar: A + dueling <= 24; c51 / qr: the head's outputs in LDS); use one group")
            sp = self._splits = self._split_plan()
            self.groups = [_Part(self, off, pool.E, self.action[off:off + pool.E], ops.empty(sp["qhead"] * pool.E * 512) if self.fused_tail else None,
                                 None if self.fused_tail else ops.empty(sp["head"] * pool.E * (n_tau if self.quant_slabs else 1) * self.L.Npad), pool)
                           for pool, off in zip(self.envs.pools, self.envs.offsets)]

    def _split_plan(self) -> dict:
        """The split-K counts of the actor step's dense GEMMs at the FULL batch (E rows, E * n_tau for the quantile heads).  A group of k envs runs its GEMMs with
        these counts instead of those of its own k (k * n_tau) rows, so that every row's sum is formed in the order of the one-group step: the split count of
        a0_dense_fwd / a0_dense_fwd_partial / a0_actor_qhead depends on the row count, and a different count is a different association of the fp32 additions."""
        L, ops, dev, E = self.L, self.ops, self.model._dev, self.E
        if self.fused_tail:
            return {"qhead": ops.dense_fwd_partial_slabs(E, 512, L.feat)}          # a0_actor_qhead: a0_fc1_splits(E, 512, K)
        R = E * self.n_tau if self.quant_slabs else E
        plan = {"fc1": dev.dense_splits("fc1", R), "head": ops.dense_fwd_partial_slabs(R, L.Npad, 512)}
        if L.algo == "fqf":
            plan["frac"] = dev.dense_splits("frac", E)
        return plan

    # ------------------------------------------------------------------ the stages of a rollout, named after the actor handle's (a0_roll_*, runtime.hip)
    def _noise_due(self, steps) -> bool:
        """agent.py:52-53: ``self.model.reset_noise()`` every reset_noise_freq steps."""
        return bool(self.cfg.learner.noisy_net) and steps % self.cfg.learner.reset_noise_freq == 0

    def _eps_ladder(self, epsilon, eps_ptr=None):
        """actor.eps_ladder: the rollout's per-env epsilons in one launch (a0_eps_ladder; from the device scalar ``eps_ptr`` inside a captured rollout), and what the
        tails then take in place of ``(epsilon, eps_ptr)``: the per-env sentinel and the vector.  A group passes its envs' slice of it."""
        from agent0_amd.ops import EPS_PER_ENV
        i0, n_total = eps_ladder_span(self.rank, self.E)
        if self.eps_vec is None:
            self.eps_vec = self.ops.zeros(self.E)
        self.ops.eps_ladder(epsilon, eps_ptr, self.ladder_alpha, self.E, i0, n_total, self.eps_vec)
        return EPS_PER_ENV, self.eps_vec

    def _roll_begin(self, roll: _Roll):
        """The epsilons, the composed weights, and which launches the rollout's steps take."""
        cfg, ops, dev, L = self.cfg, self.ops, self.model._dev, self.L
        if self.ladder_alpha > 0 and not roll.test:
            roll.epsilon, roll.eps_ptr = self._eps_ladder(roll.epsilon, roll.eps_ptr)
        if cfg.learner.noisy_net and not self._noise_due(self.steps):
            # NoisyLinear.forward composes mu + sigma * epsilon on every call (model.py:54-62), i.e. with the parameters as they are NOW; the
            # composed copies the device keeps were last written before the learner's latest Adam step (or come from a weight snapshot).
            # A rollout that does not start on a noise reset recomposes them once (with the default sample_steps = 80 it always does).
            dev.compose_noise()
        # a training rollout on the device env: the tail of every one-kernel head shares its launch with the env step
        roll.merged = roll.bound and not roll.test and bool(self.tail_env or (self.quant_tail and self.fused_commit))
        # round 5: that launch of step t also ENCODES the env's new observation (a0_actor_*_env_step_enc) — the next step starts with its features in place, and a
        # scalar-head step is two launches (fc1 GEMM | tail + env step + next encoder) instead of three.  The convolution weights do not change inside a rollout
        # (NoisyNet touches the dense layers only), the last step has no next one.
        fused_84 = dev.fused and (L.C, L.H, L.W) == (4, 84, 84)
        # not on the launch schedule (the rollout into a stage ring): there the rollout runs BESIDE the update block, which is the critical path, and a
        # workgroup that holds a CU's LDS from the tail to the end of the encoder takes more from the block than the saved boundary gives (9.43 -> 9.75 ms)
        launch_schedule = isinstance(self.replay, StageRing)
        roll.step_enc = roll.merged and fused_84 and not launch_schedule
        # quantile actors (round 6): fc1's weight operand as bf16 term planes for the rollout's T GEMMs of E * K rows, split once per rollout and after every noise
        # reset (a0_split_planes; the same exact terms the GEMM forms per tile, hence the same bits)
        roll.planes = roll.merged and self.quant_tail and bool(ops.dense_fwd_wplanes_ok(self.E * self.n_tau, 512, L.feat))
        # scalar and c51 / qr actors: the merged step's fc1 as a0_actor_fc1_kernel over weights laid out likewise (the same slabs bit for bit);
        # ``self.fc1_planes = False`` keeps the general GEMM (comparisons)
        roll.fc1p = roll.merged and self.fc1_planes and self.tail_env and bool(ops.actor_fc1_ok(self.E, 512, L.feat) if self.fused_tail
                                                                                else ops.actor_fc1_dense_ok(self.E, 512, L.feat))

    def _roll_layout_planes(self, roll: _Roll, at_start: bool = True):
        """The laid-out copies of fc1's weights this rollout reads: at its start (unless a noise reset is due there: it lays them out behind its compose), after every reset."""
        if at_start and self._noise_due(self.steps):
            return
        if roll.planes:
            self.model._dev.refresh_fc1_planes()
        if roll.fc1p:
            self.model._dev.refresh_actor_fc1_planes()

    def _roll_noise_reset(self, roll: _Roll, steps):
        """``self.model.reset_noise()`` where step ``steps`` is due one: fresh noise, the composed weights, the laid-out copies of them."""
        if self._noise_due(steps):
            self.model.reset_noise(rng=self.rng)
            self._roll_layout_planes(roll, at_start=False)

    def _roll_draw(self):
        """One step's Philox offsets, claimed ONCE for the whole batch: (seed, the two epsilon-greedy streams, their offsets, the offset of iqn's E * n_tau fractions
        where a one-kernel tail draws them).  The reference draws randint(0, A, E) and then rand(E) (agent.py:29-36): each from its own stream, inside the kernel."""
        rng, E = self.rng, self.E
        sa, su = rng.STREAM_EGREEDY_A, rng.STREAM_EGREEDY_U
        return (rng.seed, sa, su, rng.reserve(sa, E), rng.reserve(su, E), rng.reserve(rng.STREAM_TAUS, E * self.n_tau) if (self.quant_slabs and self.L.algo == "iqn") else 0)

    def _draw_args(self, part: _Part, roll: _Roll, draw, t):
        """What every tail ends in — seed, stream_a, stream_u, off_a, off_u, epsilon, action, qmax, ctrl, eps_ptr — for ``part``: env e's draws lie at the step's
        offsets + e whatever part it is in, its max-Q at row t of ``qmax_all``, its epsilon (actor.eps_ladder) at e of the vector."""
        seed, sa, su, off_a, off_u, _ = draw
        lo, hi = part.off, part.off + part.E
        eps_ptr = roll.eps_ptr if (roll.eps_ptr is None or part.E == self.E) else roll.eps_ptr[lo:hi]
        return (seed, sa, su, off_a + lo, off_u + lo, float(roll.epsilon), part.action, self.qmax_all[t * self.E + lo:t * self.E + hi], roll.ctrl, eps_ptr)

    def _roll_head(self, part: _Part, roll: _Roll, draw):
        """From ``part.ws.act3`` to what the tail reads (a0_roll_head): enqueues the chain and returns the tail's leading arguments.  Scalar heads have no chain (fc1 and
        the head run inside the tail's launches).  c51 / qr: fc1 and the head GEMM's slabs.  Quantile: the fractions — fqf: the fraction net on the part's own features,
        no draws; iqn: the part's rows of the step's draws — with their cosine features in the same launch (round 6), the embedding times the features, fc1 and the
        head GEMM's slabs over E * n_tau rows.  Split counts: ``roll.splits`` (a group: the full batch's) or the shape's own; fc1 from laid-out weights where
        ``roll`` says so."""
        L, ops, dev, rng, ws, k, nt = self.L, self.ops, self.model._dev, self.rng, part.ws, part.E, self.n_tau
        sp = roll.splits or {}
        if self.fused_tail:
            (W1, b1), (W2, b2) = dev.wb("fc1"), dev.wb("head")
            return (ws.act3, k, L.feat, W1, b1, W2, b2, L.A, L.dueling, part.scratch)
        if self.dist_tail:
            if roll.fc1p:      # a0_actor_fc1_dense: the same bits
                ops.actor_fc1_dense(ws.act3, L.feat, dev.actor_fc1_planes, dev.wb("fc1")[1], ws.h, k, 512, L.feat, True, dev.scratch(ops.dense_fwd_scratch(k, 512, L.feat)))
            else:
                dev._dense(ws.act3, L.feat, "fc1", ws.h, k, True, splits=sp.get("fc1"))
            Wh, bh = dev.wb("head")
            ns = ops.dense_fwd_partial_n(ws.h, 512, Wh, k, L.Npad, 512, sp["head"], part.slabs) if sp else ops.dense_fwd_partial(ws.h, 512, Wh, k, L.Npad, 512, part.slabs)
            return (part.slabs, ns, bh, L.Npad, L.A, L.T, L.dueling, 2 if L.algo == "c51" else 1, self.atoms, k)
        if L.algo == "fqf":
            dev.fqf_taus(ws, k, with_cos=True, splits=sp.get("frac"))
            taus, aux, mode = ws.tau_hat, ws.tau_all, 3
        else:
            # env e's n_tau fractions are draws [base + e n_tau, base + (e + 1) n_tau) whatever part it is in; a captured rollout adds ctrl[A0_CTRL_RNG_TAUS]
            if self.risk_kind:      # learner.iqn.risk: the same draws, distorted in the same launch; ws.taus receives tau'
                ops.tau_cos_features_risk(rng.seed, rng.STREAM_TAUS, draw[5] + part.off * nt, ws.taus, ws.cosx, k * nt, L.num_cosines, self.risk_kind, self.risk_eta,
                                          ctrl=rng.ctrl, ctrl_idx=rng.CTRL_INDEX[rng.STREAM_TAUS])
            else:
                ops.tau_cos_features(rng.seed, rng.STREAM_TAUS, draw[5] + part.off * nt, ws.taus, ws.cosx, k * nt, L.num_cosines, ctrl=rng.ctrl, ctrl_idx=rng.CTRL_INDEX[rng.STREAM_TAUS])
            taus, aux, mode = ws.taus, None, 1
        ns = dev.head_slabs(ws, k, taus, nt, part.slabs, cos_ready=True, w_planes=roll.planes, splits=roll.splits)
        _, bh = dev.wb("head")
        return (part.slabs, ns, bh, L.Npad, L.A, nt, L.dueling, mode, aux, k)

    def _roll_tail(self, part: _Part, roll: _Roll, draw, t):
        """The head's chain and its tail without an env step (host envs, groups, test and unbound rollouts, ``act``): one tail launch."""
        ops, head, args = self.ops, self._roll_head(part, roll, draw), self._draw_args(part, roll, draw, t)
        if self.fused_tail and roll.splits is not None:
            ops.actor_qhead_n(*head[:3], roll.splits["qhead"], *head[3:], *args)
        elif self.fused_tail:
            ops.actor_qhead(*head, *args)
        elif self.dist_tail:
            ops.actor_dist_tail(*head, *args)
        else:
            ops.actor_quantile_tail(*head, *args)

    def _act_device(self, part: _Part, obs, roll: _Roll, draw, t: int = 0, qs_slot: Optional[torch.Tensor] = None, tail: bool = True):
        """Actor.act for ``part`` on its observations (agent.py:25-39).  ``tail=False``: the encoder only — the caller runs the tail together with the env step."""
        L, ops, E, dev, ws = self.L, self.ops, self.E, self.model._dev, part.ws
        dev.encode(ws, obs, None, self.obs_bytes, 0, part.E, keep=False)
        if not tail:
            return
        if self.one_tail:
            self._roll_tail(part, roll, draw, t)
            return
        # heads no one-kernel tail accepts (the whole batch only): head with its reduction, first-max selection, the epsilon-greedy draw
        if L.algo == "fqf":
            dev.fqf_taus(ws, E)
            dev.head(ws, E, ws.tau_hat, L.F)
        elif L.algo == "iqn":
            self.rng.uniform(self.rng.STREAM_TAUS, self.taus, E * self.n_tau)
            if self.risk_kind:      # learner.iqn.risk: in place, behind the draw
                ops.risk_distort(self.taus, self.taus, E * self.n_tau, self.risk_kind, self.risk_eta)
            dev.head(ws, E, self.taus, self.n_tau)
        else:
            dev.head(ws, E)
        dev.select(ws, E, self.n_tau, self.greedy, qmax=self.qmax, atoms=self.atoms)
        ops.actor_egreedy_rng(self.greedy, *draw[:5], L.A, float(roll.epsilon), E, part.action, self.qmax, qs_slot, roll.ctrl, roll.eps_ptr)

    def _obs0(self, part: _Part, cur_obs, steps):
        """The first observation of the n-step transition that step ``steps`` emits; where the env keeps no history, ``cur_obs`` first goes into the part's ring."""
        if self.n == 1:
            return cur_obs
        count = min(steps + 1, self.n)
        if self.env_history:
            return self.envs.history(count - 1)
        R, nb = self.ring_len, part.E * self.obs_bytes
        slot, oldest = steps % R, (steps - (count - 1)) % R
        part.ring_obs[slot * nb:(slot + 1) * nb].copy_(cur_obs)
        return part.ring_obs[oldest * nb:(oldest + 1) * nb]

    def _commit_rows(self, part: _Part, roll: _Roll, t, steps, action, obs0, obs_next, reward, terminal, truncated, info):
        """Step ``t``'s rows of ``part`` leave the actor: the n-step window (agent.py:63-81), then the ring's slots [start + t E + off, ...) or the same rows of the stage
        (a test rollout keeps the window and emits nothing)."""
        ops, k, ob = self.ops, part.E, self.obs_bytes
        ops.actor_nstep(k, self.n, steps, float(self.cfg.learner.discount), action, reward, terminal, truncated, info.get("life_loss"),
                        part.ring_act, part.ring_rew, part.ring_done, part.out_act, part.out_rew, part.out_done, roll.ctrl)
        if roll.test:
            return
        row = t * self.E + part.off
        if roll.bound:
            rp = self.replay
            ops.replay_insert(rp.frames, rp.size, ob, (roll.start + row) % rp.size, k, obs0, obs_next, part.out_act, part.out_rew, part.out_done, rp.act, rp.rew, rp.done, roll.ctrl)
        else:
            st, sl = roll.stage, slice(row, row + k)
            st["obs"][sl].copy_(obs0.view(k, -1)); st["obs_next"][sl].copy_(obs_next.view(k, -1))
            st["act"][sl].copy_(part.out_act); st["rew"][sl].copy_(part.out_rew); st["done"][sl].copy_(part.out_done)

    # ------------------------------------------------------------------ agent.py:25-39
    def act(self, epsilon):
        one = self.ops.zeros(1)
        self._act_device(self.whole, self.obs, _Roll(epsilon), self._roll_draw(), qs_slot=one)
        if self.one_tail:
            self.ops.mean_rows(self.qmax_all, 1, self.E, one)
        return self.action.cpu().numpy().astype(np.int64), float(one[0])

    def reset(self):
        self.obs, _ = self.envs.reset()

    # ------------------------------------------------------------------ agent.py:44-90: four loops, each the ORDER in which it issues the stages
    def _rollout(self, roll: _Roll):
        """The body of Actor.sample's loop (agent.py:48-88), every step enqueued on the stream without touching the host."""
        cfg, ops, E, dev, part, rp = self.cfg, self.ops, self.E, self.model._dev, self.whole, self.replay
        T, gamma = roll.T, float(cfg.learner.discount)
        self._roll_begin(roll)
        self._roll_layout_planes(roll)
        feat_ready = False
        for t in range(T):
            self._roll_noise_reset(roll, self.steps)
            draw = self._roll_draw()
            if not feat_ready:
                self._act_device(part, self.obs, roll, draw, t, self.qs[t:t + 1], tail=not roll.merged)
            obs0 = self._obs0(part, self.obs, self.steps)
            mask, ret = self.stat_mask[t * E:(t + 1) * E], self.stat_ret[t * E:(t + 1) * E]
            if roll.merged:
                # the head's chain, then its tail (head, argmax, epsilon-greedy) and the env step + n-step bookkeeping + replay row in ONE launch
                kind = "qhead" if self.fused_tail else ("dist" if self.dist_tail else "quantile")
                targs = self._roll_head(part, roll, draw) + self._draw_args(part, roll, draw, t)
                enc = (dev.wt, dev.encoder_weights(), part.ws.act3) if (roll.step_enc and t + 1 < T) else None
                self.obs = self.envs.act_step_commit(targs, mask, ret, self.n, self.steps, gamma, part.ring_act, part.ring_rew, part.ring_done, obs0, rp,
                                                     (roll.start + t * E) % rp.size, kind=kind, enc=enc,
                                                     w1_planes=dev.actor_fc1_planes if (roll.fc1p and kind == "qhead") else None)
                self.fc1_launches += 1 if roll.fc1p else 0
                feat_ready = enc is not None
                self.steps += 1
                continue
            if roll.bound and not roll.test and self.fused_commit:
                # env step, n-step bookkeeping and the replay row in one launch (synthetic env)
                self.obs = self.envs.step_commit(part.action, mask, ret, self.n, self.steps, gamma, part.ring_act, part.ring_rew, part.ring_done, obs0, rp,
                                                 (roll.start + t * E) % rp.size, roll.ctrl)
                self.steps += 1
                continue
            obs_next, reward, terminal, truncated, info = self.envs.step(part.action, final_mask=mask, final_ret=ret, ctrl=roll.ctrl)
            self._commit_rows(part, roll, t, self.steps, part.action, obs0, obs_next, reward, terminal, truncated, info)
            self.steps += 1
            if roll.test:
                roll.frames_out.append(obs_next.view(E, self.L.C, self.L.H, self.L.W)[:4, -1:].cpu().numpy())
            self.obs = obs_next
        if self.one_tail:
            ops.mean_rows(self.qmax_all, T, E, self.qs)          # per-step mean max-Q (agent.py:38,88), all steps at once

    # ------------------------------------------------------------------ host envs (env_pool.HostEnvPool): nothing but inference between two env steps
    def _rollout_host(self, roll: _Roll):
        """Actor.sample's loop (agent.py:48-88) over a host env that takes its actions without waiting (``step_send`` / ``step_recv``).  What lies between "the
        workers have finished step t" and "the workers see the actions of step t + 1" is the upload and Actor.act alone: the bookkeeping of step t (n-step window,
        replay row, episode statistics: agent.py:63-88) is enqueued AFTER the actions of step t + 1 have been sent and runs while the workers step.  Same kernels on
        the same inputs in an order that respects every dependency — the bytes of ``_rollout`` (tests/test_gpu_trainer.py::test_host_env_pool_matches_device_env);
        the action buffer alternates between two tensors because step t's n-step update reads its actions after step t + 1's have been chosen."""
        ops, E, part = self.ops, self.E, self.whole
        if self._host_actions is None:
            self._host_actions = (self.action, ops.zeros(E, dtype=torch.int32))

        def bookkeeping(t, steps, action, cur_obs, obs_next, reward, terminal, truncated, info):
            sl = slice(t * E, (t + 1) * E)
            self.stat_mask[sl].copy_(info["final_mask"], non_blocking=True)
            self.stat_ret[sl].copy_(info["final_ret"], non_blocking=True)
            self._commit_rows(part, roll, t, steps, action, self._obs0(part, cur_obs, steps), obs_next, reward, terminal, truncated, info)

        self._roll_begin(roll)
        pending = None
        for t in range(roll.T):
            self._roll_noise_reset(roll, self.steps)
            part.action = self._host_actions[t & 1]
            self._act_device(part, self.obs, roll, self._roll_draw(), t, self.qs[t:t + 1])
            self.envs.step_send(part.action)
            if pending is not None:
                bookkeeping(*pending)
            obs_next, reward, terminal, truncated, info = self.envs.step_recv()
            pending = (t, self.steps, part.action, self.obs, obs_next, reward, terminal, truncated, info)
            self.steps += 1
            self.obs = obs_next
        bookkeeping(*pending)
        part.action = self._host_actions[0]
        if self.one_tail:
            ops.mean_rows(self.qmax_all, roll.T, E, self.qs)

    # ------------------------------------------------------------------ grouped host envs: CPU stepping of one group beside the GPU's inference of the other
    def _rollout_groups(self, roll: _Roll):
        """Actor.sample's loop (agent.py:48-88) over a grouped host env: while group A's worker processes step their envs, the GPU runs Actor.act for group B,
        and vice versa (the overlap the reference gets from ``num_actors`` actor processes, launch.py:30-61).  Every env sees exactly what it would see in
        a one-group rollout — its own observations, the epsilon-greedy (and iqn fraction) draws at its own offset of the step's Philox block, its own n-step window,
        the same NoisyNet noise — and group g's transitions of step t land in the ring slots [start + t E + off_g, ...): the same bytes in the same order
        (tests/test_gpu_trainer.py, tests/test_gpu_host_env_groups.py).  ``roll.test``: no n-step bookkeeping and no rows, the first four envs' newest frames per step
        into ``roll.frames_out``; unbound (and not a test): the rows go to ``roll.stage`` at the same positions.  A step's Philox offsets are claimed once for the
        whole batch and every group takes its envs' part of each; every dense GEMM runs with the full batch's split count (``roll.splits``)."""
        E, T = self.E, roll.T

        def infer_send(g, obs, draw, t):                          # Actor.act for group g, then its actions go to its workers without waiting for them
            self._act_device(g, obs, roll, draw, t)
            g.pool.step_send(g.action)

        self._roll_begin(roll)
        self._roll_noise_reset(roll, self.steps)                  # step 0's noise, ahead of its first inference
        draw = self._roll_draw()
        for gi, g in enumerate(self.groups):                      # step 0's actions: nothing to overlap with yet
            infer_send(g, self.obs[gi], draw, 0)
        for t in range(T):
            nxt_draw = self._roll_draw() if t + 1 < T else None
            frames = []
            for gi, g in enumerate(self.groups):
                k, off = g.E, g.off
                cur_obs = self.obs[gi]
                sl = slice(t * E + off, t * E + off + k)
                obs_next, reward, terminal, truncated, info = g.pool.step_recv(self.stat_mask[sl], self.stat_ret[sl])      # waits for THIS group's workers only
                if not roll.test:
                    self._commit_rows(g, roll, t, self.steps, g.action, self._obs0(g, cur_obs, self.steps), obs_next, reward, terminal, truncated, info)
                elif off < 4:                                       # the newest frame of the first four envs (agent.py / trainer.py:131-132), gathered over the groups
                    frames.append(obs_next.view(k, self.L.C, self.L.H, self.L.W)[:4 - off, -1:].cpu().numpy())
                self.obs[gi] = obs_next
                if nxt_draw is not None:                            # the next step's actions for this group, while the other group's workers are stepping
                    if gi == 0:
                        # NoisyNet: the next step's noise, once, behind every group's inference of this step and ahead of any of the next
                        self._roll_noise_reset(roll, self.steps + 1)
                    infer_send(g, obs_next, nxt_draw, t + 1)
            if roll.test:
                roll.frames_out.append(np.concatenate(frames, axis=0))
            self.steps += 1
        self.ops.mean_rows(self.qmax_all, T, E, self.qs)

    def _graph_eligible(self, T, bound, test, state_dict) -> bool:
        cfg = self.cfg
        return (self.use_graph and bound and not test and state_dict is None and hasattr(self.envs, "_cur") and T % len(self.envs._obs) == 0
                and (not cfg.learner.noisy_net or T % cfg.learner.reset_noise_freq == 0) and (self.n == 1 or self.env_history or T % self.ring_len == 0))

    def _snapshot(self):
        rng = self.rng
        return {"g": self.envs.g, "steps": self.steps, "slot": self.replay.write_cursor(), "rng": dict(rng.offsets), "cur": self.envs._cur}

    def _rollout_graphed(self, roll: _Roll):
        """One hipGraph launch per rollout: the 80 x ~10 launches are captured once; counters that keep advancing (env step, n-step
        index, Philox offsets, replay cursor) reach the kernels through a device control block, epsilon through a device scalar."""
        rng, rp, epsilon, T, start = self.rng, self.replay, roll.epsilon, roll.T, roll.start
        if self._graph is None:
            if self._graph_warm < 2:                     # eager first: lazy allocations (workspaces, scratch) happen here
                self._graph_warm += 1
                self._rollout(roll)
                return
            self._ctrl_host.zero_(); self.ctrl.zero_(); self._eps_host[0] = float(epsilon); self.eps_dev.copy_(self._eps_host)
            rng.ctrl = self.ctrl
            base = self._snapshot()
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, **graph_capture_kwargs()):
                self._rollout(replace(roll, ctrl=self.ctrl, eps_ptr=self.eps_dev))
            rng.ctrl = None                              # the captured kernels hold the pointer; eager rollouts must not add stale deltas
            after = self._snapshot()
            assert after["cur"] == base["cur"]
            self._graph = (graph, base, {k: after["rng"].get(k, 0) - base["rng"].get(k, 0) for k in after["rng"]})
            graph.replay()                               # capture only records; this is the rollout itself
            return
        graph, base, rng_adv = self._graph
        assert self.envs._cur == base["cur"]
        h = self._ctrl_host
        h[0] = self.envs.g - base["g"]
        h[1] = self.steps - base["steps"]
        h[2] = rng.offsets.get(rng.STREAM_EGREEDY_A, 0) - base["rng"].get(rng.STREAM_EGREEDY_A, 0)
        h[3] = rng.offsets.get(rng.STREAM_EGREEDY_U, 0) - base["rng"].get(rng.STREAM_EGREEDY_U, 0)
        h[4] = (start - base["slot"]) % rp.size
        h[5] = rng.offsets.get(rng.STREAM_TAUS, 0) - base["rng"].get(rng.STREAM_TAUS, 0)
        h[6] = rng.offsets.get(rng.STREAM_NOISE, 0) - base["rng"].get(rng.STREAM_NOISE, 0)
        self._eps_host[0] = float(epsilon)
        self.ctrl.copy_(h, non_blocking=True)
        self.eps_dev.copy_(self._eps_host, non_blocking=True)
        graph.replay()
        self.envs.g += T
        self.steps += T
        for k, v in rng_adv.items():
            rng.offsets[k] = rng.offsets.get(k, 0) + v

    def sample(self, epsilon, state_dict=None, test: bool = False):
        return self.sample_finish(self.sample_async(epsilon, state_dict, test))

    def sample_async(self, epsilon, state_dict=None, test: bool = False):
        """Enqueue one rollout on the current stream and return without waiting for it (the device counterpart of
        ``actor.futures.sample(...)``, launch.py:34-36); ``sample_finish`` collects the result."""
        cfg, ops, E = self.cfg, self.ops, self.E
        if isinstance(state_dict, DeepQNet):
            self.model._dev.copy_from(state_dict._dev)          # device-to-device weight snapshot
            state_dict = None
        elif state_dict is not None:
            self.model.load_state_dict(state_dict)
        T = int(cfg.actor.sample_steps)
        bound = self.replay is not None and not test
        st = None
        if not bound and not test:
            st = self._stage
            if st is None or st["obs"].shape[0] != T * E:
                st = self._stage = {"obs": ops.zeros(T * E, self.obs_bytes, dtype=torch.uint8), "obs_next": ops.zeros(T * E, self.obs_bytes, dtype=torch.uint8),
                                    "act": ops.zeros(T * E, dtype=torch.int32), "rew": ops.zeros(T * E), "done": ops.zeros(T * E)}
        start = self.replay.write_cursor() if bound else 0
        frames_out = []
        roll = _Roll(epsilon, T=T, start=start, bound=bound, test=test, stage=st, frames_out=frames_out, splits=self._splits)
        if self.groups is not None:
            self._rollout_groups(roll)
        elif self._graph_eligible(T, bound, test, state_dict):
            self._rollout_graphed(roll)
        elif bound and hasattr(self.envs, "step_send") and os.environ.get("A0_HOST_ROLLOUT", "1") != "0":      # 0: the step-by-step order of _rollout (same bytes; a tuning aid)
            self._rollout_host(roll)
        else:
            self._rollout(roll)
        done_ev = torch.cuda.Event()
        done_ev.record()
        return Pending(T, bound, test, st, start, frames_out, done_ev)

    def block_of(self, pending) -> TransitionBlock:
        """The TransitionBlock of a rollout that has been issued (``sample_async``) but not necessarily finished: what ``replay.extend`` needs is
        known on the host from the start (row count, ring position); the rows themselves are ordered before any later kernel on the stream."""
        T, bound, test, st, start, frames_out, done_ev = pending
        if test:
            raise ValueError("a test rollout produces frames, not transitions")
        if bound:
            return TransitionBlock(T * self.E, start=start, source=self.replay if isinstance(self.replay, StageRing) else None)
        return TransitionBlock(T * self.E, staged=st)

    def sample_finish(self, pending):
        T, bound, test, st, start, frames_out, done_ev = pending
        E = self.E
        done_ev.synchronize()
        # one device->host copy per rollout: mean max-Q per step and finished-episode returns, in the reference's order
        qs = self.qs[:T].cpu().tolist()
        mask = self.stat_mask[:T * E].cpu().numpy() != 0
        rs = self.stat_ret[:T * E].cpu().numpy()[mask].tolist()
        if test:
            return frames_out, rs, qs
        return self.block_of(pending), rs, qs

    def stats_async(self, pending):
        """The statistics of an issued rollout on their way to page-locked host buffers, stream-ordered behind it (and ahead of the next rollout, which reuses the
        device buffers); ``stats_finish`` waits for exactly these copies, not for whatever was enqueued afterwards."""
        T = pending.T
        n = T * self.E
        out = [pinned_copy(self._stat_host, name, src) for name, src in (("qs", self.qs[:T]), ("mask", self.stat_mask[:n]), ("ret", self.stat_ret[:n]))]
        ev = torch.cuda.Event()
        ev.record()
        return (ev, out)

    def stats_finish(self, handle):
        """(returns, per-step mean max-Q) as ``sample_finish`` reports them."""
        ev, (qs, mask, ret) = handle
        ev.synchronize()
        return ret.numpy()[mask.numpy() != 0].tolist(), qs.tolist()

    # ------------------------------------------------------------------ resumable snapshots (deepq/snapshot.py)
    def _state_desc(self) -> dict:
        cfg = self.cfg
        return {"E": self.E, "T": int(cfg.actor.sample_steps), "A": int(self.L.A), "dueling": int(bool(self.L.dueling)), "n_step": self.n,
                "env_task": int(getattr(self.envs, "task", 0)), "reset_noise_freq": int(cfg.learner.reset_noise_freq), "discount": float(cfg.learner.discount),
                "K": len(getattr(self.envs, "_obs", ()))}

    def state_dict(self) -> dict:
        """What the next rollout reads that earlier rollouts wrote, in the fields of the actor handle's state blob (a0_actor_state_save): step counter, Philox seed and
        offsets, the device env's state, the n-step windows and the last rollout's statistics.  Device-resident env only: the emulators of a host env live in worker
        processes and cannot be saved — a resumed run resets them and starts with empty n-step windows."""
        if not hasattr(self.envs, "state_dict"):
            raise RuntimeError("Actor.state_dict: host environments cannot be saved")
        env, T = self.envs.state_dict(), int(self.cfg.actor.sample_steps)
        d = self._state_desc()
        d.update(cur=env["cur"], g=env["g"], steps=int(self.steps), rng_seed=int(self.rng.seed), rng_off=[int(self.rng.offsets.get(i, 0)) for i in range(8)],
                 env_seed=env["seed"], rank=env["rank"], obs=env["obs"].numpy(), ep_ret=env["ep_ret"].numpy(), ring_act=self.ring_act.cpu().numpy(),
                 ring_rew=self.ring_rew.cpu().numpy(), ring_done=self.ring_done.cpu().numpy(), qs=self.qs[:T].cpu().numpy(),
                 stat_mask=self.stat_mask[:T * self.E].cpu().numpy(), stat_ret=self.stat_ret[:T * self.E].cpu().numpy())
        return d

    def load_state_dict(self, d: dict):
        from .snapshot import check_actor_desc
        check_actor_desc(d, self._state_desc())
        E, T, K = self.E, int(self.cfg.actor.sample_steps), d["K"]
        self.envs.load_state_dict({"g": d["g"], "cur": d["cur"], "seed": d["env_seed"], "rank": d["rank"], "obs": torch.from_numpy(np.asarray(d["obs"])).reshape(K, -1),
                                   "ep_ret": torch.from_numpy(np.asarray(d["ep_ret"]))})
        self.obs = self.envs.obs
        self.steps = int(d["steps"])
        self.rng.seed = int(d["rng_seed"])
        self.rng.offsets = {i: int(o) for i, o in enumerate(d["rng_off"]) if o}
        dev = self.ops.device
        for name in ("ring_act", "ring_rew", "ring_done"):
            getattr(self, name).copy_(torch.from_numpy(np.asarray(d[name])).to(dev))
        self.qs[:T].copy_(torch.from_numpy(np.asarray(d["qs"])).to(dev))
        self.stat_mask[:T * E].copy_(torch.from_numpy(np.asarray(d["stat_mask"])).to(dev))
        self.stat_ret[:T * E].copy_(torch.from_numpy(np.asarray(d["stat_ret"])).to(dev))
        self._graph, self._graph_warm = None, 0          # a captured rollout holds the counters it was captured at

    def pending_from(self, start: int):
        """The handle of a rollout that had been issued ahead when the snapshot was taken and whose rows and statistics the loaded state holds."""
        ev = torch.cuda.Event()
        ev.record()
        return Pending(int(self.cfg.actor.sample_steps), True, False, None, int(start), [], ev)

    def close(self):
        self.envs.close()


class BaseLearner:
    def __init__(self, cfg: ExpConfig, ops=None):
        self.cfg = cfg
        self.ops = ops = _ops_from(cfg, ops)
        lc = cfg.learner
        L = layout_from_cfg(cfg)
        self.rng = DeviceRng(ops, cfg.seed + 15485863)      # ahead of the engine: learner.aug_shift draws its shifts from this seed (the object, so that a loaded snapshot's seed is followed)
        self.engine = DeviceLearner(ops, L, int(lc.batch_size), discount=lc.discount, n_step=lc.n_step_q, double_q=lc.double_q, lr=lc.learning_rate,
                                    target_update_freq=lc.target_update_freq, vmin=lc.c51.vmin, vmax=lc.c51.vmax, K=lc.iqn.K, N=lc.iqn.N, N_dash=lc.iqn.N_dash,
                                    max_grad_norm=lc.max_grad_norm, mdqn_tau=lc.mdqn.tau, mdqn_lo=lc.mdqn.lo, clip_grad_norm=lc.clip_grad_norm, target_tau=lc.target_tau,
                                    aug_shift=lc.aug_shift, aug_rng=self.rng, net_reset_freq=lc.net_reset_freq, net_reset_shrink=lc.net_reset_shrink,
                                    weight_decay=lc.weight_decay, redo_freq=lc.redo_freq, redo_tau=lc.redo_tau, redo_recycle=lc.redo_recycle,
                                    rank_freq=lc.rank_freq, rank_delta=lc.rank_delta, munchausen=lc.iqn.munchausen, mdqn_alpha=lc.mdqn.alpha,
                                    hl_gauss=lc.c51.hl_gauss, risk=lc.iqn.risk, risk_eta=lc.iqn.risk_eta)
        self.model = DeepQNet(cfg, ops=ops, dev_net=self.engine.online, rng=self.rng)
        self.model_target = DeepQNet(cfg, ops=ops, dev_net=self.engine.target, rng=self.rng)
        self.engine.sync_target(force=True)                 # model_target = deepcopy(model), agent.py:100
        self.batch_indices = torch.arange(lc.batch_size, device=ops.device)
        self.optimizer = self.engine                        # Adam state lives in the engine's flat buffers
        B = int(lc.batch_size)
        self._taus = [ops.empty(B * n) for n in (lc.iqn.K, lc.iqn.N_dash, lc.iqn.N)] if L.algo == "iqn" else None
        self._ones = torch.ones(B, device=ops.device)
        self.use_graph = True
        self._graphs, self._graph_warm = {}, {}
        # updates issued through this learner (eager or replayed): the device keeps the same count in state[6] and files each update's mean loss under it
        # (DeviceLearner.loss_ring), so the Trainer can read a block's means back in one copy
        self.updates_issued = 0

    @property
    def update_steps(self) -> int:
        return int(self.engine.state[1])

    # ------------------------------------------------------------------ hot path: batch addressed by ring slots
    def target_stage_batch(self, frames: torch.Tensor, slot: torch.Tensor, row_bytes: int, parity: int):
        """The target network's pass of the update that will consume this batch (``train_batch(..., tstage=parity)``), enqueued on the CURRENT stream —
        the Trainer's pipelined update block calls it on a second stream while the previous update is in flight.  Replayed from a hipGraph per parity."""
        eng = self.engine
        if not self.use_graph:
            return eng.target_stage(frames, slot, row_bytes, parity)
        key = ("tstage", frames.data_ptr(), slot.data_ptr(), row_bytes, parity)
        g = self._graphs.get(key)
        if g is None:
            if self._graph_warm.get(key, 0) < 2:
                self._graph_warm[key] = self._graph_warm.get(key, 0) + 1
                return eng.target_stage(frames, slot, row_bytes, parity)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, **graph_capture_kwargs()):
                eng.target_stage(frames, slot, row_bytes, parity)
            self._graphs[key] = g
        g.replay()

    def train_batch(self, frames: torch.Tensor, slot: Optional[torch.Tensor], row_bytes: int, act, rew, done, weights, rand=None, tstage=None):
        """``rand`` (parity tests): the update's random / proposed fractions handed in instead of drawn here — see DeviceLearner.forward_dense;
        the tensors must be persistent device buffers (the update is replayed from a hipGraph that holds their addresses)."""
        cfg = self.cfg
        if cfg.learner.noisy_net:
            eng = self.engine
            if eng.noise_joint is not None:
                # the two resets of agent.py:125-127 (online, then target) as ONE fill of the joint buffer: the same Philox draws as two fills
                self.rng.normal(self.rng.STREAM_NOISE, 0.1, eng.noise_joint, eng.noise_joint.numel())
            else:
                self.model.reset_noise(compose=False)            # DeviceLearner.forward_dense composes both nets' effective weights
                self.model_target.reset_noise(compose=False)
        if rand is None and self._taus is not None:
            for t in self._taus:
                self.rng.uniform(self.rng.STREAM_TAUS, t, t.numel())
            rand = self._taus
        out = self._update(frames, slot, row_bytes, act, rew, done, weights, rand, tstage)
        return out if isinstance(out, tuple) else (out, None)

    def _update(self, frames, slot, row_bytes, act, rew, done, weights, rand, tstage=None):
        """engine.update, replayed from hipGraphs when the caller keeps handing in the same device buffers (the Trainer's hot loop
        does: the replay's persistent batch tensors).  The whole update is ONE graph — under data parallelism too: the gradient exchange
        (dist.RcclGradAllReduce -> a0_dp_allreduce) is a stream-ordered launch like any other and is captured with it, the dense bucket's
        all-reduce as a parallel branch beside the encoder backward.  Only a hook that must run on the host (a plain callable, or the
        torch.distributed fallback) splits the update into three graphs — forward + dense backward | encoder backward | optimizer step —
        around its eager calls."""
        eng = self.engine
        self.updates_issued += 1
        if not self.use_graph:
            return eng.update(frames, slot, row_bytes, act, rew, done, weights, rand=rand, tstage=tstage)
        hooked = eng.grad_hook is not None and not getattr(eng.grad_hook, "in_graph", False)
        key = (frames.data_ptr(), None if slot is None else slot.data_ptr(), row_bytes, act.data_ptr(), rew.data_ptr(), done.data_ptr(), weights.data_ptr(), hooked, tstage)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 8 or self._graph_warm.get(key, 0) < 2:       # two eager runs first: every lazy allocation has happened
                self._graph_warm[key] = self._graph_warm.get(key, 0) + 1
                return eng.update(frames, slot, row_bytes, act, rew, done, weights, rand=rand, tstage=tstage)
            mode = graph_capture_kwargs()
            g_f, g_e, g_apply = torch.cuda.CUDAGraph(), (torch.cuda.CUDAGraph() if hooked else None), (torch.cuda.CUDAGraph() if hooked else None)
            torch.cuda.synchronize()
            try:
                with torch.cuda.graph(g_f, **mode):
                    out = eng.forward_dense(frames, slot, row_bytes, act, rew, done, weights, rand, tstage=tstage)
                    if not hooked:                                # the whole update is one graph, in-graph exchange included
                        eng.exchange_begin()
                        eng.backward_encoder(fuse_tail=True)
                        eng.exchange_end()
                        eng.apply()
            except Exception as e:      # noqa: BLE001
                if eng.grad_hook is None or hooked:
                    raise
                # an RCCL build that cannot be captured: keep the same exchange, issued eagerly between three graphs from now on
                import sys
                print(f"agent0_amd: capturing the gradient exchange into the update's hipGraph failed ({e}); splitting the update around it", file=sys.stderr)
                eng.grad_hook.in_graph = False
                torch.cuda.synchronize()
                return eng.update(frames, slot, row_bytes, act, rew, done, weights, rand=rand, tstage=tstage)
            if hooked:
                with torch.cuda.graph(g_e, **mode):
                    eng.backward_encoder()
                with torch.cuda.graph(g_apply, **mode):
                    eng.apply()
            g = self._graphs[key] = (g_f, g_e, g_apply, out)      # capturing records the launches without running them
        g[0].replay()
        if g[1] is not None:
            eng.exchange_begin()
            g[1].replay()
            eng.exchange_end()
            g[2].replay()
        return g[3]

    # ------------------------------------------------------------------ reference signature (agent.py:124-169)
    def train(self, data):
        frames, actions, rewards, terminals, weights, indices = data
        dev = self.ops.device
        B = frames.shape[0]
        u8 = frames.to(dev)
        u8 = (u8 if u8.dtype == torch.uint8 else u8.round().clamp_(0, 255).to(torch.uint8)).reshape(-1).contiguous()
        q_loss, f_loss = self.train_batch(u8, None, u8.numel() // B, actions.to(dev).to(torch.int32).contiguous(), rewards.to(dev).float().contiguous(),
                                          terminals.to(dev).float().contiguous(), weights.to(dev).float().contiguous())
        skipped = bool(self.engine.state[3])
        # CPU copies, like the reference's `.detach().cpu()` (agent.py:163-169); the Trainer's hot loop uses train_batch and stays on the device
        return {"q_loss": None if skipped else q_loss[:B].cpu(), "fraction_loss": None if f_loss is None else f_loss[:B].cpu(),
                "indices": indices.long().cpu()}


class DQNLearner(BaseLearner):
    pass


class MDQNLearner(BaseLearner):
    pass


class C51Learner(BaseLearner):
    pass


class QRLearner(BaseLearner):
    pass


class IQNLearner(BaseLearner):
    pass


class FQFLearner(BaseLearner):
    pass
