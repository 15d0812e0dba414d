"""``Trainer``: the reference's orchestration loop, unchanged in shape, with every tensor resident in HBM.

Mirrors /root/reference agent0/deepq/trainer.py:19-189 — ``Trainer(cfg, use_lp=False)`` with ``run``, ``step``,
``test``, ``logging``, ``final``, the epsilon schedule (46-50, eps(0) = 1 + min_eps as in the reference) and the result
keys (111-118): frames, fraction_loss, loss, return_train, return_train_max, qmax, fps.
Per iteration: ``actors[1].sample(eps)`` rolls ``sample_steps`` env steps and writes the transitions straight into the
replay ring; ``step`` commits them and runs ``learner_steps`` updates (sample -> importance weights -> train ->
priority update), all enqueued on one HIP stream with a single device->host read at the end for the loss means.
wandb / tensorboard are used only if importable and enabled (neither ships in this image).
"""
from __future__ import annotations

import logging
import math
import os
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import agent as agents
from .config import ExpConfig, ReplayEnum, to_dict
from .layout import NetLayout
from .replay import ReplayDataset, StageRing
from agent0_amd.common.atari_wrappers import make_atari
from agent0_amd.common.utils import pinned_copy, set_random_seed


def _git_sha() -> str:
    from .main import _git_sha as sha
    return sha()


PROGRESS_COLUMNS = ("frames", "fraction_loss", "loss", "return_train", "return_train_max", "qmax", "fps")      # trainer.py:111-118 + fps (180-181)
REDO_LAYERS, REDO_NEURONS = NetLayout.REDO_LAYERS, 672      # learner.redo_freq: (block, first neuron, neurons) of the hidden layers
REDO_COLUMNS = ("dormant_frac",) + tuple(f"dormant_frac_{name}" for name, _, _ in REDO_LAYERS)


def epsilon_schedule(cfg: ExpConfig):
    def fn(step):
        if step > cfg.trainer.exploration_steps:
            return cfg.actor.min_eps
        return (1.0 - step / cfg.trainer.exploration_steps) + cfg.actor.min_eps
    return fn


@dataclass
class _BlockStats:
    """What one update block leaves for the host (after the learner's ``_Upd`` and the actor's ``_Roll``).  ``_block`` opens it with the slots the block's statistics
    will lie in and counts its updates; ``Trainer._stats`` fills the host tensors — page-locked copies in flight, or ``.cpu()`` reads; ``finish`` books them once the
    host has waited for them.  The slot counts are update counts: a ring's slot is the count modulo its length."""
    n_upd: int = 0
    ring0: Optional[int] = None                  # the block's first slot in DeviceLearner.loss_ring; None: a0_mean_rows filled ``loss`` from index 0
    gn0: Optional[int] = None                    # learner.clip_grad_norm: the block's first slot in DeviceLearner.gnorm_ring; None: off
    has_frac: bool = False                       # fqf: the block left fraction-loss means
    state: Optional[torch.Tensor] = None         # the unfused optimizer tail does not advance the slot counter: the status words, [6] = the slot of the block's last norm
    loss: Optional[torch.Tensor] = None          # the host tensors; absent ones stay None
    floss: Optional[torch.Tensor] = None
    gnorm: Optional[torch.Tensor] = None
    wd_partials: Optional[torch.Tensor] = None

    def finish(self, tr):
        """Extends ``tr.Ls`` / ``tr.FLs``, sets ``tr.GNs`` (the block's norms, its newest ring-length ones when it is longer than the ring) and ``tr.PN`` (learner.weight_decay:
        the decay launch leaves one double per workgroup, a0_weight_decay; the norm is finished here — the sum in index order, the square root in double)."""
        n = self.n_upd
        if not n:
            return
        if self.ring0 is None:
            tr.Ls.extend(self.loss[:n].tolist())
        else:
            tr.Ls.extend(float(self.loss[(self.ring0 + i) % self.loss.numel()]) for i in range(n))
        if self.floss is not None:
            tr.FLs.extend(self.floss[:n].tolist())
        if self.gnorm is not None:
            cap = self.gnorm.numel()
            k = min(n, cap)
            tr.GNs = [float(self.gnorm[(self.gn0 + n - k + i) % cap]) for i in range(k)] if self.state is None else [float(self.gnorm[int(self.state[6]) % cap])]
        if self.wd_partials is not None:
            total = 0.0
            for x in self.wd_partials.tolist():
                total += x
            tr.PN = math.sqrt(total)


class Trainer:
    def __init__(self, cfg: ExpConfig, use_lp: bool = False, ops=None, rank: int = 0, primary: bool = True):
        """``primary=False`` (data-parallel replicas other than rank 0, launch.py here): no run directory, msg.log, tensorboard / wandb, final
        checkpoint or final test — the replicas are identical, so rank 0 reports for all of them."""
        self.cfg, self.use_lp, self.rank, self.primary = cfg, use_lp, rank, primary
        set_random_seed(cfg.seed)
        if cfg.device.value != "cuda":
            raise RuntimeError("agent0_amd runs on MI355X only: set device=cuda (no CPU fallback)")
        if ops is None:
            from agent0_amd.ops import HipOps
            ops = HipOps()
        self.ops = ops
        if ops.trace_enabled() and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ops.trace_rank(rank)                          # roctx ranges carry the rank ("r3:exchange") in a data-parallel job
        dummy_env = make_atari(cfg.env_id, 1, ops=ops)
        self.obs_shape = tuple(dummy_env.observation_space.shape[1:])
        self.act_dim = int(dummy_env.action_space[0].n)
        dummy_env.close()
        if not cfg.obs_shape or len(tuple(cfg.obs_shape)) != 3:
            cfg.obs_shape = self.obs_shape
        if not cfg.action_dim:
            cfg.action_dim = self.act_dim
        try:
            learner_cls = getattr(agents, f"{cfg.learner.algo.name.upper()}Learner")
        except AttributeError:
            raise NotImplementedError(f"No such learner for {cfg.learner.algo.name}")
        self.learner = learner_cls(cfg, ops=ops)
        self.replay = ReplayDataset(cfg, ops=ops)
        if not use_lp:
            # the reference builds a test actor [0] and a train actor [1] sharing the learner's model (trainer.py:41-44)
            self.actors = [None, agents.Actor(cfg, self.learner.model, replay=self.replay, ops=ops, rank=rank)]
        else:
            # launch.py semantics on one device: the train actor owns a COPY of the network, refreshed when a rollout is issued
            # (launch.py:34-36,58-62), rolls out on its own HIP stream into a stage ring while the learner runs its update block on the
            # current stream.  ``overlap=False`` issues the same work on one stream (used by the tests to show the overlap is race-free).
            self.stage = StageRing(ops, 2 * cfg.actor.sample_steps * cfg.actor.num_envs, self.replay.obs_bytes)
            self.actors = [None, agents.Actor(cfg, None, replay=self.stage, ops=ops, rank=rank)]
            # high priority: a rollout kernel that becomes ready goes ahead of the update block's queued kernels.  No difference with the device env (9.43 - 9.49 ms
            # either way); with a host env, whose workers wait for every step's actions, 23.5 -> 21.7 ms per iteration (profiles/r04_experiments.md)
            self.actor_stream = torch.cuda.Stream(priority=-1)
            self.overlap = True
        # what is in flight between two iterations: the launch schedule's rollout (``_pending``), the main schedule's rollout issued ahead (``_prefetched``)
        self._pending = self._prefetched = None
        # who runs the loop (``_native_loop``): None = undecided, False = the Python classes (``native_loop_reason`` says why), or the NativeLoop
        self._nl, self.native_loop_reason = None, None
        self._resume = None                               # ``load_snapshot``: what the handles take over at the first iteration
        self.on_snapshot_loaded = None                    # launch.TrainerNode's hook, called at the end of ``load_snapshot``
        self._stat_host = {}                              # ``_stats``: its page-locked buffers
        self._updates_done = None                         # the device's update count where the host has read it anyway (``_pipeline_ok``)
        self.pipelined_blocks = 0
        self._tstream = self._tev = self._mev = None      # the pipelined block's stream and events, created at first use
        self.epsilon_fn = epsilon_schedule(cfg)
        self.writer = None
        self._wandb = None
        if cfg.wandb and primary:
            try:
                import wandb
                wandb.init(project=cfg.name, config=to_dict(cfg))
                self._wandb = wandb
            except ImportError:
                pass
        if cfg.tb and primary:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(cfg.logdir)
            except ImportError:
                pass
        self.logger = logging.getLogger("agent0")
        # the reference gets level INFO and a console handler from Hydra's job-logging defaults; without Hydra they are set here, so that
        # msg.log and the console carry the per-iteration lines (trainer.py:158-169)
        if self.logger.getEffectiveLevel() > logging.INFO:
            self.logger.setLevel(logging.INFO)
        if not logging.getLogger().handlers and not any(isinstance(h, logging.StreamHandler) and not isinstance(h, logging.FileHandler) for h in self.logger.handlers):
            console = logging.StreamHandler()
            console.setFormatter(logging.Formatter("[%(asctime)s][%(name)s][%(levelname)s] - %(message)s"))
            self.logger.addHandler(console)
        if primary:
            try:
                os.makedirs(cfg.logdir, exist_ok=True)
                self.logger.addHandler(logging.FileHandler(os.path.join(cfg.logdir, "msg.log")))
            except OSError:
                pass
        self.num_transitions = cfg.actor.sample_steps * cfg.actor.num_envs
        self.Ls, self.Rs, self.RTs, self.Qs, self.FLs = [], [], [], [], []
        self.GNs = []                                     # learner.clip_grad_norm: the pre-clip gradient norms of the last update block
        self.PN = None                                    # learner.weight_decay: the parameter norm in front of the decay of the last update block's last update
        self.frame_count = 0
        L = int(cfg.learner.learner_steps)
        self._loss_means = ops.zeros(max(L, 1))
        self._floss_means = ops.zeros(max(L, 1))

    # ------------------------------------------------------------------ checkpoint / resume
    def save_checkpoint(self, path: str):
        """Weights under the reference's state_dict keys (loadable by the reference's DeepQNet) + optimizer and counters."""
        eng = self.learner.engine
        blob = {"model": {k: v.cpu() for k, v in self.learner.model.state_dict().items()},
                "model_target": {k: v.cpu() for k, v in self.learner.model_target.state_dict().items()},
                "adam_m": eng.adam_m.cpu(), "adam_v": eng.adam_v.cpu(), "state": eng.state.cpu(), "frame_count": self.frame_count,
                "algo": self.cfg.learner.algo.name, "obs_shape": tuple(self.cfg.obs_shape), "action_dim": int(self.cfg.action_dim),
                # what agent0/summary.py:39-58 reads from a run: the test returns ("ITRs"), the frame count, and — there from params.json —
                # game / algo / commit; all in the checkpoint here (agent0_amd/summary.py)
                "ITRs": [float(x) for x in self.RTs], "game": str(self.cfg.env_id), "name": str(self.cfg.name), "sha": _git_sha()}
        if hasattr(eng, "rms_sq"):
            blob["rms_sq"] = eng.rms_sq.cpu()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(blob, path)
        return path

    def load_checkpoint(self, path: str, weights_only: bool = False):
        blob = torch.load(path, map_location="cpu", weights_only=True)      # tensors, dicts, tuples, strings, ints only
        if blob.get("algo") not in (None, self.cfg.learner.algo.name) or int(blob.get("action_dim", self.cfg.action_dim)) != int(self.cfg.action_dim):
            raise ValueError(f"checkpoint {path} was written for {blob.get('algo')} / {blob.get('action_dim')} actions")
        self.learner.model.load_state_dict(blob["model"])
        self.learner.model_target.load_state_dict(blob.get("model_target", blob["model"]))
        if not weights_only and "adam_m" in blob:
            eng = self.learner.engine
            eng.adam_m.copy_(blob["adam_m"]); eng.adam_v.copy_(blob["adam_v"]); eng.state.copy_(blob["state"])
            if "rms_sq" in blob and hasattr(eng, "rms_sq"):
                eng.rms_sq.copy_(blob["rms_sq"])
            self.frame_count = int(blob.get("frame_count", 0))
            self._updates_done = None
            self.learner.updates_issued = int(eng.state[6])      # the device's count of loss-ring entries travels with the state block

    # ------------------------------------------------------------------ resumable snapshots: the run CONTINUES (deepq/snapshot.py, csrc/snapshot.hip)
    @property
    def _device_env(self) -> bool:
        """The device-resident env: its state can be saved (``Actor.state_dict``)."""
        return hasattr(self.actors[1].envs, "state_dict")

    @property
    def _host_env(self) -> bool:
        """Emulator processes, one pool or groups of them: a rollout occupies the host thread until its last step."""
        envs = self.actors[1].envs
        return hasattr(envs, "step_send") or hasattr(envs, "pools")

    def _snapshot_geometry(self):
        from . import snapshot as snap
        return snap.geometry(to_dict(self.cfg), "launch" if self.use_lp else "main", "device" if self._device_env else "host")

    def _snapshot_dir(self, path: str) -> str:
        return os.path.join(path, f"rank{self.rank}") if int(os.environ.get("WORLD_SIZE", "1")) > 1 else path

    def save_snapshot(self, path: str) -> str:
        """Everything a fresh process needs to continue THIS run: ``path/checkpoint.pth`` (``save_checkpoint``), ``path/state.pth`` (sampler, actor and learner
        state, the ring's metadata and priorities, the statistics windows) and ``path/frames.bin`` (the ring's frames, deduplicated by a0_snapshot_pack on their way
        out: each chunk of at most 4 096 rows goes through one device buffer and one page-locked host buffer, so host memory does not grow with ``replay.size``).
        A rollout issued ahead is waited for and saved as pending — the resumed run consumes it as this one would have.  Written to ``path.tmp`` and renamed, so a job
        killed mid-write leaves the previous snapshot intact.

        The continuation is bit-identical for the device-resident env.  HOST environments (emulator processes) cannot be saved: the snapshot restores learner,
        replay and sampler; the envs are reset, the actor's n-step windows start empty and a rollout in flight is booked first.  Data parallel: every rank writes
        ``path/rank<k>/``, no collective is added (untested beyond one rank, like everything multi-GPU here)."""
        from . import snapshot as snap
        path = self._snapshot_dir(path)
        nl = self._nl or None
        actor, rp, eng = self.actors[1], self.replay, self.learner.engine
        device_env = self._device_env
        # ---- what is in flight
        if not device_env:
            self._book_in_flight()
            pending = None
        elif nl is not None:
            pending = nl.wait_pending()
        else:
            pf = self._pending if self.use_lp else self._prefetched
            if pf is not None and self.use_lp:
                pf.done_ev.synchronize()
            pending = None if pf is None else {"kind": "launch" if self.use_lp else "main", "start": int(pf.start)}
        torch.cuda.synchronize()
        # ---- handle / class state
        if nl is not None:
            st = nl.state()
        else:
            st = {"replay": torch.from_numpy(snap.replay_blob(**rp.state_dict())), "learner_rng": [int(self.learner.rng.seed)] + [int(self.learner.rng.offsets.get(i, 0)) for i in range(8)]}
            if device_env:
                st["actor"] = torch.from_numpy(snap.actor_blob(actor.state_dict()))
        cpu = lambda t: None if t is None else t.detach().cpu().clone()
        st.update(pending=pending, frame_count=int(self.frame_count), updates_issued=int(self.learner.updates_issued),
                  windows={"Ls": list(self.Ls), "Rs": list(self.Rs), "RTs": list(self.RTs), "Qs": list(self.Qs), "FLs": list(self.FLs)},
                  act=cpu(rp.act), rew=cpu(rp.rew), done=cpu(rp.done), max_p=cpu(rp._pstate), priority=cpu(rp.priority) if rp.prioritize and not rp.use_sumtree else None,
                  tree=cpu(rp.tree) if rp.use_sumtree else None,
                  net={"online": cpu(eng.online.flat), "target": cpu(eng.target.flat), "eff_online": cpu(eng.online.eff), "eff_target": cpu(eng.target.eff),
                       "noise": cpu(eng.noise_joint) if eng.noise_joint is not None else ([cpu(eng.online.noise_buf), cpu(eng.target.noise_buf)] if eng.L.noisy else None),
                       "scalars": cpu(eng.scalars), "loss_ring": cpu(eng.loss_ring)})
        if eng.gnorm_ring is not None:
            st["net"]["gnorm_ring"] = cpu(eng.gnorm_ring)
        if self.use_lp:
            sg = self.stage
            st["stage"] = {"written": int(sg.written), "act": cpu(sg.act), "rew": cpu(sg.rew), "done": cpu(sg.done)}
        # ---- files
        tmp = snap.begin_write(path)
        self.save_checkpoint(os.path.join(tmp, "checkpoint.pth"))
        n_pending = self.num_transitions if (pending and pending["kind"] == "main") else 0       # rows of a rollout issued ahead lie at the write cursor, not yet committed
        plan = snap.chunk_plan(rp.size, min(rp.top + n_pending, rp.size), rp.written + n_pending)
        ff = snap.FrameFile(self.ops, rp.obs_bytes // 4, max((c["rows"] for c in plan), default=1))
        with open(os.path.join(tmp, "frames.bin"), "wb") as f:
            chunks = ff.write(f, rp.frames, plan, int(self.cfg.actor.num_envs), "replay")
            if self.use_lp:
                sg = self.stage
                chunks += ff.write(f, sg.frames, snap.chunk_plan(sg.size, min(sg.written, sg.size), sg.written, ff.max_rows), int(self.cfg.actor.num_envs), "stage")
            f.flush()
            os.fsync(f.fileno())
        st["meta"] = snap.make_meta(to_dict(self.cfg), self._snapshot_geometry(), chunks, rp.obs_bytes // 4,
                                    {"seed": int(self.cfg.seed), "packed_bytes": int(sum(c["bytes"] for c in chunks)), "ring_bytes": int(sum(c["rows"] for c in chunks)) * rp.row_bytes})
        torch.save(st, os.path.join(tmp, "state.pth"))
        snap.commit_write(path)
        return path

    def _book_in_flight(self):
        """A rollout issued ahead and never consumed is booked into the replay, a launch-schedule rollout in flight is waited for and dropped (what ``final`` does)."""
        if self._pending is not None:
            self.actors[1].sample_finish(self._pending)
            self._pending = None
        if self._nl:
            self._nl.drain_lp() if self.use_lp else self._nl.drain()
        if self._prefetched is not None:
            pending, self._prefetched = self._prefetched, None
            transitions, returns, qmax = self.actors[1].sample_finish(pending)
            self._book(transitions)
            self._collect(returns, qmax)

    def load_snapshot(self, path: str):
        """The inverse of ``save_snapshot``, into a freshly constructed Trainer of the same configuration (refused, with the differing keys named, when ring
        geometry, algo, ``num_envs``, ``n_step_q``, replay policy, schedule or env kind differ).  The seed is part of the state: a Trainer built with another seed
        continues the SAVED run.  The first iteration after it hands the loop to the library's handles as a new run would — over the restored buffers, with the
        restored state — or keeps it on the Python classes; a snapshot written under one loads under the other."""
        from . import snapshot as snap
        if self.frame_count != 0 or self.replay.written != 0 or self._nl:
            raise RuntimeError("load_snapshot needs a freshly constructed Trainer")
        path = snap.resolve_dir(self._snapshot_dir(path))
        st = torch.load(os.path.join(path, "state.pth"), map_location="cpu", weights_only=True)
        meta = st["meta"]
        snap.check_meta(meta)
        snap.check_geometry(meta["geometry"], self._snapshot_geometry(), f"snapshot {path}")
        actor, rp, eng, ln = self.actors[1], self.replay, self.learner.engine, self.learner
        dev = self.ops.device
        self.cfg.seed = int(meta["seed"])
        self.load_checkpoint(os.path.join(path, "checkpoint.pth"))
        net = st["net"]
        eng.online.flat.copy_(net["online"]); eng.target.flat.copy_(net["target"])
        eng.online.refresh_wt(); eng.target.refresh_wt()
        if net["eff_online"] is not None:
            eng.online.eff.copy_(net["eff_online"]); eng.target.eff.copy_(net["eff_target"])
        if net["noise"] is not None:
            if eng.noise_joint is not None:
                eng.noise_joint.copy_(net["noise"])
            else:
                eng.online.noise_buf.copy_(net["noise"][0]); eng.target.noise_buf.copy_(net["noise"][1])
        eng.scalars.copy_(net["scalars"]); eng.loss_ring.copy_(net["loss_ring"])
        if net.get("gnorm_ring") is not None and eng.gnorm_ring is not None:      # absent from snapshots written without learner.clip_grad_norm
            eng.gnorm_ring.copy_(net["gnorm_ring"])
        ln.rng.seed = int(st["learner_rng"][0])
        ln.rng.offsets = {i: int(o) for i, o in enumerate(st["learner_rng"][1:]) if o}
        ln.updates_issued = int(st["updates_issued"])
        # ---- replay: metadata, priorities, sampler state, frames
        rp.act.copy_(st["act"]); rp.rew.copy_(st["rew"]); rp.done.copy_(st["done"])
        if st["priority"] is not None:
            rp.priority.copy_(st["priority"])
        if st["tree"] is not None:
            rp._tree.copy_(st["tree"])
        rp.load_state_dict(snap.parse_replay_blob(st["replay"].numpy()))
        rp._pstate.copy_(st["max_p"])
        if self.use_lp:
            sg = self.stage
            sg.written = int(st["stage"]["written"])
            sg.act.copy_(st["stage"]["act"]); sg.rew.copy_(st["stage"]["rew"]); sg.done.copy_(st["stage"]["done"])
        ff = snap.FrameFile(self.ops, int(meta["frame_bytes"]), max((c["rows"] for c in meta["chunks"]), default=1))
        with open(os.path.join(path, "frames.bin"), "rb") as f:
            ff.read(f, rp.frames, [c for c in meta["chunks"] if c["buf"] == "replay"])
            if self.use_lp:
                ff.read(f, self.stage.frames, [c for c in meta["chunks"] if c["buf"] == "stage"])
        # ---- actor (device env), statistics, what was in flight
        pending = st.get("pending")
        if st.get("actor") is not None and self._device_env:
            actor.load_state_dict(snap.parse_actor_blob(st["actor"].numpy(), rp.obs_bytes))
            if pending and pending["kind"] == "main":
                self._prefetched = actor.pending_from(pending["start"])
            elif pending and self.use_lp:
                self._pending = actor.pending_from(pending["start"])
        w = st["windows"]
        self.Ls, self.Rs, self.RTs, self.Qs, self.FLs = list(w["Ls"]), list(w["Rs"]), list(w["RTs"]), list(w["Qs"]), list(w["FLs"])
        self.frame_count = int(st["frame_count"])
        self._updates_done = None
        self._resume = {"actor": st.get("actor"), "replay": st["replay"], "learner_rng": st["learner_rng"], "pending": pending}
        torch.cuda.synchronize()
        if self.on_snapshot_loaded is not None:      # launch.TrainerNode: the ranks agree on rank 0's reset seed again (learner.net_reset_freq)
            self.on_snapshot_loaded()
        return path

    # ------------------------------------------------------------------ trainer.py:74-119
    def step(self, transitions, returns, qmax):
        self._collect(returns, qmax)
        self._step_device(transitions)
        return self._result()

    # ------------------------------------------------------------------ the stages of one iteration, under the names NativeLoop gives its own: rollout, book, block, stats, collect, close
    def _book(self, transitions):
        """A finished (or merely issued: ``Actor.block_of``) rollout's rows become part of the replay and of the frame count."""
        self.replay.extend(transitions)
        self.frame_count += self.num_transitions

    def _collect(self, returns, qmax):
        self.Qs.extend(qmax)
        self.Rs.extend(returns)

    def _close(self, tic, sync=None):
        """The iteration's result dict with its ``fps``; ``sync``: what the host waits for before the clock is read (nothing, when the next rollout has been issued ahead)."""
        result = self._result()
        if sync is not None:
            sync()
        result.update(fps=self.num_transitions / (time.time() - tic))
        return result

    def _step_device(self, transitions, defer: bool = False):
        """trainer.py:76-110 without the host-side statistics: book the rollout, run the update block, send for its statistics.  Everything here is enqueued on the
        stream; nothing waits for the device except, without ``defer``, the one read of the block's statistics at the end — with it the caller gets the record and
        calls its ``finish`` once it has waited for an event recorded after this call."""
        self._book(transitions)
        blk = self._stats(self._block(), defer)
        if defer:
            return blk
        blk.finish(self)
        return None

    def _block_open(self, on_ring: bool) -> _BlockStats:
        """The record of the block about to be issued.  The Adam launch files every update's loss mean — and with learner.clip_grad_norm on its pre-clip gradient norm — in
        the slot of the update's count (DeviceLearner.loss_ring / gnorm_ring); ``on_ring`` False: a0_mean_rows per update fills ``_loss_means`` instead."""
        ln, eng = self.learner, self.learner.engine
        self.GNs = []
        return _BlockStats(ring0=ln.updates_issued if on_ring else None, gn0=ln.updates_issued if eng.gnorm_ring is not None else None,
                           state=None if eng.online.fused else eng.state)

    def _block(self) -> _BlockStats:
        """The update block, once the replay holds ``training_start_steps`` rows: pipelined where it may be, else strictly serial."""
        ln, eng = self.learner, self.learner.engine
        # the loss means come off the ring when the fused optimizer tail runs, the block fits the ring and ``train_batch`` is the learner's own
        blk = self._block_open(eng.online.fused and self.cfg.learner.learner_steps <= eng.loss_ring.numel() and "train_batch" not in vars(ln)
                               and os.environ.get("A0_LOSS_RING", "1") != "0")
        if len(self.replay) <= self.cfg.trainer.training_start_steps:
            return blk
        if self._pipeline_ok():
            with self.ops.range("update_block"):
                self._update_block_pipelined(blk)
        else:
            self._update_block_serial(blk)
        return blk

    def _mean_buffers(self, n: int):
        if self._loss_means.numel() < n or self._floss_means.numel() < n:       # learner_steps changed after construction
            self._loss_means, self._floss_means = self.ops.zeros(n), self.ops.zeros(n)

    def _update_block_serial(self, blk: _BlockStats):
        """trainer.py:83-104: sample -> train -> priority update, ``learner_steps`` times on the current stream."""
        cfg, rp = self.cfg, self.replay
        B = cfg.learner.batch_size
        self._mean_buffers(cfg.learner.learner_steps)
        for i in range(cfg.learner.learner_steps):
            b = rp.sample()
            q_loss, f_loss = self.learner.train_batch(rp.frames, b.slot, rp.row_bytes, b.act, b.rew, b.done, b.weights)
            if cfg.replay.policy == ReplayEnum.prioritize:
                rp.update_priority(b.idx, q_loss, state=self.learner.engine.state)
            if blk.ring0 is None:
                self.ops.mean_rows(q_loss, 1, B, self._loss_means[i:i + 1])      # one launch; read back once per update block
            if f_loss is not None:
                self.ops.mean_rows(f_loss, 1, B, self._floss_means[i:i + 1])
                blk.has_frac = True
            blk.n_upd += 1

    def _stats(self, blk: _BlockStats, defer: bool) -> _BlockStats:
        """The block's statistics on their way to the host: read now (the one device->host stop of the update block), or with ``defer`` (``run_iteration(prefetch=True)``,
        the launch schedule) copied into page-locked buffers, stream-ordered behind the block and ahead of whatever is enqueued next.  The gradient norms and the last
        update's sums of squares travel with the loss means: one more small copy per block each, none per update."""
        if not blk.n_upd:
            return blk
        eng = self.learner.engine
        read = (lambda name, src: pinned_copy(self._stat_host, name, src)) if defer else (lambda name, src: src.cpu())
        blk.loss = read("means", self._loss_means) if blk.ring0 is None else read("ring", eng.loss_ring)
        if blk.has_frac:
            blk.floss = read("fmeans", self._floss_means)
        if blk.gn0 is not None:
            blk.gnorm = read("gnorm", eng.gnorm_ring)
        if eng.wd_partials is not None:
            blk.wd_partials = read("wd_partials", eng.wd_partials)
        # the device's update count (NaN-skipped steps do not count) for the next block's pipelining decision: read only where the host has just waited for the
        # block anyway, so that the next block can be enqueued behind the rollout without a stop
        self._updates_done = int(eng.state[1]) if not defer and self._pipeline_candidate() else None
        return blk

    # ------------------------------------------------------------------ the update block with the target network's passes one update ahead
    def _pipeline_candidate(self) -> bool:
        cfg, ln = self.cfg, self.learner
        # OFF by default: measured slower than the strictly serial block on MI355X (profiles/r04_experiments.md) — kept as a tested option
        return (os.environ.get("A0_PIPELINE_TARGET", "0") == "1" and cfg.replay.policy != ReplayEnum.prioritize and cfg.learner.learner_steps >= 2
                and ln.engine.target_stage_supported and ln.use_graph)

    def _pipeline_ok(self) -> bool:
        """Uniform replay (the next batch does not depend on this update's priorities), a learner whose target pass can run as a stage of its own, the
        hot-loop entry points not wrapped by a test harness, and no target sync inside this block: Adam's fused target copy at the end of update k would race
        with the target pass of batch k + 1 — such a block (one in target_update_freq / learner_steps) runs strictly in order."""
        cfg, ln = self.cfg, self.learner
        if not self._pipeline_candidate():
            return False
        if "sample" in vars(self.replay) or "train_batch" in vars(ln) or "update_priority" in vars(self.replay):      # instance-level wrappers (tests/test_gpu_trace.py)
            return False
        if self._updates_done is None:
            self._updates_done = int(ln.engine.state[1])          # one small read per block; NaN-skipped steps do not count, so the device's number is the one to use
        c0, L, f = self._updates_done, int(cfg.learner.learner_steps), int(cfg.learner.target_update_freq)
        return (c0 + L) // f == c0 // f                           # no multiple of f in (c0, c0 + L]: no sync in this block, however many steps a NaN skips

    def _update_block_pipelined(self, blk: _BlockStats):
        """trainer.py:83-104's loop with the same work in the same per-update order, except that batch k + 1 is drawn and pushed through the TARGET network
        (encoder + fc1 GEMM, ~70 us for dqn at B = 512) on a second stream while update k runs: those kernels fill the CUs that update k's latency-bound
        launches (512-row GEMMs, head / loss, reductions, Adam) leave idle.  Two sets of batch and target-stage buffers alternate; update k + 1 waits for its
        stage through an event, the stage of batch k + 2 waits for update k (the last reader of the buffers it overwrites).  Numbers are unchanged."""
        cfg, rp, ln = self.cfg, self.replay, self.learner
        L, B = int(cfg.learner.learner_steps), cfg.learner.batch_size
        self._mean_buffers(L)
        if self._tstream is None:
            self._tstream = torch.cuda.Stream()
            self._tev = [torch.cuda.Event(), torch.cuda.Event()]
            self._mev = torch.cuda.Event()
        self.pipelined_blocks += 1
        cur = torch.cuda.current_stream()
        batches = [None, None]
        batches[0] = rp.sample(buf=0)
        ln.target_stage_batch(rp.frames, batches[0].slot, rp.row_bytes, 0)          # the first batch's stage has nothing to hide behind: same stream
        for i in range(L):
            p = i & 1
            if i + 1 < L:
                q = p ^ 1
                self._mev.record(cur)                     # update i - 1 (last reader of parity q's buffers) is complete on the main stream here
                self._tstream.wait_event(self._mev)
                with torch.cuda.stream(self._tstream):
                    batches[q] = rp.sample(buf=q)
                    ln.target_stage_batch(rp.frames, batches[q].slot, rp.row_bytes, q)
                    self._tev[q].record(self._tstream)
            if i > 0:
                cur.wait_event(self._tev[p])
            b = batches[p]
            q_loss, _ = ln.train_batch(rp.frames, b.slot, rp.row_bytes, b.act, b.rew, b.done, b.weights, tstage=p)
            if blk.ring0 is None:
                self.ops.mean_rows(q_loss, 1, B, self._loss_means[i:i + 1])
        blk.n_upd = L

    def _result(self):
        """The result dict of trainer.py:111-118; with learner.clip_grad_norm on also ``grad_norm``, the mean pre-clip gradient norm over the last block's updates; with
        learner.net_reset_freq on also ``net_resets`` = update_steps // N; with learner.weight_decay on also ``param_norm``, the L2 norm of everything Adam owns in
        front of the decay of the last block's last update; with learner.redo_freq on also ``dormant_frac`` and ``dormant_frac_conv1|conv2|conv3|fc1``, the share of
        dormant neurons at the newest evaluation, overall and per layer; with learner.rank_freq on also ``feature_rank``, srank_delta of the fc1 activations at the
        newest evaluation."""
        eng = self.learner.engine
        out = self._result_base()
        if eng.gnorm_ring is not None:
            out["grad_norm"] = np.mean(self.GNs) if len(self.GNs) > 0 else None
        if eng.net_reset_freq > 0:      # learner.net_reset_freq: the resets so far, from the device's step count (one small read per logged iteration)
            out["net_resets"] = int(eng.state[1]) // eng.net_reset_freq
        if eng.wd_partials is not None:
            out["param_norm"] = self.PN
        if eng.redo_freq > 0:           # learner.redo_freq: the newest evaluation's dormant counts (one small read more per logged iteration); NaN until there is one
            c = (self._nl.redo_views[2] if self._nl else eng.redo_counts).tolist()      # the handle evaluates into buffers of its own
            seen = c[5] >= 0
            out["dormant_frac"] = c[4] / float(REDO_NEURONS) if seen else float("nan")
            for (name, _, n), k in zip(REDO_LAYERS, c[:4]):
                out[f"dormant_frac_{name}"] = k / float(n) if seen else float("nan")
        # learner.rank_freq: the newest evaluation's rank (one small read more per logged iteration); NaN until there is one and for -1 (a non-finite activation).
        # An engine stand-in written before the setting existed has no such field.
        if getattr(eng, "rank_freq", 0) > 0:
            r = (self._nl.rank_views[1] if self._nl else eng.rank_result).tolist()      # the handle evaluates into buffers of its own
            out["feature_rank"] = float(r[0]) if r[2] >= 0 and r[0] >= 0 else float("nan")
        return out

    def _result_base(self):
        return dict(
            frames=self.frame_count,
            fraction_loss=np.mean(self.FLs[-20:]) if len(self.FLs) > 0 else None,
            loss=np.mean(self.Ls[-20:]) if len(self.Ls) > 0 else None,
            return_train=np.mean(self.Rs[-20:]) if len(self.Rs) > 0 else None,
            return_train_max=np.max(self.Rs) if len(self.Rs) > 0 else None,
            qmax=np.mean(self.Qs[-100:]) if len(self.Qs) > 0 else None,
        )

    # ------------------------------------------------------------------ trainer.py:121-156
    def test(self):
        cfg = self.cfg
        if self.actors[0] is None:
            self.actors[0] = agents.Actor(cfg, self.learner.model, replay=None, ops=self.ops, rank=self.rank + 1000)
        if self.use_lp:
            torch.cuda.synchronize()                # the test actor shares the learner's weights: no update may be in flight
        rs = []
        video = []
        self.logger.info("Testing ... ")
        self.actors[0].reset()
        guard = 0
        while len(rs) < cfg.trainer.test_episodes and guard < 200:
            images, returns, _ = self.actors[0].sample(cfg.actor.test_eps, test=True)
            rs.extend(returns)
            if len(video) < 3600:                   # trainer.py:131-132: the newest frame of the first four envs, per step
                video.extend(images)
            guard += 1
        self.RTs.extend(rs)
        # trainer.py:134-135: (n, t, c, h, w) uint8 with the grey channel repeated three times
        self.last_test_video = np.repeat(np.stack(video, axis=1), 3, axis=2) if video else None
        if rs:
            if self.writer is not None:
                self.writer.add_scalar("return_test", np.mean(rs), self.frame_count)
                self.writer.add_scalar("return_test_max", np.max(self.RTs), self.frame_count)
                if self.last_test_video is not None and hasattr(self.writer, "add_video"):
                    self.writer.add_video("test_video", self.last_test_video, self.frame_count, fps=60)
            if self._wandb is not None:
                self._wandb.log({"return_test": np.mean(rs), "frame": self.frame_count})
                self._wandb.log({"return_test_max": np.max(self.RTs), "frame": self.frame_count})
                if self.last_test_video is not None:
                    self._wandb.log({"test_video": self._wandb.Video(self.last_test_video, fps=60, format="mp4"), "frame": self.frame_count})
            self.logger.info(f"TEST ---> Frames: {self.frame_count} | Return Avg: {np.mean(rs):.2f} Max: {np.max(rs)}")
        return rs

    def logging(self, result):
        if not self.primary:
            return
        self._progress_row(result)
        msg = ""
        for k, v in result.items():
            if v is None:
                continue
            if self.writer is not None:
                self.writer.add_scalar(k, v, self.frame_count)
            if self._wandb is not None:
                self._wandb.log({k: v, "frame": self.frame_count})
            if k == "net_resets":
                msg += f"{k}: {v} | "
            elif k.startswith("dormant_frac"):
                msg += f"{k}: {v:.3f} | "
            elif k == "feature_rank":
                msg += f"{k}: {v:.0f} | "
            elif k in ["frames", "loss", "qmax", "fps", "grad_norm", "param_norm"] or "return" in k:
                msg += f"{k}: {v:.2f} | "
        self.logger.info(msg)

    def _progress_row(self, result):
        """One CSV row per logged iteration under the run directory (``progress.csv``, columns = the result keys of trainer.py:111-118 plus
        fps): the machine-readable twin of msg.log, aggregated across runs by agent0_amd/summary.py."""
        import csv

        try:
            path = os.path.join(self.cfg.logdir, "progress.csv")
            new = not os.path.exists(path)
            with open(path, "a", newline="") as f:
                w = csv.writer(f)
                cols = PROGRESS_COLUMNS + (("grad_norm",) if "grad_norm" in result else ())      # only with learner.clip_grad_norm on
                cols = cols + (("net_resets",) if "net_resets" in result else ())               # only with learner.net_reset_freq on
                cols = cols + (("param_norm",) if "param_norm" in result else ())               # only with learner.weight_decay on
                cols = cols + tuple(k for k in REDO_COLUMNS if k in result)                      # only with learner.redo_freq on
                cols = cols + (("feature_rank",) if "feature_rank" in result else ())           # only with learner.rank_freq on
                if new:
                    w.writerow(cols)
                w.writerow(["" if result.get(k) is None else result[k] for k in cols])
        except OSError:
            pass

    # ------------------------------------------------------------------ the launch schedule (launch.py:30-63)
    def _snapshot_lp(self):
        """First half of ``actor.futures.sample(eps, state_dict)`` (launch.py:34-36,58-62): epsilon from the frame count as it is now, and the weight snapshot on the
        learner's stream — ordered after every update enqueued so far and before the next one.  Returns (epsilon, the event the rollout has to wait for)."""
        eps = self.epsilon_fn(self.frame_count)
        self.actors[1].model._dev.copy_from(self.learner.model._dev)
        return eps, torch.cuda.current_stream().record_event()

    def _rollout_lp(self, eps, ev):
        """Second half: the rollout into the free half of the stage, on the actor stream once the snapshot has landed, without waiting for it."""
        st = self.actor_stream if self.overlap else torch.cuda.current_stream()
        st.wait_event(ev)
        with torch.cuda.stream(st):
            pending = self.actors[1].sample_async(eps)
        self.stage.written += self.num_transitions  # the next rollout goes to the other half of the stage
        return pending

    def run_iteration_lp(self):
        """One pass of the loop body of launch.py:44-63: collect the finished rollout, issue the next one with the current weights,
        then run the update block on the collected transitions while that rollout is in flight."""
        tic = time.time()
        if self._pending is None:
            self._pending = self._rollout_lp(*self._snapshot_lp())      # launch.py:32-37 primes the pipeline before the loop
        transitions, returns, qmax = self.actors[1].sample_finish(self._pending)
        snap = self._snapshot_lp()
        if self.overlap and self._host_env:
            # a HOST env's rollout occupies this thread until its last step (it waits for the worker processes), so the update block — which needs nothing from the
            # thread once enqueued — goes first and the rollout then runs on the actor stream beside it: launch.py's actor processes stepping their emulators while
            # the learner trains (launch.py:44-63).  Same dependencies as the order below (weights snapshot before the block's first Adam, epsilon from the frame
            # count before the commit, the rollout into the other half of the stage), hence the same numbers (tests/test_gpu_trainer.py).
            self._collect(returns, qmax)
            blk = self._step_device(transitions, defer=True)
            self._pending = self._rollout_lp(*snap)
            torch.cuda.synchronize()
            blk.finish(self)
            return self._close(tic)
        self._pending = self._rollout_lp(*snap)
        self._collect(returns, qmax)
        self._step_device(transitions)
        return self._close(tic, torch.cuda.synchronize)

    # ------------------------------------------------------------------ who runs the loop
    def _native_loop(self):
        """The library's own handles over this Trainer's buffers (deepq/native_loop.py) when the configuration is one they cover, nothing has wrapped the hot-loop
        methods and no gradient hook is installed; decided at the first iteration, and final from then on (the handles own the actor's and the sampler's state)."""
        if self._nl is None:
            self._decide_native_loop()
        if not self._nl:
            return None
        if not self._unwrapped():
            raise RuntimeError("Trainer: a gradient hook or a method wrapper was installed after the native loop had taken over the run")
        return self._nl

    def _unwrapped(self) -> bool:
        from . import native_loop
        return native_loop.hook_ok(self.learner.engine.grad_hook) and not any(native_loop._wrapped(o) for o in (self, self.replay, self.learner, self.actors[1]))

    def _decide_native_loop(self):
        """Once per Trainer, and with ``final`` (which closes the handles) the only writer of ``_nl`` and ``native_loop_reason``."""
        from . import native_loop
        resume, self._resume = self._resume, None          # a loaded snapshot is the second legitimate starting point: the handles take over its state
        under_way = resume is None and (self._prefetched is not None or self.replay.written != 0 or self.actors[1].steps != 0 or self._pending is not None)
        why = native_loop.eligible(self)
        if why is None and (under_way or not self._unwrapped()):
            why = "hot-loop methods wrapped, a gradient hook, or a run already under way"
        nl = None
        if why is None:
            try:
                nl = native_loop.NativeLoop(self)
                if resume is not None:
                    nl.load_state(resume, resume["pending"])
                    self._prefetched = self._pending = None      # the handles hold what was in flight
            except RuntimeError as e:            # a create call refused the configuration: NativeLoop has destroyed what it had created; the Python classes run the loop
                nl, why = None, f"handle creation failed: {e}"
                if self.primary:
                    self.logger.info("host loop: Python classes (%s)", why)
        self._nl, self.native_loop_reason = (False, why) if nl is None else (nl, None)
        if nl is not None and self.primary:
            self.logger.info("host loop: library handles over this Trainer's buffers, device env or one host-env pool (agent0_amd/deepq/native_loop.py); A0_NATIVE_LOOP=0 keeps the Python classes in charge")

    def run_iteration(self, prefetch: bool = False):
        """One pass of the loop body of trainer.py:176-182; returns the result dict including fps.

        ``prefetch=True`` (``run()`` for every iteration but the last, bench.py's ``main`` schedule): the NEXT iteration's rollout is enqueued before the host
        waits for this iteration's statistics, which travel through page-locked buffers behind an event — same kernels in the same stream order with the same
        arguments (the next epsilon depends on the frame count only), so every number is the one the unpipelined loop produces
        (tests/test_gpu_trainer.py::test_prefetched_rollouts_change_no_number), but the GPU does not idle while Python collects statistics, logs and builds the
        next launch.  A rollout issued ahead is consumed by the next call (whatever its ``prefetch``), or booked into the replay by ``final()``."""
        nl = self._native_loop()
        with self.ops.range("iteration"):                 # roctx (A0_ROCTX=1): the handles open `rollout`, `sample`, `update`, `exchange` inside it
            if nl is not None:
                return nl.run_iteration_lp() if self.use_lp else nl.run_iteration(prefetch)
            return self.run_iteration_lp() if self.use_lp else self._run_iteration_py(prefetch)

    def _run_iteration_py(self, prefetch: bool):
        tic = time.time()
        # Same work in the same stream order as ``step(*actor.sample(eps))`` — the update block's kernels are ordered behind the rollout's — but
        # the host does not stop between them: the rollout's statistics (episode returns, per-step max-Q: one small read-back) are collected
        # after the update block has been enqueued instead of before, so the GPU never waits for Python at the rollout / update boundary.
        actor = self.actors[1]
        pending, self._prefetched = self._prefetched, None
        if pending is None:
            pending = actor.sample_async(self.epsilon_fn(self.frame_count))
        blk = self._step_device(actor.block_of(pending), defer=prefetch)
        if not prefetch:
            _, returns, qmax = actor.sample_finish(pending)
        else:
            st = actor.stats_async(pending)                                     # ahead of the next rollout, which overwrites the statistics buffers
            self._prefetched = actor.sample_async(self.epsilon_fn(self.frame_count))
            returns, qmax = actor.stats_finish(st)
            blk.finish(self)
        self._collect(returns, qmax)
        return self._close(tic, None if prefetch else torch.cuda.synchronize)

    def run(self):
        cfg = self.cfg
        if cfg.mode.name in ("finetune", "play"):
            if not cfg.checkpoint:
                raise ValueError(f"mode={cfg.mode.name} needs checkpoint=<path>")
            if cfg.mode.name == "finetune" and os.path.isdir(cfg.checkpoint):
                self.load_snapshot(cfg.checkpoint)           # a snapshot directory: the run continues (replay, sampler, actor and all)
            else:
                self.load_checkpoint(cfg.checkpoint, weights_only=(cfg.mode.name == "play"))
        if cfg.mode.name == "play":
            return self.final(save=False)
        remaining = max(cfg.trainer.total_steps - self.frame_count, 0)
        trainer_steps = remaining // self.num_transitions + 1
        ahead = os.environ.get("A0_PREFETCH_ROLLOUT", "1") != "0"
        snap_freq = int(cfg.trainer.snapshot_freq)
        for i in range(trainer_steps):
            self.logging(self.run_iteration(prefetch=ahead and i + 1 < trainer_steps))
            if snap_freq > 0 and (i + 1) % snap_freq == 0 and i + 1 < trainer_steps:
                self.save_snapshot(os.path.join(cfg.logdir, "snapshot"))
        self.final()

    def final(self, save: bool = True):
        self._book_in_flight()                                # so that replay and counters agree with the device
        if save and int(self.cfg.trainer.snapshot_freq) > 0:
            try:
                self.save_snapshot(os.path.join(self.cfg.logdir, "snapshot"))
            except OSError:
                pass
        try:
            if self.primary:
                self.test()
        finally:
            if save and self.primary:        # after the final test, so that its returns ("ITRs") are part of the run's record — and even if it failed
                try:
                    self.save_checkpoint(os.path.join(self.cfg.logdir, "final.pth"))
                except OSError:
                    pass
        if self._nl:
            self._nl.close()
            self._nl = False
        for actor in self.actors:
            if actor is not None:
                actor.close()
