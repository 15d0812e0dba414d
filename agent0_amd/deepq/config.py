"""Experiment configuration: the reference's ``ExpConfig`` tree, field for field, plus a Hydra-style override parser.

Mirrors /root/reference agent0/deepq/config.py:6-145 (enums 6-39, algorithm sub-configs 42-69, LearnerConfig 72-95,
TrainerConfig 98-105, ActorConfig 108-115, ReplayConfig 118-124, ExpConfig 127-145).  The reference builds the tree
with Hydra's ConfigStore + dacite (main.py:16-41); neither is installed here, so ``parse_overrides`` accepts the same
dotted ``key=value`` command-line syntax (README.md:44-53) and coerces enums / bools / numbers itself.

Additions (all default to the reference's behaviour being available):
  replay.sumtree   bool, default True — with ``replay.policy=prioritize`` draw batches proportionally from the HBM
                   sum-tree (what the north star builds).  False reproduces the reference, which despite its name
                   samples uniformly and only re-weights (quirks Q1/Q2/Q7 of SURVEY.md).
  learner.algo     accepts ``iqr`` (README spelling) as an alias of ``iqn`` (quirk Q10).
  env_task         reward task of the device-resident synthetic env (include/agent0_hip.h A0_ENV_TASK_*): ``stream`` (default; an action-independent reward
                   stream — the throughput workload) or ``block`` (learnable: +1 for naming the quadrant of the bright block in the newest frame,
                   -1 for the next class; chance 0, optimum +1 per step) or ``chase`` (temporal credit: the action moves the block on a 4 x 4 lattice, +1 only on
                   arrival at the target cell three to six moves away; optimum 0.25 per step) — what the learning tests train on.  Ignored by real Atari envs.
  actor.env_groups int, default 1 — host environments only: the number of groups the vector env is split into (env_pool.HostEnvGroups), each with its
                   own worker processes and page-locked ring, so that the CPU steps one group while the GPU infers the other (the counterpart of the
                   reference's ``num_actors`` actor processes, launch.py:30-61).  1 = one HostEnvPool.  Every setting gives the same bytes; which one is
                   fastest depends on the emulator's CPU cost per step, so it is the user's choice.  Ignored by the device-resident synthetic env.
  actor.eps_ladder float, default 0.0 (off; any value <= 0 is off).  alpha > 0: training rollouts explore with one epsilon PER ENVIRONMENT, Ape-X's ladder: env i of
                   the N environments acts with eps_i = eps^(1 + alpha * i / (N - 1)), eps being the scheduled scalar (so the decay to ``actor.min_eps`` keeps
                   working; Ape-X's own recipe is ``actor.min_eps=0.4 actor.eps_ladder=7``).  Env 0 keeps eps; while eps >= 1 — the warm-up, where the schedule
                   starts at 1 + min_eps (quirk Q15) — every env keeps it, so a ladder run is byte-identical to a plain one until eps drops below 1.  i and N
                   count over the whole job: rank * num_envs + e of world * num_envs under data parallelism, the env's index in the whole vector env for a
                   grouped host env.  Test rollouts, ``mode=play`` and ``Actor.act`` keep the scalar.  The vector is derived from eps every rollout: a snapshot
                   does not store it, and the setting may change across a resume like ``actor.min_eps``.
  learner.clip_grad_norm  float, default -1.0 (off; any value <= 0 is off).  > 0: every update scales the gradient Adam steps on — the whole Q-network: conv blocks, fc1,
                   the head, NoisyNet sigmas, the cosine embedding; not the fqf fraction net, which keeps ``max_grad_norm`` and its RMSprop step — by
                   min(1, clip_grad_norm / (norm + 1e-6)), i.e. ``torch.nn.utils.clip_grad_norm_`` with its defaults, and the pre-clip norm is reported as
                   ``grad_norm``.  The norm is that of the batch-SUM gradient (the loss is summed over the batch, quirk Q5), after the data-parallel exchange has
                   summed the ranks: a recipe's "10" for a batch-mean loss corresponds to 10 * batch_size here, times the world size under data parallelism.
  learner.target_tau  float, default 0.0 (off; any value <= 0 is off; >= 1 is refused — that is the hard copy).  0 < tau < 1: the target network is not overwritten
                   but moves towards the online one, target <- target + tau * (online - target) over the whole module, at exactly the updates where the hard
                   copy would have happened: every ``learner.target_update_freq`` updates, which keeps its meaning and default (the classical recipe is
                   ``learner.target_update_freq=1 learner.target_tau=0.005``).  The copy at construction and on checkpoint load stays a hard copy.  No state of
                   its own: the target is already in every snapshot, and the setting may change across a resume like ``actor.min_eps``.
  learner.aug_shift  int, default 0 (off; negative values, values >= min(H, W) of ``obs_shape`` and values above 16 are refused).  p > 0: DrQ's random shift of the
                   replay batch — every sampled observation is padded by p pixels with edge replication and cropped back at a random offset, one (dy, dx) in
                   [-p, p]^2 for all planes of an observation, st and st_next of a sample drawn independently; every pass of the update (target, double-Q,
                   online, conv1's weight gradient) reads the same shifted batch and the ring is never written.  DrQ's value for 84 x 84 frames is 4.  It applies to
                   the learner's batch only: training rollouts, test rollouts and ``mode=play`` see the frames unshifted, as in DrQ.  The synthetic env's ``block``
                   and ``chase`` tasks encode their information in position, so no learning claim is made for them.  The draws come from Philox stream 7 of the
                   learner's seed at the position the device's update count names: no state of its own, nothing new in a snapshot, and the setting may change
                   across a resume like ``actor.min_eps``.  Not with ``A0_PIPELINE_TARGET=1`` (the separately staged target pass reads the ring).
  learner.net_reset_freq  int, default 0 (off; negative values are refused).  N > 0: after every update that was not NaN-skipped and left ``update_steps`` a positive
                   multiple of N the Q-network is re-initialised on the device (a0_net_reset, one launch behind the update): fc1, the heads, NoisyNet's mu / sigma and
                   the cosine embedding get fresh values of the constructor's scale, the encoder (conv1 - conv3) keeps the share ``learner.net_reset_shrink`` of
                   its values, Adam's moments and bias correction restart, the target becomes a copy of the online network.  The fqf fraction net and its RMSprop
                   state are left alone.  BBF uses 40000, SR-SPR 20000 / replay ratio.  The fresh values are a function of (the learner's seed, the reset number, the
                   element): no state of its own, a resumed run resets as the uninterrupted one does.  Adds the statistic ``net_resets``.  Not together with
                   ``A0_PIPELINE_TARGET=1``.  (The name avoids ``reset_noise_freq``, which is NoisyNet's.)
  learner.net_reset_shrink  float in [0, 1], default 1.0 (anything else, NaN included, is refused).  The share alpha of the encoder that survives a reset,
                   p <- alpha * p + (1 - alpha) * fresh: 1.0 leaves the encoder untouched (Nikishin et al. 2022: the last layers only), 0.5 is BBF's and SR-SPR's
                   shrink-and-perturb, 0 re-initialises it.  Without ``learner.net_reset_freq`` it does nothing.
  learner.weight_decay  float, default 0.0 (off; any value <= 0 is off; NaN is refused).  lambda > 0: decoupled weight decay, ``torch.optim.AdamW(weight_decay=lambda)``:
                   every update that is not NaN-skipped first shrinks everything Adam owns — the convolutions, fc1, the heads, NoisyNet's mu and sigma, the
                   cosine embedding, biases included; not the fqf fraction net, which clipping and resets leave alone too — by p <- p - c * p,
                   c = learning_rate * lambda rounded to fp32 once, and then takes the Adam step on the shrunk values with the gradient computed at the undecayed
                   ones (a0_weight_decay, one launch in front of the Adam form; the update takes the three-launch tail, as under ``learner.clip_grad_norm``).
                   BBF and SR-SPR use 0.1.  c >= 1 is refused, and so is 0 < c < 2^-24, which would move no fp32 value.  Masks that exempt biases or sigmas are
                   not offered.  Adds the statistic ``param_norm``: the L2 norm of everything Adam owns as it stood in front of the decay of the block's last
                   update.  No state of its own, nothing new in a snapshot, and the setting may change across a resume like ``actor.min_eps``.
  learner.redo_freq  int, default 0 (off; negative values are refused).  N > 0: after every update that was not NaN-skipped and left ``update_steps`` a positive
                   multiple of N the dormancy score of Sokar et al. 2023 is taken on the device for the 672 hidden neurons (conv1's 32, conv2's 64 and conv3's 64
                   output channels, fc1's 512 units) from the activations of that update's batch: s_i = mean|h_i| / (the layer's mean of those means), dormant iff
                   s_i <= ``learner.redo_tau`` (a0_redo_score, two launches behind the update).  With ``learner.redo_recycle`` the dormant neurons are recycled
                   (ReDo; a0_redo_recycle, a third launch): incoming weights and bias get fresh values of the constructor's scale, outgoing weights become 0, Adam's
                   moments of both become 0; the rest of the network, the target network and the replay ring are untouched.  The fresh values are a function of
                   (the learner's seed, the recycle number, the element) on Philox stream 9: no state of its own, a resumed run recycles as the uninterrupted one
                   does.  Adds the statistics ``dormant_frac`` and ``dormant_frac_conv1|conv2|conv3|fc1`` (NaN until the first evaluation and after a resume).
                   Refused under the data-parallel path (``A0_DP_FORCE=1`` included): the ranks see different batches and would draw different masks.
  learner.redo_tau  float in [0, 1), default 0.1 (the paper's recycling threshold; anything else, NaN included, is refused with the number named).  0 counts only
                   neurons that are exactly silent; the paper's diagnostic uses 0.025.  Without ``learner.redo_freq`` it does nothing.
  learner.redo_recycle  bool, default true.  false measures only.  true together with ``learner.noisy_net`` is refused: ReDo is undefined for mu / sigma pairs.
  learner.rank_freq  int, default 0 (off; negative values are refused).  N > 0: after every update that was not NaN-skipped and left ``update_steps`` a positive
                   multiple of N the feature rank of Kumar et al. 2021 (srank_delta) is taken on the device from the fc1 activations X [rows][512] of that update's
                   differentiated pass (rows = the batch; the B * N rows of that pass for iqn / fqf): G = X^T X accumulated in double on the fp64 matrix pipe, its
                   512 eigenvalues, sigma_i = sqrt(lambda_i) with sigma_i = 0 where lambda_i <= 512 * 2^-52 * lambda_1, and the smallest k whose leading sigmas
                   reach the share 1 - ``learner.rank_delta`` of their sum (a0_feature_rank, two launches behind the update).  Nothing the update uses is written: a
                   run with the setting on is bit-identical to the same run with it off, so it is allowed under the data-parallel path (every rank evaluates
                   its own batch, rank 0's number is logged; verified on one rank only).  Adds the statistic ``feature_rank`` (NaN until the first evaluation and
                   after a resume, and when an activation was not finite); ``DeviceLearner.feature_spectrum()`` returns the 512 sigmas.  No state of its own,
                   nothing new in a snapshot, and the setting may change across a resume.
  learner.rank_delta  float in the open interval (0, 1), default 0.01 (the paper's delta; anything else, NaN included, is refused with the number named).  Without
                   ``learner.rank_freq`` it does nothing.
  learner.iqn.munchausen  bool, default false.  true (``learner.algo=iqn`` only): Munchausen-IQN (Vieillard, Pietquin, Geist 2020, section 5 and appendix B).  The
                   quantile targets become y_j = r + alpha * clamp(tau log pi(a|s), lo, 0) + gamma^n (1 - d) sum_a' pi(a'|s') (z'_j(a') - tau log pi(a'|s')), pi the softmax at
                   temperature tau of the TARGET network's mean over the N' target fractions, on s' and — one encoder pass and one N'-row head pass more — on s, at the
                   same fractions; there is no greedy next action, so the K-row selection pass is not run (its K fractions are still drawn: the Philox position is a
                   plain iqn run's).  It reads ``learner.mdqn.tau`` (0.03), ``learner.mdqn.alpha`` (0.9) and ``learner.mdqn.lo`` (-1): ``learner.mdqn.alpha`` is honoured
                   here and still unused by ``learner.algo=mdqn``, which keeps the reference's quirks — tau in alpha's place (Q17) and the temperature-1 softmax — and does
                   not change by a bit.  This follows the paper, not those quirks.  Acting is unchanged (epsilon-greedy on the K-sample mean).  Refused: any other algo
                   (fqf included), ``learner.double_q`` (no argmax to decouple), tau <= 0, alpha < 0, lo > 0 or any of them NaN or infinite, ``A0_PIPELINE_TARGET=1``.
                   No state of its own, nothing new in a snapshot, no new statistic, and the setting may change across a resume.
  learner.c51.hl_gauss  float, default 0.0 = off (any value <= 0 is off).  rho > 0 (``learner.algo=c51`` only): the HL-Gauss classification target of Farebrother et
                   al. 2024 ("Stop Regressing", ICML 2024) in the place of C51's projected target distribution.  Network, support, acting rule and cross entropy stay;
                   the atoms z_t = vmin + t Delta, Delta = (vmax - vmin) / (num_atoms - 1), become bin CENTRES with edges e_k = vmin - Delta / 2 + k Delta, and the
                   scalar target y = clamp(r + gamma^n (1 - d) E[Z(s', a*)], vmin, vmax) — a* chosen as before, the expectation under the TARGET network's softmax —
                   is spread over the bins as m_t = [Phi((e_{t+1} - y) / sigma) - Phi((e_t - y) / sigma)] / [Phi((e_T - y) / sigma) - Phi((e_0 - y) / sigma)] with
                   sigma = rho Delta (rho is the paper's sigma / Delta; its value is 0.75).  y is formed in fp32, the Gaussian mass in double on the device and rounded
                   to fp32 once.  Refused: NaN or infinite, rho > num_atoms (a sanity limit: sigma beyond the whole support), a sigma that is not a normal fp32
                   number, any other algo.  ``A0_PIPELINE_TARGET=1`` is allowed: c51's staged target pass ends at the fc1 slabs and the loss kernel reads them as
                   before.  No state of its own, nothing new in a snapshot, no new statistic, no Philox draw, and the setting may change across a resume.
  learner.iqn.risk  string, default ``neutral``; one of ``neutral | cvar | pow | cpw | wang``, case-insensitive (``learner.algo=iqn`` only): a risk-sensitive policy
                   (Dabney et al. 2018, section 4).  With tau the uniform fraction, the policy argmax_a (1/K) sum_k Q_{beta(tau_k)}(x, a) evaluates the network at
                   tau' = beta(tau): cvar eta tau; pow tau^(1/(1+|eta|)) for eta >= 0 and 1 - (1-tau)^(1/(1+|eta|)) for eta < 0; cpw tau^eta / (tau^eta + (1-tau)^eta)^(1/eta);
                   wang Phi(Phi^-1(tau) + eta).  It applies wherever the policy is evaluated: every actor evaluation (training and test rollouts, ``mode=play``,
                   ``Actor.act``; device env, host envs, ``actor.env_groups``, the attached pool) and, in the update, the K selection fractions of the greedy next
                   action only (the target network's, or the online network's under ``learner.double_q``).  The N' target and N online fractions stay uniform; loss,
                   priorities, NaN skip, Adam and target sync are untouched.  The distortion draws nothing: every Philox position is a neutral run's.  The paper's Norm
                   distortion is left out (it changes the number of draws).  Refused: an unknown name, any other algo (fqf included: its fractions are proposed, not
                   drawn), ``learner.iqn.munchausen`` (its target's policy is the softmax of the risk-neutral mean).  ``A0_PIPELINE_TARGET=1`` is allowed (the staged
                   target pass ends at the fc1 slabs and reads no fraction; iqn has no such stage anyway).  No state of its own, nothing new in a snapshot, no
                   new statistic, and the setting may change across a resume.
  learner.iqn.risk_eta  float, default 0.0: the distortion's parameter.  cvar and cpw: 0 < eta <= 1 (the paper: cvar 0.25 and 0.1, cpw 0.71); pow: finite, |eta| <= 64
                   (the paper: -2; eta < 0 is risk-averse); wang: finite, |eta| <= 8 (the paper: +-0.75; eta < 0 is risk-averse).  ``neutral`` ignores it.  Anything
                   else, NaN included, is refused with the setting and the number named.
  device           ``cuda`` is the only supported device: this build has no CPU path (it raises instead).
  checkpoint       path of a checkpoint written by ``Trainer.save_checkpoint``; read when ``mode`` is ``finetune`` (resume training)
                   or ``play`` (evaluate only) — the reference declares those modes (config.py:26-29) but never implements them.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field, fields, is_dataclass
from enum import Enum
from typing import Any, List, Sequence, get_type_hints


class AlgoEnum(Enum):
    dqn = 0
    c51 = 1
    qr = 2
    iqn = 3
    fqf = 4
    mdqn = 5


class ActorEnum(Enum):
    greedy = 0
    random = 1
    epsilon = 2


class ReplayEnum(Enum):
    uniform = 0
    prioritize = 1


class ModeEnum(Enum):
    train = 0
    finetune = 1
    play = 2


class EnvEnum(Enum):
    atari = 0
    mujoco = 1


class DeviceEnum(Enum):
    cuda = "cuda"
    cpu = "cpu"


ALGO_ALIASES = {"iqr": "iqn"}


@dataclass
class C51Config:
    num_atoms: int = 51
    vmax: float = 10
    vmin: float = -10
    hl_gauss: float = 0.0


@dataclass
class QRConfig:
    num_atoms: int = 200
    vmax: Any = None
    vmin: Any = None


@dataclass
class IQNConfig:
    K: int = 32
    N: int = 64
    N_dash: int = 64
    num_cosines: int = 64
    F: int = 32
    munchausen: bool = False
    risk: str = "neutral"
    risk_eta: float = 0.0


@dataclass
class MDQNConfig:
    tau: float = 0.03
    alpha: float = 0.9
    lo: float = -1


@dataclass
class LearnerConfig:
    algo: AlgoEnum = AlgoEnum.dqn
    discount: float = 0.99
    batch_size: int = 512
    learning_rate: float = 5e-4
    fraction_lr: float = 2.5e-8
    max_grad_norm: float = -1.0
    clip_grad_norm: float = -1.0
    target_update_freq: int = 500
    target_tau: float = 0.0
    aug_shift: int = 0
    net_reset_freq: int = 0
    net_reset_shrink: float = 1.0
    weight_decay: float = 0.0
    redo_freq: int = 0
    redo_tau: float = 0.1
    redo_recycle: bool = True
    rank_freq: int = 0
    rank_delta: float = 0.01
    learner_steps: int = 20
    double_q: bool = False
    dueling_head: bool = False
    n_step_q: int = 1
    noisy_net: bool = False
    reset_noise_freq: int = 4
    c51: C51Config = field(default_factory=C51Config)
    qr: QRConfig = field(default_factory=QRConfig)      # the reference passes the CLASS as default (quirk Q10); instances here
    iqn: IQNConfig = field(default_factory=IQNConfig)
    mdqn: MDQNConfig = field(default_factory=MDQNConfig)


@dataclass
class TrainerConfig:
    total_steps: int = int(1e7)
    training_start_steps: int = int(1e5)
    exploration_steps: int = int(1e6)
    log_freq: int = 10
    test_freq: int = 500
    test_episodes: int = 20
    snapshot_freq: int = 0                 # iterations between resumable snapshots into <logdir>/snapshot (Trainer.save_snapshot); 0 = off


@dataclass
class ActorConfig:
    policy: ActorEnum = ActorEnum.random
    num_envs: int = 16
    sample_steps: int = 80
    test_steps: int = 800
    min_eps: float = 0.01
    test_eps: float = 0.001
    env_groups: int = 1
    eps_ladder: float = 0.0


@dataclass
class ReplayConfig:
    size: int = int(1e6)
    policy: ReplayEnum = ReplayEnum.uniform
    beta0: float = 0.4
    alpha: float = 0.5
    eps: float = 0.01
    sumtree: bool = True


@dataclass
class ExpConfig:
    env_id: str = "Breakout"
    env_type: EnvEnum = EnvEnum.atari
    obs_shape: Any = (0,)
    action_dim: int = 0
    num_actors: int = 3
    seed: int = 42
    device: DeviceEnum = DeviceEnum.cuda
    name: str = "agent0"
    mode: ModeEnum = ModeEnum.train
    logdir: str = "logs"
    wandb: bool = True
    tb: bool = True
    checkpoint: str = ""
    env_task: str = "stream"
    learner: LearnerConfig = field(default_factory=LearnerConfig)
    trainer: TrainerConfig = field(default_factory=TrainerConfig)
    actor: ActorConfig = field(default_factory=ActorConfig)
    replay: ReplayConfig = field(default_factory=ReplayConfig)


# ----------------------------------------------------------------------------- overrides
def _coerce(raw: str, current: Any, annotation: Any):
    if isinstance(current, Enum):
        enum_t = type(current)
        name = ALGO_ALIASES.get(raw.lower(), raw) if enum_t is AlgoEnum else raw
        for member in enum_t:
            if member.name.lower() == name.lower() or str(member.value).lower() == name.lower():
                return member
        raise ValueError(f"{raw!r} is not one of {[m.name for m in enum_t]}")
    if isinstance(current, bool):
        if raw.lower() in ("true", "1", "yes", "on"):
            return True
        if raw.lower() in ("false", "0", "no", "off"):
            return False
        raise ValueError(f"{raw!r} is not a boolean")
    if isinstance(current, int) and not isinstance(current, bool):
        try:
            return int(raw)
        except ValueError:
            f = float(raw)            # e.g. total_steps=1e7
            if f != int(f):
                raise
            return int(f)
    if isinstance(current, float):
        return float(raw)
    if isinstance(current, (tuple, list)):
        inner = raw.strip("()[] ")
        vals = [int(v) for v in inner.split(",") if v.strip()]
        return tuple(vals)
    if current is None:
        if raw.lower() in ("null", "none"):
            return None
        try:
            return float(raw)
        except ValueError:
            return raw
    return raw


def apply_override(cfg: Any, dotted: str, raw: str) -> None:
    obj = cfg
    parts = dotted.split(".")
    for p in parts[:-1]:
        if not hasattr(obj, p):
            raise KeyError(f"unknown config group {p!r} in {dotted!r}")
        obj = getattr(obj, p)
    leaf = parts[-1]
    if not is_dataclass(obj) or leaf not in {f.name for f in fields(obj)}:
        raise KeyError(f"unknown config key {dotted!r}")
    setattr(obj, leaf, _coerce(raw, getattr(obj, leaf), None))


def parse_overrides(argv: Sequence[str], cfg: ExpConfig | None = None) -> ExpConfig:
    """``["env_id=Enduro", "learner.algo=c51", "actor.num_envs=256"]`` -> ExpConfig (Hydra's dotted override syntax)."""
    cfg = cfg or ExpConfig()
    for item in argv:
        if "=" not in item:
            raise ValueError(f"override {item!r} is not of the form key=value")
        key, raw = item.split("=", 1)
        apply_override(cfg, key.lstrip("+"), raw)
    return cfg


def to_dict(cfg: Any) -> dict:
    out = {}
    for f in fields(cfg):
        v = getattr(cfg, f.name)
        out[f.name] = to_dict(v) if is_dataclass(v) else (v.name if isinstance(v, Enum) else v)
    return out


def from_dict(d: dict, cfg: ExpConfig | None = None) -> ExpConfig:
    """dacite.from_dict equivalent for this tree (main.py:28)."""
    cfg = cfg or ExpConfig()

    def fill(obj, dd):
        for k, v in dd.items():
            cur = getattr(obj, k)
            if is_dataclass(cur) and isinstance(v, dict):
                fill(cur, v)
            elif isinstance(cur, Enum) and not isinstance(v, Enum):
                setattr(obj, k, _coerce(str(v), cur, None))
            else:
                setattr(obj, k, v)

    fill(cfg, d)
    return cfg
