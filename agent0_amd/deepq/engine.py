"""Device-side network and learner: composes the HIP kernels (through ``ops``) into the forward passes, losses,
backward passes and optimizer steps of the six reference learners.

``ops`` is the only door to the GPU (agent0_amd.ops.HipOps).  The composition is written against that interface so
the CPU test-suite can drive the very same code with an emulation backend (tests/cpu_ops.py) that runs the shared
C++ layer orchestration on the host — the product itself never does that.

Reference mapping (paths relative to the reference repo):
  DeviceNet.forward / qvalues   agent0/deepq/model.py:323-330 + heads 123-131, 163-177, 190-192, 219-257, 268-284
  DeviceLearner.update          agent0/deepq/agent.py:124-169 (BaseLearner.train) + train_step of each learner
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import torch

from .layout import Block, NetLayout

MODE_IDENT, MODE_MEAN, MODE_C51, MODE_FQF = 0, 1, 2, 3


def clip_limit(value) -> float:
    """``learner.clip_grad_norm`` as the learner uses it: the limit when it is positive, -1.0 (off) for anything else — zero, a negative number, None."""
    return float(value) if value is not None and value > 0 else -1.0


def target_tau_value(value) -> float:
    """``learner.target_tau`` as the learner uses it: tau when 0 < tau < 1, 0.0 (off) for zero, a negative number or None; tau >= 1 — the hard copy, which
    ``learner.target_update_freq`` alone gives — is refused."""
    if value is None or not value > 0:
        return 0.0
    tau = float(value)
    if tau >= 1.0:
        raise ValueError(f"learner.target_tau={tau!r}: must be below 1 (tau >= 1 is the hard copy: leave learner.target_tau off)")
    return tau


WEIGHT_DECAY_MIN_C = 2.0 ** -24      # the smallest lr * lambda, as an fp32 number, that still moves an fp32 parameter


def weight_decay_value(value, lr) -> float:
    """``learner.weight_decay`` as the learner uses it: the per-update coefficient c = fl32(lr * lambda) — formed in double, rounded to fp32 once — when lambda > 0,
    0.0 (off) for zero, a negative number or None.  Refused: NaN, c >= 1 (the update would wipe or flip the parameters) and 0 < c < 2^-24 (such a c moves no fp32
    value, and silently doing nothing is worse than an error)."""
    if value is None:
        return 0.0
    lam = float(value)
    if lam != lam:
        raise ValueError("learner.weight_decay=nan: must be a number (0.0 or any value <= 0 is off)")
    if not lam > 0:
        return 0.0
    c = float(torch.tensor(float(lr) * lam, dtype=torch.float64).to(torch.float32))
    if not c < 1.0:
        raise ValueError(f"learner.weight_decay={lam!r}: learning_rate * weight_decay = {float(lr)!r} * {lam!r} = {float(lr) * lam!r} must be below 1")
    if c < WEIGHT_DECAY_MIN_C:
        raise ValueError(f"learner.weight_decay={lam!r}: learning_rate * weight_decay = {float(lr)!r} * {lam!r} = {float(lr) * lam!r} is below 2^-24 = "
                         f"{WEIGHT_DECAY_MIN_C!r} and would move no fp32 parameter")
    return c


def aug_shift_value(value, obs_shape, pipeline_target: Optional[bool] = None) -> int:
    """``learner.aug_shift`` as the learner uses it: the pad p of DrQ's random shift, 0 (off) for zero or None.  Refused: a negative or fractional value, p >= min(H, W)
    of ``obs_shape`` (C, H, W), p > 16 — the kernel's own limits (a0_augment_shift) — and any p > 0 together with ``A0_PIPELINE_TARGET=1`` (``pipeline_target``; None
    reads the environment): the separately staged target pass reads the ring before the update that shifts the batch exists."""
    if value is None or value == 0:
        return 0
    if int(value) != value or value < 0:
        raise ValueError(f"learner.aug_shift={value!r}: must be a whole number of pixels >= 0 (0 is off)")
    p = int(value)
    H, W = int(obs_shape[-2]), int(obs_shape[-1])
    if p >= min(H, W):
        raise ValueError(f"learner.aug_shift={p}: must be below min(H, W) = {min(H, W)} of obs_shape {tuple(obs_shape)}")
    if p > 16:
        raise ValueError(f"learner.aug_shift={p}: must be at most 16 (DrQ's value for 84 x 84 frames is 4)")
    if pipeline_target is None:
        pipeline_target = os.environ.get("A0_PIPELINE_TARGET", "0") == "1"
    if pipeline_target:
        raise ValueError(f"learner.aug_shift={p}: not together with A0_PIPELINE_TARGET=1 (the separately staged target pass reads the unshifted ring)")
    return p


def munchausen_value(value, tau=0.03, alpha=0.9, lo=-1.0, algo: str = "iqn", double_q: bool = False, pipeline_target: Optional[bool] = None):
    """``learner.iqn.munchausen`` with ``learner.mdqn.tau`` / ``alpha`` / ``lo`` as the learner uses them: ``(on, tau, alpha, lo)``, the three numbers as Python floats.
    Refused, whether or not the setting is on: a tau that is not a finite number above 0 (as an fp32 number too — the kernel gets fp32), an alpha that is not a finite
    number >= 0, a lo that is not a finite number <= 0.  Refused with the setting on: any ``algo`` but iqn (fqf included), ``learner.double_q`` (the Munchausen target has
    no argmax to decouple), and ``A0_PIPELINE_TARGET=1`` (``pipeline_target``; None reads the environment): the update has two target passes and none of them is staged."""
    on = bool(value) if value is not None else False
    t, a, l = (float("nan") if x is None else float(x) for x in (tau, alpha, lo))
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(torch.float32))
    if not (t > 0 and math.isfinite(t) and f32(t) > 0 and math.isfinite(f32(t))):
        raise ValueError(f"learner.iqn.munchausen: learner.mdqn.tau={tau!r} must be a finite number above 0")
    if not (a >= 0 and math.isfinite(a) and math.isfinite(f32(a))):
        raise ValueError(f"learner.iqn.munchausen: learner.mdqn.alpha={alpha!r} must be a finite number >= 0")
    if not (l <= 0 and math.isfinite(l) and math.isfinite(f32(l))):
        raise ValueError(f"learner.iqn.munchausen: learner.mdqn.lo={lo!r} must be a finite number <= 0")
    if on:
        if algo != "iqn":
            raise ValueError(f"learner.iqn.munchausen=true: for learner.algo=iqn only, not learner.algo={algo} (mdqn is the scalar head's Munchausen learner)")
        if double_q:
            raise ValueError("learner.iqn.munchausen=true: not together with learner.double_q=true (the Munchausen target has no argmax to decouple)")
        if pipeline_target is None:
            pipeline_target = os.environ.get("A0_PIPELINE_TARGET", "0") == "1"
        if pipeline_target:
            raise ValueError("learner.iqn.munchausen=true: not together with A0_PIPELINE_TARGET=1 (the update has two target passes and neither is staged separately)")
    return on, t, a, l


RISK_PAPER_ETA = {"cvar": "0.25 or 0.1", "pow": "-2", "cpw": "0.71", "wang": "0.75 or -0.75"}      # Dabney et al. 2018, section 4


def risk_value(risk, eta=0.0, algo: str = "iqn", munchausen: bool = False):
    """``learner.iqn.risk`` / ``learner.iqn.risk_eta`` as the actor and the learner use them: ``(kind, eta)``, kind the A0_RISK_* number (0: neutral) and eta a Python
    float (0.0 for neutral, which ignores it).  Refused, each with the setting and the number named: a name that is none of neutral | cvar | pow | cpw | wang (any
    letter case; None is neutral), an eta outside the kind's range — cvar and cpw 0 < eta <= 1 (cvar: as an fp32 number too, the kernel multiplies by that), pow
    finite |eta| <= 64, wang finite |eta| <= 8 —, NaN or infinite; and with a kind other than neutral: any ``algo`` but iqn (fqf included: its fractions are
    proposed, not drawn) and ``learner.iqn.munchausen`` (its target's policy is the softmax of the risk-neutral mean).  ``A0_PIPELINE_TARGET=1`` / ``tstage`` need no
    refusal of their own: the staged target pass (``target_stage``) ends at the fc1 slabs and reads no fraction, and an iqn learner has no such stage to begin with."""
    from agent0_amd.ops import RISK_KINDS
    name = "neutral" if risk is None else str(risk).strip().lower()
    if name not in RISK_KINDS:
        raise ValueError(f"learner.iqn.risk={risk!r} is not one of {' | '.join(RISK_KINDS)}")
    kind = RISK_KINDS[name]
    if kind == 0:
        return 0, 0.0
    e = float("nan") if eta is None else float(eta)
    if name in ("cvar", "cpw"):
        ok = 0.0 < e <= 1.0 and (name == "cpw" or float(torch.tensor(e, dtype=torch.float64).to(torch.float32)) > 0.0)
        want = "0 < eta <= 1"
    else:
        lim = 64.0 if name == "pow" else 8.0
        ok, want = abs(e) <= lim, f"a finite number with |eta| <= {lim:g}"
    if not ok:
        hint = f" (the default 0 is not a {name} parameter; the paper uses {RISK_PAPER_ETA[name]})" if e == 0.0 else f" (the paper uses {RISK_PAPER_ETA[name]})"
        raise ValueError(f"learner.iqn.risk={name}: learner.iqn.risk_eta={eta!r} must be {want}{hint}")
    if algo != "iqn":
        raise ValueError(f"learner.iqn.risk={name}: for learner.algo=iqn only, not learner.algo={algo} (fqf proposes its fractions, it does not draw them)")
    if munchausen:
        raise ValueError(f"learner.iqn.risk={name}: not together with learner.iqn.munchausen=true (its target's policy is the softmax of the risk-neutral mean; "
                         "acting on a distorted one is a different agent)")
    return kind, e


def hl_gauss_value(value, vmin=-10.0, vmax=10.0, num_atoms=51, algo: str = "c51", pipeline_target: Optional[bool] = None):
    """``learner.c51.hl_gauss`` as the learner uses it: ``(rho, sigma)`` as Python floats, sigma = rho * Delta with Delta = (vmax - vmin) / (num_atoms - 1) formed in
    double — the number the kernels receive, as a double — and ``(0.0, 0.0)`` (off) for zero, a negative number or None.  Refused: a rho that is NaN or infinite;
    with the setting on: rho > num_atoms (sigma would exceed the whole support and the histogram is flat: a sanity limit, not a numerical one), a sigma that is
    not a normal fp32 number (a degenerate support included), and any ``algo`` but c51.  ``A0_PIPELINE_TARGET=1`` (``pipeline_target``) is ALLOWED and the
    argument is only accepted for symmetry with the other settings: c51's separately staged target pass ends at the target's fc1 slabs, which the loss kernel reads
    as it does without the stage, and nothing this setting changes is read or written by that stage."""
    if value is None:
        return 0.0, 0.0
    rho = float(value)
    if not math.isfinite(rho):
        raise ValueError(f"learner.c51.hl_gauss={value!r}: must be a finite number (0.0 or any value <= 0 is off; the paper's sigma / Delta is 0.75)")
    if not rho > 0:
        return 0.0, 0.0
    if algo != "c51":
        raise ValueError(f"learner.c51.hl_gauss={rho!r}: for learner.algo=c51 only, not learner.algo={algo}")
    T = int(num_atoms)
    if rho > T:
        raise ValueError(f"learner.c51.hl_gauss={rho!r}: must be at most learner.c51.num_atoms = {T} (sigma = rho * Delta would exceed the whole support)")
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))
    delta = (f32(vmax) - f32(vmin)) / (T - 1) if T > 1 else float("nan")      # of vmin and vmax as the kernels receive them (fp32), as a0_learner_set_hl_gauss forms it
    sigma = rho * delta
    s32 = f32(sigma)
    if not (math.isfinite(s32) and s32 >= 2.0 ** -126):
        raise ValueError(f"learner.c51.hl_gauss={rho!r}: sigma = rho * (vmax - vmin) / (num_atoms - 1) = {rho!r} * ({float(vmax)!r} - {float(vmin)!r}) / {T - 1} = {sigma!r} "
                         "is not a normal fp32 number")
    return rho, sigma


def net_reset_value(freq, shrink=1.0, pipeline_target: Optional[bool] = None):
    """``learner.net_reset_freq`` / ``learner.net_reset_shrink`` as the learner uses them: ``(N, alpha)``, N = 0 (off) for zero or None.  Refused: a negative or
    fractional N, an alpha outside [0, 1] (NaN included; checked whether or not N is on), and N > 0 together with ``A0_PIPELINE_TARGET=1`` (``pipeline_target``; None
    reads the environment): the separately staged target pass reads a target network the reset rewrites."""
    if freq is None:
        freq = 0
    if isinstance(freq, bool) or int(freq) != freq or freq < 0:
        raise ValueError(f"learner.net_reset_freq={freq!r}: must be a whole number of updates >= 0 (0 is off)")
    alpha = 1.0 if shrink is None else float(shrink)
    if not (0.0 <= alpha <= 1.0):
        raise ValueError(f"learner.net_reset_shrink={shrink!r}: must lie in [0, 1] (1 keeps the encoder, 0 re-initialises it)")
    n = int(freq)
    if n > 0:
        if pipeline_target is None:
            pipeline_target = os.environ.get("A0_PIPELINE_TARGET", "0") == "1"
        if pipeline_target:
            raise ValueError(f"learner.net_reset_freq={n}: not together with A0_PIPELINE_TARGET=1 (the separately staged target pass reads a target the reset rewrites)")
    return n, alpha


def redo_value(freq, tau=0.1, recycle=True, noisy=False, data_parallel: Optional[bool] = None):
    """``learner.redo_freq`` / ``learner.redo_tau`` / ``learner.redo_recycle`` as the learner uses them: ``(N, tau, recycle)``, N = 0 (off) for zero or None.
    Refused: a negative or fractional N, a tau that is not a finite number in [0, 1) (checked whether or not N is on), and with N > 0: recycling together with
    ``learner.noisy_net`` (``noisy``; measuring only is allowed) and any use under the data-parallel path (``data_parallel``; None reads WORLD_SIZE and
    ``A0_DP_FORCE``): the ranks see different batches, would draw different masks and would diverge."""
    if freq is None:
        freq = 0
    if isinstance(freq, bool) or int(freq) != freq or freq < 0:
        raise ValueError(f"learner.redo_freq={freq!r}: must be a whole number of updates >= 0 (0 is off)")
    t = 0.1 if tau is None else float(tau)
    if not (0.0 <= t < 1.0):
        raise ValueError(f"learner.redo_tau={tau!r}: must be a finite number in [0, 1) (0 recycles only neurons that are exactly silent)")
    n, rec = int(freq), bool(recycle)
    if n > 0:
        if rec and noisy:
            raise ValueError(f"learner.redo_freq={n}: learner.redo_recycle=true is undefined together with learner.noisy_net (mu / sigma pairs); "
                             "learner.redo_recycle=false measures only")
        if data_parallel is None:
            data_parallel = int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 or os.environ.get("A0_DP_FORCE", "0") == "1"
        if data_parallel:
            raise ValueError(f"learner.redo_freq={n}: not under the data-parallel path (A0_DP_FORCE=1 included): the ranks see different batches and would draw "
                             "different dormancy masks")
    return n, t, rec


def rank_value(freq, delta=0.01):
    """``learner.rank_freq`` / ``learner.rank_delta`` as the learner uses them: ``(N, delta)``, N = 0 (off) for zero or None.  Refused: a negative or fractional N, a
    delta that is not a number in the open interval (0, 1) (checked whether or not N is on).  Allowed under the data-parallel path: the evaluation writes nothing
    the update uses, so the replicas cannot diverge."""
    if freq is None:
        freq = 0
    if isinstance(freq, bool) or int(freq) != freq or freq < 0:
        raise ValueError(f"learner.rank_freq={freq!r}: must be a whole number of updates >= 0 (0 is off)")
    d = 0.01 if delta is None else float(delta)
    if not (0.0 < d < 1.0):
        raise ValueError(f"learner.rank_delta={delta!r}: must be a number in the open interval (0, 1)")
    return int(freq), d


class Workspace:
    """Activations of one forward pass over ``B`` observations (``n_tau`` quantile samples each for IQN/FQF)."""

    def __init__(self, ops, L: NetLayout, B: int, n_tau: int = 1, grads: bool = False):
        self.B, self.n_tau, self.grads = B, n_tau, grads
        R = B * n_tau if L.quantile else B
        self.R = R
        self.act1 = ops.empty(B * L.H1 * L.W1 * 32)
        self.act2 = ops.empty(B * L.H2 * L.W2 * 64)
        self.act3 = ops.empty(B * L.feat)
        self.h = ops.empty(R * 512)
        self.raw = ops.empty(R * L.Npad)
        self.q = ops.empty(R * L.A * L.T)
        if L.quantile:
            self.cosx = ops.empty(R * L.num_cosines)
            self.emb = ops.empty(R * L.feat)
            self.x = ops.empty(R * L.feat)
            self.taus = ops.empty(R)
        if L.algo == "fqf":
            self.frac_logits = ops.empty(B * L.Fpad)
            self.tau_all = ops.empty(B * (L.F + 1))
            self.tau_hat = ops.empty(B * L.F)
        if grads:
            self.dq = ops.zeros(R * L.A * L.T)
            self.draw = ops.empty(R * L.Npad)
            self.dh = ops.empty(R * 512)
            self.d3 = ops.empty(B * L.feat)
            self.d2 = ops.empty(B * L.H2 * L.W2 * 64)
            self.d1 = ops.empty(B * L.H1 * L.W1 * 32)
            if L.quantile:
                self.dx = ops.empty(R * L.feat)
                self.demb = ops.empty(R * L.feat)


class DeviceNet:
    """One set of network parameters on the device in the packed layout, plus forward-pass composition."""

    def __init__(self, ops, L: NetLayout, net_handle):
        self.ops, self.L, self.net = ops, L, net_handle
        self.flat = ops.zeros(L.n_params_padded)
        self.eff = ops.zeros(max(L.n_eff, 4)) if L.noisy else None
        # noise vectors in KERNEL order (noise_in of first_dense permuted to (h,w,c))
        # All of them live in ONE buffer, in the order reset_noise draws them and each padded to a multiple of four floats — the stride of
        # the Philox offsets (DeviceRng._advance) — so a single normal fill over the buffer produces exactly the draws of nine fills.
        self.noise: Dict[str, Dict[str, torch.Tensor]] = {}
        sizes = [(prefix, leaf, n) for prefix, block, r0, r1, in_f in L.noise_modules
                 for leaf, n in (("noise_in", in_f), ("noise_out_weight", r1 - r0), ("noise_out_bias", r1 - r0))]
        self.noise_buf = ops.zeros(max(sum((n + 3) // 4 * 4 for _, _, n in sizes), 4))
        off = 0
        for prefix, leaf, n in sizes:
            self.noise.setdefault(prefix, {})[leaf] = self.noise_buf[off:off + n]
            off += (n + 3) // 4 * 4
        self.noise_len = off
        self._noise_sizes = sizes
        self._scratch: Optional[torch.Tensor] = None
        # fused per-observation encoder (encoder_fused.hip): needs k-major copies of the conv weights, refreshed when they change
        self.fused = bool(ops.fused_supported(L.C, L.H, L.W))
        self.fused_dgrad = self.fused and bool(ops.dgrad_fused_supported(L.C, L.H, L.W))
        self.wt = ops.zeros(ops.conv_wt_floats(L.C)) if self.fused else None
        self.fc1_planes = self.actor_fc1_planes = None       # the actor's laid-out copies of fc1's weights (refresh_fc1_planes / refresh_actor_fc1_planes allocate them)

    def adopt_noise_buf(self, buf: torch.Tensor):
        """Move the noise vectors into ``buf`` (noise_len floats of a buffer the caller owns): the learner puts its two networks' vectors back to back, in
        draw order, so that ONE normal fill serves both resets of a train call (agent.py:125-127)."""
        assert buf.numel() >= self.noise_len
        buf[: self.noise_len].copy_(self.noise_buf[: self.noise_len])
        self.noise_buf = buf[: self.noise_len]
        off = 0
        for prefix, leaf, n in self._noise_sizes:
            self.noise[prefix][leaf] = buf[off:off + n]
            off += (n + 3) // 4 * 4

    def refresh_wt(self):
        if self.fused:
            self.ops.conv_wt_refresh(self.encoder_weights(), self.L.C, self.wt)

    def copy_from(self, other: "DeviceNet"):
        """Device-to-device snapshot of another DeviceNet of the same layout: parameters, k-major conv copies, NoisyNet noise
        vectors and composed weights.  This is what replaces shipping ``state_dict()`` to an actor (launch.py:34-36,58-62)."""
        self.flat.copy_(other.flat)
        if self.wt is not None:
            self.wt.copy_(other.wt)
        if self.eff is not None:
            self.eff.copy_(other.eff)
        if self.noise:
            self.noise_buf.copy_(other.noise_buf)

    # ------------------------------------------------------------------ weights
    def block(self, name: str) -> Block:
        return self.L.blocks[name]

    def wb(self, name: str):
        """(W, b) views of the EFFECTIVE weights of a dense layer (composed ones for NoisyNet)."""
        if self.L.noisy and name in ("fc1", "head"):
            blk, buf = self.L.eff[name], self.eff
        else:
            blk, buf = self.L.blocks[name], self.flat
        return buf[blk.w], buf[blk.b]

    def encoder_weights(self):
        f, B = self.flat, self.L.blocks
        return {"w1": f[B["conv1"].w], "b1": f[B["conv1"].b], "w2": f[B["conv2"].w], "b2": f[B["conv2"].b], "w3": f[B["conv3"].w], "b3": f[B["conv3"].b]}

    def compose_mods(self):
        L = self.L
        mods = []
        for prefix, block, r0, r1, in_f in L.noise_modules:
            mu, sg, ef = L.blocks[block + ".mu"], L.blocks[block + ".sigma"], L.eff[block]
            nz = self.noise[prefix]
            mods.append((self.flat[mu.all], self.flat[sg.all], self.eff[ef.all], mu.N, mu.K, r0, r1, nz["noise_in"], nz["noise_out_weight"], nz["noise_out_bias"]))
        return mods

    def compose_noise(self):
        """NoisyLinear.reset_noise's weight_epsilon/bias_epsilon + forward composition (model.py:54-62,78-83)."""
        mods = self.compose_mods()
        if mods:
            self.ops.noisy_multi(False, mods)              # the two or three modules in one launch

    def set_noise(self, prefix: str, noise_in, noise_out_weight, noise_out_bias):
        """Install the three noise vectors of one NoisyLinear (reference order/layout; model.py:73-76)."""
        nz = self.noise[prefix]
        dev = self.flat.device
        nz["noise_in"].copy_(self.L.noise_in_to_kernel(prefix, torch.as_tensor(noise_in, dtype=torch.float32).to(dev)))
        nz["noise_out_weight"].copy_(torch.as_tensor(noise_out_weight, dtype=torch.float32).to(dev))
        nz["noise_out_bias"].copy_(torch.as_tensor(noise_out_bias, dtype=torch.float32).to(dev))

    def load_state_dict(self, sd):
        """Reference-format state_dict (keys/shapes of agent0/deepq/model.py) -> packed device parameters."""
        dev = self.flat.device
        sd = {k: torch.as_tensor(v).to(dev) for k, v in sd.items()}
        self.L.pack(sd, self.flat)
        self.refresh_wt()
        for prefix, *_ in self.L.noise_modules:
            if f"{prefix}.noise_in" in sd:
                self.set_noise(prefix, sd[f"{prefix}.noise_in"], sd[f"{prefix}.noise_out_weight"], sd[f"{prefix}.noise_out_bias"])
        if self.L.noisy:
            self.compose_noise()

    def state_dict(self):
        """Packed device parameters -> reference-format entries (trainables + NoisyNet buffers)."""
        out = self.L.unpack(self.flat)
        for prefix, *_ in self.L.noise_modules:
            nz = self.noise[prefix]
            nin = self.L.noise_in_from_kernel(prefix, nz["noise_in"]).clone()
            f = lambda x: x.sign() * x.abs().sqrt()
            out[f"{prefix}.weight_epsilon"] = torch.outer(f(nz["noise_out_weight"]), f(nin))
            out[f"{prefix}.bias_epsilon"] = f(nz["noise_out_bias"])
            out[f"{prefix}.noise_in"] = nin
            out[f"{prefix}.noise_out_weight"] = nz["noise_out_weight"].clone()
            out[f"{prefix}.noise_out_bias"] = nz["noise_out_bias"].clone()
        return out

    def scratch(self, n: int) -> Optional[torch.Tensor]:
        if n <= 0:
            return None
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = self.ops.empty(n)
        return self._scratch

    # ------------------------------------------------------------------ forward
    def encode(self, ws: Workspace, frames, slot, sample_stride, chan_off, B, keep: bool = True):
        """frames -> act3 (and act1/act2 when ``keep``: only a pass that is differentiated needs them in HBM)."""
        if self.fused:
            self.ops.encoder_fwd_fused(self.net, self.wt, self.encoder_weights(), frames, slot, sample_stride, chan_off, B,
                                       ws.act1 if keep else None, ws.act2 if keep else None, ws.act3)
        else:
            self.ops.encoder_fwd(self.net, self.encoder_weights(), frames, slot, sample_stride, chan_off, B, ws.act1, ws.act2, ws.act3)

    def dense_splits(self, name, R) -> int:
        """The split-K count ``_dense`` uses for layer ``name`` over ``R`` rows."""
        blk = self.L.eff[name] if (self.L.noisy and name in ("fc1", "head")) else self.L.blocks[name]
        return self.ops.dense_fwd_splits(R, blk.N, blk.K)

    def _dense(self, X, ldx, name, Y, R, relu, splits: Optional[int] = None):
        """``splits``: the split-K count to use instead of the shape's own (a grouped actor step passes the full batch's, ``Actor._split_plan``)."""
        W, b = self.wb(name)
        blk = self.L.eff[name] if (self.L.noisy and name in ("fc1", "head")) else self.L.blocks[name]
        N, K = blk.N, blk.K
        if splits is not None:
            self.ops.dense_fwd_n(X, ldx, W, b, Y, R, N, K, relu, splits, self.scratch(splits * R * N if splits > 1 else 0))
            return
        self.ops.dense_fwd(X, ldx, W, b, Y, R, N, K, relu, self.scratch(self.ops.dense_fwd_scratch(R, N, K)))

    def head(self, ws: Workspace, B, taus: Optional[torch.Tensor] = None, n_tau: int = 1, feat: Optional[torch.Tensor] = None):
        """features -> q.  Dense algos: q [B][A][T].  Quantile algos: taus [B*n_tau] -> q [B][n_tau][A].
        ``feat`` overrides ws.act3 (evaluating a head on another pass's features)."""
        L, ops = self.L, self.ops
        feat = ws.act3 if feat is None else feat
        if not L.quantile:
            self._dense(feat, L.feat, "fc1", ws.h, B, True)
            self._dense(ws.h, 512, "head", ws.raw, B, False)
            ops.dueling_fwd(ws.raw, L.Npad, ws.q, B, L.A, L.T, L.dueling)
            return ws.q
        R = B * n_tau
        ops.cos_features(taus, ws.cosx, R, L.num_cosines)
        if not ws.grads and ops.dense_fwd_scratch(R, L.feat, L.num_cosines) == 0:
            # a pass that is not differentiated: embedding x features in the GEMM's epilogue, the embedding never reaches HBM
            Wc, bc = self.wb("cos")
            ops.dense_fwd_mul(ws.cosx, L.num_cosines, Wc, bc, feat, n_tau, ws.x, R, L.feat, L.num_cosines, True)
        elif ws.grads and ops.dense_fwd_mul_keep_ok(R, L.feat, L.num_cosines, L.num_cosines):
            # the differentiated pass: the embedding is kept for the backward pass, embedding x features written beside it in the same launch
            Wc, bc = self.wb("cos")
            ops.dense_fwd_mul_keep(ws.cosx, L.num_cosines, Wc, bc, feat, n_tau, ws.emb, ws.x, R, L.feat, L.num_cosines, True)
        else:
            self._dense(ws.cosx, L.num_cosines, "cos", ws.emb, R, True)
            ops.hadamard_fwd(ws.emb, feat, ws.x, B, n_tau, L.feat)
        self._dense(ws.x, L.feat, "fc1", ws.h, R, True)
        self._dense(ws.h, 512, "head", ws.raw, R, False)
        ops.dueling_fwd(ws.raw, L.Npad, ws.q, R, L.A, 1, L.dueling)
        return ws.q

    def refresh_fc1_planes(self):
        """fc1's EFFECTIVE weights as bf16 term planes (a0_split_planes) for ``head_slabs(.., w_planes=True)``: the actor refreshes them when a rollout starts and after
        every NoisyNet compose, and reuses them for the rollout's GEMMs of E * K rows (same exact terms as the GEMM would form per tile: same bits)."""
        W, _ = self.wb("fc1")
        if self.fc1_planes is None:
            self.fc1_planes = torch.empty(self.ops.weight_planes_words(512, self.L.feat), dtype=torch.int32, device=self.flat.device)
        self.ops.split_planes(W, self.fc1_planes, 512, self.L.feat)

    def refresh_actor_fc1_planes(self):
        """fc1's EFFECTIVE weights as fragment-ordered bf16 term planes (a0_actor_fc1_planes) for the scalar and c51 / qr actors' per-step fc1 (a0_actor_fc1_kernel):
        refreshed like ``refresh_fc1_planes``, when a rollout starts and after every NoisyNet compose."""
        W, _ = self.wb("fc1")
        if self.actor_fc1_planes is None:
            self.actor_fc1_planes = torch.empty(self.ops.actor_fc1_planes_words(512, self.L.feat), dtype=torch.int32, device=self.flat.device)
        self.ops.actor_fc1_planes(W, self.actor_fc1_planes, 512, self.L.feat)

    def head_slabs(self, ws: Workspace, B, taus: torch.Tensor, n_tau: int, slabs: torch.Tensor, cos_ready: bool = False, w_planes: bool = False,
                   splits: Optional[dict] = None) -> int:
        """Quantile heads of a pass that is not differentiated, up to the head GEMM's split-K slabs [ns][B * n_tau][Npad] (the consumer kernel finishes
        the layer: a0_actor_quantile_tail_env_step / a0_actor_quantile_tail).  Returns the slab count.  ``cos_ready``: ``ws.cosx`` already holds the fractions' cosine
        features (the launch that produced the fractions wrote them: a0_tau_cos_features / a0_fqf_taus_cos).  ``splits``: {"fc1": n, "head": n} — the split counts of
        another row count's launches (a grouped actor step: the full batch's)."""
        L, ops = self.L, self.ops
        R = B * n_tau
        if not cos_ready:
            ops.cos_features(taus, ws.cosx, R, L.num_cosines)
        Wc, bc = self.wb("cos")
        ops.dense_fwd_mul(ws.cosx, L.num_cosines, Wc, bc, ws.act3, n_tau, ws.x, R, L.feat, L.num_cosines, True)
        if w_planes:      # ``refresh_fc1_planes`` has run since fc1's effective weights last changed
            ops.dense_fwd_wplanes(ws.x, L.feat, self.fc1_planes, self.wb("fc1")[1], ws.h, R, 512, L.feat, True)
        else:
            self._dense(ws.x, L.feat, "fc1", ws.h, R, True, splits=None if splits is None else splits["fc1"])
        Wh, _ = self.wb("head")
        if splits is not None:
            return ops.dense_fwd_partial_n(ws.h, 512, Wh, R, L.Npad, 512, splits["head"], slabs)
        return ops.dense_fwd_partial(ws.h, 512, Wh, R, L.Npad, 512, slabs)

    def fc1(self, ws: Workspace, B):
        """features -> relu(fc1) only (the fused DQN head kernel takes it from there)."""
        self._dense(ws.act3, self.L.feat, "fc1", ws.h, B, True)

    def fqf_taus(self, ws: Workspace, B, with_cos: bool = False, splits: Optional[int] = None):
        """FQFHead.prop_taus (model.py:268-278): fraction net on (detached) features -> taus, tau_hats (``with_cos``: and the tau_hats' cosine features into ``ws.cosx``).
        ``splits``: the fraction GEMM's split count (see ``_dense``)."""
        L = self.L
        self._dense(ws.act3, L.feat, "frac", ws.frac_logits, B, False, splits=splits)
        if with_cos:
            self.ops.fqf_taus_cos(ws.frac_logits, L.Fpad, ws.tau_all, ws.tau_hat, ws.cosx, L.num_cosines, B, L.F)
        else:
            self.ops.fqf_taus(ws.frac_logits, L.Fpad, ws.tau_all, ws.tau_hat, B, L.F)

    def select(self, ws: Workspace, B, n_tau, a_star, qsel=None, qmax=None, atoms=None):
        """argmax_a head.qval (greedy action) from the activations in ``ws``."""
        L, ops = self.L, self.ops
        if L.algo in ("dqn", "mdqn"):
            ops.select_action(ws.q, L.A, 1, 1, B, L.A, 1, MODE_IDENT, None, a_star, qsel, qmax)
        elif L.algo == "qr":
            ops.select_action(ws.q, L.A * L.T, L.T, 1, B, L.A, L.T, MODE_MEAN, None, a_star, qsel, qmax)
        elif L.algo == "c51":
            ops.select_action(ws.q, L.A * L.T, L.T, 1, B, L.A, L.T, MODE_C51, atoms, a_star, qsel, qmax)
        elif L.algo == "iqn":
            ops.select_action(ws.q, n_tau * L.A, 1, L.A, B, L.A, n_tau, MODE_MEAN, None, a_star, qsel, qmax)
        else:  # fqf: sum_i (tau_{i+1} - tau_i) q(tau_hat_i)
            ops.select_action(ws.q, n_tau * L.A, 1, L.A, B, L.A, n_tau, MODE_FQF, ws.tau_all, a_star, qsel, qmax)


class _Upd:
    """One update's per-call context (the handle's ``a0_upd``): the batch as every pass reads it (``_upd_prepare`` re-points it at the shifted copy under
    learner.aug_shift; ``backward_encoder`` reads it again), and what the family's forward left: ``have_draw`` / ``have_dh`` — the loss launch wrote the head
    output's gradient / the head's data gradient itself — and fqf's fraction loss."""
    __slots__ = ("frames", "slot", "stride", "act", "rew", "done", "wgt", "rand", "tstage", "have_draw", "have_dh", "frac")

    def __init__(self, frames, slot, stride, act, rew, done, wgt, rand, tstage):
        self.frames, self.slot, self.stride, self.act, self.rew, self.done, self.wgt, self.rand, self.tstage = frames, slot, stride, act, rew, done, wgt, rand, tstage
        self.have_draw, self.have_dh, self.frac = False, False, None


class DeviceLearner:
    """Online + target network, gradients, Adam / RMSprop state and the per-algorithm update."""
    SHAPE_PREDICATES = ("dense_fwd_partial_multi_ok", "dense_dgrad_wgrad_ok", "dense_dgrad_wgrad_ok2", "dense_dgrad_wgrad2_ok", "dense_dgrad_hadamard_ok")

    def __init__(self, ops, L: NetLayout, batch_size: int, *, discount=0.99, n_step=1, double_q=False, lr=5e-4,
                 target_update_freq=500, vmin=-10.0, vmax=10.0, K=32, N=64, N_dash=64, max_grad_norm=-1.0, adam_eps=None,
                 mdqn_tau=0.03, mdqn_lo=-1.0, clip_grad_norm=-1.0, target_tau=0.0, aug_shift=0, aug_rng=None, net_reset_freq=0, net_reset_shrink=1.0,
                 weight_decay=0.0, redo_freq=0, redo_tau=0.1, redo_recycle=True, rank_freq=0, rank_delta=0.01, munchausen=False, mdqn_alpha=0.9, hl_gauss=0.0,
                 risk="neutral", risk_eta=0.0):
        self.ops, self.L, self.B = ops, L, batch_size
        self.net = ops.net(L.C, L.H, L.W)
        self.online = DeviceNet(ops, L, self.net)
        self.target = DeviceNet(ops, L, self.net)
        self.noise_joint = None
        if L.noisy and self.online.noise_len % 4 == 0:
            # both networks' noise vectors back to back in the order a train call draws them (online, then target: agent.py:125-127)
            n = self.online.noise_len
            self.noise_joint = ops.zeros(2 * n)
            self.online.adopt_noise_buf(self.noise_joint[:n])
            self.target.adopt_noise_buf(self.noise_joint[n:])
        self.grads = ops.zeros(L.n_params_padded + 4)     # tail slot [n_params_padded]: the NaN flag as a float, reduced with the dense bucket
        self.adam_m = ops.zeros(L.n_params_padded)
        self.adam_v = ops.zeros(L.n_params_padded)
        self.state = ops.zeros(8, dtype=torch.int32)
        self.scalars = ops.zeros(4)
        # batch means of the last 1024 updates' per-sample losses, written by the Adam launch itself (a0_adam_step_sync_wt: ring slot = state[6] % 1024)
        self.loss_ring = ops.zeros(1024)
        # learner.clip_grad_norm > 0: the gradient Adam steps on is scaled to this global L2 norm (torch.nn.utils.clip_grad_norm_); the pre-clip norm of every
        # update goes to gnorm_ring, slot for slot beside loss_ring.  Off (<= 0): neither buffer exists and apply() issues what it always did.
        self.clip_grad_norm = clip_limit(clip_grad_norm)
        self.gnorm_partials = ops.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64) if self.clip_grad_norm > 0 else None
        self.gnorm_ring = ops.zeros(1024) if self.clip_grad_norm > 0 else None
        # learner.target_tau in (0, 1): the Adam forms get the period 0 (never a hard copy) and one launch behind them blends the target towards the online network at
        # the updates the period names (a0_target_blend).  Off (0.0): apply() issues what it always did.
        self.target_tau = target_tau_value(target_tau)
        # learner.aug_shift = p > 0: forward_dense first shifts the batch into aug_stage (a0_augment_shift: Philox stream 7 of aug_rng.seed — the learner's DeviceRng — at
        # the update count state[6]) and every pass reads that dense batch.  Off (0): no buffer, no launch, and the passes get the arguments they always got.
        self.aug_shift = aug_shift_value(aug_shift, (L.C, L.H, L.W))
        self.aug_rng, self.aug_stage = aug_rng, None
        if self.aug_shift > 0:
            if not self.online.fused:
                # adam_step_sync / adam_step_sync_clip, the forms behind the unfused encoder, file no loss mean and so never advance state[6]: every update would repeat update 0's shifts
                raise ValueError(f"learner.aug_shift={self.aug_shift}: needs observations the fused encoder kernels cover — only their Adam forms advance the update count the shifts are drawn by")
            if aug_rng is None or not hasattr(ops, "augment_shift"):
                raise ValueError(f"learner.aug_shift={self.aug_shift}: needs the learner's DeviceRng (aug_rng) and a backend with augment_shift")
            self.aug_stage = ops.empty(batch_size * 2 * L.C * L.H * L.W, dtype=torch.uint8)
        # learner.net_reset_freq = N > 0: apply() ends with one launch more (a0_net_reset) that re-initialises the network after every N-th successful update and returns
        # at once otherwise.  The fresh values come from Philox stream 8 of the low 32 bits of aug_rng.seed — the learner's DeviceRng, so a loaded snapshot's seed is
        # followed — unless net_reset_seed names another one (data parallelism: every rank takes rank 0's).  Off (0): no table, no launch.
        self.net_reset_freq, self.net_reset_shrink = net_reset_value(net_reset_freq, net_reset_shrink)
        self.net_reset_seed = None
        self.reset_segs = None
        if self.net_reset_freq > 0:
            if aug_rng is None or not hasattr(ops, "net_reset"):
                raise ValueError(f"learner.net_reset_freq={self.net_reset_freq}: needs the learner's DeviceRng (aug_rng) and a backend with net_reset")
            self.reset_segs = L.reset_segments()
        # learner.weight_decay = lambda > 0: apply() shrinks everything Adam owns by c = fl32(lr * lambda) in one launch in front of the Adam form (a0_weight_decay),
        # which also leaves the sums of squares of the values it read in wd_partials (the statistic ``param_norm``).  That launch reads the NaN flag the one-launch
        # tail's bookkeeping would have lowered, so the update takes the three-launch tail, as under clipping.  Off (0.0): no buffer, no launch.
        self.wd_coef = weight_decay_value(weight_decay, lr)
        self.weight_decay = float(weight_decay) if self.wd_coef > 0 else 0.0
        self.wd_partials = None
        if self.wd_coef > 0:
            if not hasattr(ops, "weight_decay"):
                raise ValueError(f"learner.weight_decay={weight_decay!r}: needs a backend with weight_decay")
            self.wd_partials = ops.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64)
        # learner.redo_freq = N > 0: apply() issues two launches more (a0_redo_score) that leave the dormancy scores, the mask and the counts of the 672 hidden neurons
        # after every N-th successful update, and with learner.redo_recycle a third (a0_redo_recycle) that recycles the dormant ones — between the blend and the
        # reset launch; all return at once on other updates.  Fresh values: Philox stream 9 of the seed ``reset_seed()`` names.  Off (0): no buffer, no launch.
        self.redo_freq, self.redo_tau, self.redo_recycle = redo_value(redo_freq, redo_tau, redo_recycle, noisy=L.noisy)
        self.redo_partials = self.redo_scores = self.redo_mask = self.redo_counts = self.redo_segs = None
        if self.redo_freq > 0:
            if not hasattr(ops, "redo_score") or (self.redo_recycle and aug_rng is None):
                raise ValueError(f"learner.redo_freq={self.redo_freq}: needs a backend with redo_score and, to recycle, the learner's DeviceRng (aug_rng)")
            self.redo_partials = ops.empty(ops.REDO_PARTIALS * ops.REDO_NEURONS, dtype=torch.float64)
            self.redo_scores, self.redo_mask = ops.zeros(ops.REDO_NEURONS), ops.zeros(ops.REDO_NEURONS, dtype=torch.int32)
            self.redo_counts = ops.zeros(8, dtype=torch.int32)
            self.redo_counts[5] = -1                   # never evaluated
            if self.redo_recycle:
                self.redo_segs = L.reset_segments()
        # learner.rank_freq = N > 0: apply() issues two launches more (a0_feature_rank) that leave the singular values of the fc1 activations and their srank after
        # every N-th successful update — behind the blend, in front of the dormancy and reset launches; both return at once on other updates and write nothing the
        # update uses.  Off (0): no buffer, no launch.
        self.rank_freq, self.rank_delta = rank_value(rank_freq, rank_delta)
        self.rank_gram = self.rank_spectrum = self.rank_result = None
        self.rank_views = None          # a learner handle's own (spectrum, result) while NativeLoop drives the updates: what feature_spectrum() then reads
        if self.rank_freq > 0:
            if not hasattr(ops, "feature_rank"):
                raise ValueError(f"learner.rank_freq={self.rank_freq}: needs a backend with feature_rank")
            self.rank_gram = ops.empty(ops.RANK_GRAM_DOUBLES, dtype=torch.float64)
            self.rank_spectrum = ops.zeros(ops.RANK_FEATURES, dtype=torch.float64)
            self.rank_result = ops.zeros(8, dtype=torch.int32)
            self.rank_result[2] = -1                   # never evaluated
        # learner.iqn.munchausen: _fwd_iqn builds the quantile targets with miqn_target from the target network's passes on s' and on s (``ws_m``, B * N' rows) instead of
        # the greedy quantile_target; tau, alpha, lo are learner.mdqn's (alpha is honoured here; mdqn leaves it unused, quirk Q17).  Off: no buffer, and _fwd_iqn issues
        # what it always did.  (For mdqn the numbers were never checked here and still are not.)
        self.munchausen, self.mdqn_alpha = False, float(mdqn_alpha)
        if munchausen:
            self.munchausen, _, self.mdqn_alpha, _ = munchausen_value(munchausen, mdqn_tau, mdqn_alpha, mdqn_lo, algo=L.algo, double_q=double_q)
            if not hasattr(ops, "miqn_target"):
                raise ValueError("learner.iqn.munchausen=true: needs a backend with miqn_target")
        # learner.iqn.risk: _fwd_iqn distorts the K selection fractions of the greedy next action into ``t_risk`` (B * K floats, the engine's own: ``u.rand`` is only
        # read) with one risk_distort launch, and the selection pass reads that.  Off (neutral): no buffer, and _fwd_iqn issues what it always did.  The setting is
        # fixed once an update has been issued (``set_risk``).
        self.risk_kind, self.risk_eta, self.t_risk, self._risk_fixed = 0, 0.0, None, False
        self.set_risk(risk, risk_eta, K=K)
        # learner.c51.hl_gauss = rho > 0: _fwd_dist ends with c51_hl_gauss_head_loss_slabs — the Gaussian histogram of the scalar TD target in the projected
        # distribution's place — instead of c51_head_loss_slabs; hl_gauss_sigma = rho * Delta is the double the kernel receives.  A staged target pass (tstage) is
        # allowed: it ends at the fc1 slabs.  Off (0.0): _fwd_dist issues what it always did.
        self.hl_gauss, self.hl_gauss_sigma = hl_gauss_value(hl_gauss, vmin, vmax, L.T, algo=L.algo) if hl_gauss else (0.0, 0.0)
        if self.hl_gauss > 0 and not hasattr(ops, "c51_hl_gauss_head_loss_slabs"):
            raise ValueError(f"learner.c51.hl_gauss={self.hl_gauss!r}: needs a backend with c51_hl_gauss_head_loss_slabs")
        self.discount, self.n_step, self.double_q = discount, n_step, double_q
        self.gamma_n = float(discount ** n_step)
        self.lr, self.target_update_freq = lr, target_update_freq
        self.adam_eps = (1e-2 / batch_size) if adam_eps is None else adam_eps
        self.vmin, self.vmax = float(vmin), float(vmax)
        self.K, self.N, self.N_dash = K, N, N_dash
        self.max_grad_norm = max_grad_norm
        self.mdqn_tau, self.mdqn_lo = float(mdqn_tau), float(mdqn_lo)
        self.family = self._family()
        B = batch_size
        self.ws_m = self.atoms = self._fc1_slabs = self._q_cur = self._dist_buf = None
        if L.quantile:
            n_on = N if L.algo == "iqn" else L.F
            n_tg = N_dash if L.algo == "iqn" else L.F
            n_sel = K if L.algo == "iqn" else L.F
            self.ws_o = Workspace(ops, L, B, n_on, grads=True)
            self.ws_t = Workspace(ops, L, B, max(n_tg, n_sel))
            self.ws_s = Workspace(ops, L, B, n_sel) if double_q else None
            if self.munchausen:
                self.ws_m = Workspace(ops, L, B, n_tg)      # the target network on the CURRENT observation at the N' target fractions
            if L.algo == "fqf":
                self.ws_f = Workspace(ops, L, B, L.F)        # q at taus[1:-1] for the fraction loss (F-1 used)
                self.rms_sq = ops.zeros(L.blocks["frac"].size)
                self.frac_loss = ops.empty(B)
                self.dfrac_logits = ops.zeros(B * L.Fpad)
                self.clip = ops.zeros(1)
            self.y = ops.empty(B * n_tg)
        else:
            self.ws_o = Workspace(ops, L, B, grads=True)
            self.ws_t = Workspace(ops, L, B)
            self.ws_s = Workspace(ops, L, B) if double_q else None
            if L.algo == "qr":
                self.y = ops.empty(B * L.T)
                self.qr_taus = ((2 * torch.arange(L.T, dtype=torch.float32) + 1) / (2.0 * L.T)).to(ops.device)
            if L.algo == "mdqn":
                self.ws_m = Workspace(ops, L, B)
        if L.algo == "c51":
            self.atoms = torch.linspace(self.vmin, self.vmax, L.T).to(ops.device)
            self.m_proj = ops.empty(B * L.T)
        if self.family == "scalar":
            # the passes' fc1 split-K slabs, which the head / loss kernel finishes: online on s, target on s', and the third pass's (double-Q; mdqn)
            n = ops.dense_fwd_partial_slabs(B, 512, L.feat) * B * 512
            self._fc1_slabs = [ops.empty(n) for _ in range(3 if double_q or L.algo == "mdqn" else 2)]
            self._q_cur = ops.empty(B * L.A) if L.algo == "mdqn" else None
        elif self.family == "dist":
            self._ws_dist()
        self._tst = {}         # A0_PIPELINE_TARGET=1: the separately staged target pass's buffers, per parity (``_tstage_buf``)
        self.a_star = ops.zeros(B, dtype=torch.int32)
        self.loss = ops.empty(B)
        n_slab = max(ops.encoder_bwd_scratch(self.net, B),
                     ops.dense_wgrad_scratch(self.ws_o.R, L.Npad, 512), ops.dense_wgrad_scratch(self.ws_o.R, 512, L.feat),
                     ops.dense_wgrad_scratch(self.ws_o.R, L.feat, L.num_cosines) if L.quantile else 0,
                     ops.dense_wgrad_scratch(B, L.Fpad, L.feat) if L.algo == "fqf" else 0, 4)
        # head + fc1 (+ cosine embedding) reduce in disjoint regions of one launch
        shapes = [(self.ws_o.R, L.Npad, 512), (self.ws_o.R, 512, L.feat)] + ([(self.ws_o.R, L.feat, L.num_cosines)] if L.quantile else [])
        n_slab = max(n_slab, ops.dense_wgrad_multi_scratch(shapes))
        # Round 4: without a gradient hook the dense layers' slab reductions ride in the encoder weight gradients' reduction launch (a0_pending_reduce: one launch less
        # per update, same sums) — their slabs then have to survive until that launch, so the encoder's get a region of their own behind them
        self._enc_slab_off, self._defer_dense = 0, False
        if self.online.fused and self.online.fused_dgrad and os.environ.get("A0_DEFER_DENSE_REDUCE", "1") != "0":
            self._enc_slab_off, self._defer_dense = ops.dense_wgrad_multi_scratch(shapes), True
            n_slab = max(n_slab, self._enc_slab_off + ops.encoder_bwd_scratch(self.net, B))
        self._pend = None
        # the update's tail as one launch (ops.update_tail: slab sums, Adam, target copy, weight copies); without the deferred sums the three launches are composed
        self.fused_tail = self._defer_dense
        self._tail_plan = self._upd = None
        # the grouped / paired launches' shape predicates, looked up once: HipOps and CpuOps have all five (a test holds them to the names); a backend without such a launch answers no
        self._ok = {n: getattr(ops, n, lambda *shape: False) for n in self.SHAPE_PREDICATES}
        self.slabs = ops.empty(n_slab)
        self.obs_bytes = L.C * L.H * L.W
        self.grad_hook = None       # data parallelism: callable(grads, state) run between backward and the optimizer (dist.GradAllReduce)

    # ------------------------------------------------------------------ helpers
    def sync_target(self, force=True):
        self.ops.target_sync(self.target.flat, self.online.flat, self.L.n_params_padded, self.state, force)
        self.target.refresh_wt()

    def _hard_freq(self) -> int:
        """The target period the Adam forms get: 0 — their "never sync" — while learner.target_tau is on."""
        return 0 if self.target_tau > 0 else self.target_update_freq

    def _blend_target(self, force=False):
        """learner.target_tau: one launch behind the update's Adam form; it blends when the committed step count is a multiple of the period (or ``force``) and returns
        at once otherwise.  The target's weight copies follow when the encoder runs in the fused kernels."""
        if self.target_tau <= 0:
            return
        L, tg = self.L, self.target
        self.ops.target_blend(tg.flat, self.online.flat, L.n_params_padded, self.target_tau, self.state, self.target_update_freq, force,
                              *((tg.encoder_weights(), L.C, tg.wt) if tg.fused else ()))

    def reset_seed(self) -> int:
        """The 32-bit seed of learner.net_reset_freq's fresh values: ``net_reset_seed`` when one was set (rank 0's, under data parallelism), else the low 32 bits of
        the learner's DeviceRng seed as it stands now."""
        return int(self.net_reset_seed if self.net_reset_seed is not None else self.aug_rng.seed) & 0xFFFFFFFF

    def _reset_net(self, force=False, k_host=0):
        """learner.net_reset_freq: the update's last launch, behind the Adam form and the blend; it resets when this update was not NaN-skipped and left the step count
        a positive multiple of the period (or ``force``, as reset number ``k_host``) and returns at once otherwise."""
        if self.net_reset_freq <= 0:
            return
        L, on, tg = self.L, self.online, self.target
        self.ops.net_reset(on.flat, tg.flat, self.adam_m, self.adam_v, L.n_adam, L.n_params_padded, self.reset_segs, self.net_reset_shrink, self.reset_seed(), self.state,
                           self.net_reset_freq, force, k_host, *((on.encoder_weights(), L.C, on.wt, tg.wt) if on.fused else ()))

    def _feature_rank(self, force=False):
        """learner.rank_freq: behind the Adam form and the blend, in front of the dormancy and reset launches — Gram matrix, spectrum and srank of the fc1 activations
        the differentiated pass has left in ``ws_o`` (for iqn / fqf that pass's B * N rows, what ``_redo`` scores); the two launches act when this update was not
        NaN-skipped and left the step count a positive multiple of the period (or ``force``) and return at once otherwise.  They only read the activations."""
        if self.rank_freq <= 0:
            return
        h = self.ws_o.h
        self.ops.feature_rank(h, h.numel() // self.ops.RANK_FEATURES, self.rank_delta, self.state, self.rank_freq, force, self.rank_gram, self.rank_spectrum, self.rank_result)

    def feature_spectrum(self):
        """The 512 singular values (descending, zero under the floor) of the fc1 activations at the newest evaluation of learner.rank_freq as a numpy array — what
        entropy-based or stable rank need; None while the setting is off and before the first evaluation."""
        if self.rank_freq <= 0:
            return None
        spectrum, result = self.rank_views or (self.rank_spectrum, self.rank_result)
        return spectrum.cpu().numpy() if int(result[2]) >= 0 else None

    def _redo(self, force=False, k_host=0):
        """learner.redo_freq: behind the Adam form and the blend, in front of the reset launch — scores, mask and counts from the activations the differentiated pass
        has left in ``ws_o`` (for iqn / fqf the fc1 rows are that pass's B * N rows), then the recycle launch; all of them act when this update was not NaN-skipped and
        left the step count a positive multiple of the period (or ``force``, as recycle number ``k_host``) and return at once otherwise."""
        if self.redo_freq <= 0:
            return
        if self.grad_hook is not None:
            raise ValueError(f"learner.redo_freq={self.redo_freq}: not with a gradient exchange installed (the data-parallel path): the ranks see different batches and "
                             "would draw different dormancy masks")
        L, on, ws = self.L, self.online, self.ws_o
        B = self.B
        rows = (B * L.H1 * L.W1, B * L.H2 * L.W2, B * (L.feat // 64), ws.h.numel() // 512)
        self.ops.redo_score(ws.act1, ws.act2, ws.act3, ws.h, self.redo_tau, self.state, self.redo_freq, force, self.redo_partials, self.redo_scores, self.redo_mask,
                            self.redo_counts, rows)
        if self.redo_recycle:
            self.ops.redo_recycle(on.flat, self.adam_m, self.adam_v, L.n_adam, L.n_params_padded, self.redo_segs, L.redo_blocks(), self.redo_mask, self.reset_seed(), self.state,
                                  self.redo_freq, force, k_host, *((on.encoder_weights(), L.C, on.wt) if on.fused else ()))

    def _grad(self, name: str) -> torch.Tensor:
        L = self.L
        key = name + ".mu" if (L.noisy and name in ("fc1", "head")) else name
        return self.grads[L.blocks[key].all]

    def _backward_dense(self, ws: Workspace, B, have_draw: bool = False, have_dh: bool = False):
        """dq (w.r.t. the combined head output) -> the gradients of every dense block (head, fc1, cosine embedding, NoisyNet sigmas)
        and d3, the gradient w.r.t. the encoder output.  After this call the flat gradient range [L.conv_end, L.n_adam) is final:
        the data-parallel exchange of that range (95 % of the parameters) can run while the encoder backward is still computing."""
        L, ops, on = self.L, self.ops, self.online
        R, T = ws.R, (1 if L.quantile else L.T)
        if not have_draw:
            ops.dueling_bwd(ws.dq, ws.draw, L.Npad, R, L.A, T, L.dueling)
        Wh, _ = on.wb("head")
        Wf, _ = on.wb("fc1")
        # the data gradients first, then every dense weight gradient with ONE slab reduction
        wg = [(ws.draw, ws.h, 512, self._grad("head"), R, L.Npad, 512)]
        if not have_dh:
            if self._ok["dense_dgrad_wgrad_ok2"](R, L.Npad, 512):
                # round 5: a distributional head's data gradient (64 tiles) and weight gradient (32 - 104 tiles) side by side in one launch
                ops.dense_dgrad_wgrad(ws.draw, Wh, ws.h, 512, ws.dh, self._grad("head"), R, L.Npad, 512)
                wg = []
            else:
                ops.dense_dgrad(ws.draw, Wh, ws.h, ws.dh, R, L.Npad, 512)
        if not L.quantile:
            if wg and self._ok["dense_dgrad_wgrad2_ok"](R, 512, L.feat, L.Npad, 512):
                # round 5: ... and the head's weight gradient, which waits for the loss kernel only, in the same launch (its few tiles fill slots the pair leaves empty)
                ops.dense_dgrad_wgrad2(ws.dh, Wf, ws.act3, L.feat, ws.d3, self._grad("fc1"), R, 512, L.feat, ws.draw, ws.h, 512, self._grad("head"), L.Npad, 512)
                wg = []
            elif self._ok["dense_dgrad_wgrad_ok"](R, 512, L.feat):
                # fc1's data gradient and weight gradient — 392 tiles each at R = 512 — as ONE launch that keeps the chip's workgroup slots filled (bit-identical)
                ops.dense_dgrad_wgrad(ws.dh, Wf, ws.act3, L.feat, ws.d3, self._grad("fc1"), R, 512, L.feat)
            else:
                wg.append((ws.dh, ws.act3, L.feat, self._grad("fc1"), R, 512, L.feat))
                ops.dense_dgrad(ws.dh, Wf, ws.act3, ws.d3, R, 512, L.feat)
        else:
            n = ws.n_tau
            wg.append((ws.dh, ws.x, L.feat, self._grad("fc1"), R, 512, L.feat))
            if self._ok["dense_dgrad_hadamard_ok"](R, 512, L.feat, n):
                # round 6: dx = dh W never reaches HBM — the embedding product's backward runs in the data-gradient GEMM's epilogue
                ops.dense_dgrad_hadamard(ws.dh, Wf, ws.emb, ws.act3, ws.demb, ws.d3, R, 512, L.feat, n)
            else:
                ops.dense_dgrad(ws.dh, Wf, None, ws.dx, R, 512, L.feat)
                ops.hadamard_bwd(ws.dx, ws.emb, ws.act3, ws.demb, ws.d3, B, n, L.feat)
            wg.append((ws.demb, ws.cosx, L.num_cosines, self._grad("cos"), R, L.feat, L.num_cosines))
        # data parallelism exchanges the dense range right after this call: its reductions cannot wait for the encoder's launch then
        defer = self._defer_dense and self.grad_hook is None
        self._pend = ops.pending_reduce() if defer else None
        if wg:
            ops.dense_wgrad_multi(wg, self.slabs, **({"pend": self._pend} if defer else {}))
        if L.noisy and not defer:
            self._noisy_sigma_grads()

    def _noisy_sigma_grads(self):
        """d sigma = d eff * eps for every NoisyLinear module, from the (reduced) gradients in the mu blocks."""
        L, on = self.L, self.online
        mods = []
        for prefix, block, r0, r1, in_f in L.noise_modules:
            mu, sg = L.blocks[block + ".mu"], L.blocks[block + ".sigma"]
            nz = on.noise[prefix]
            mods.append((self.grads[mu.all], None, self.grads[sg.all], mu.N, mu.K, r0, r1, nz["noise_in"], nz["noise_out_weight"], nz["noise_out_bias"]))
        self.ops.noisy_multi(True, mods)

    def backward_encoder(self, fuse_tail: bool = False):
        """d3 -> the three convolution blocks' gradients (flat range [0, L.conv_end)); the second half of the backward pass, on the
        batch of the last forward_dense call.  ``fuse_tail``: apply() follows at once, so the slab sums may be left to its launch (ops.update_tail) — not under a
        gradient hook or clipping, which need the summed gradient first, nor under weight decay, whose launch reads the NaN flag the one-launch tail lowers early, nor
        when NoisyNet's sigma gradients wait for deferred dense sums."""
        L, ops, on = self.L, self.ops, self.online
        u, ws, B = self._upd, self.ws_o, self.B
        frames, slot, stride = u.frames, u.slot, u.stride
        g1, g2, g3 = self.grads[L.blocks["conv1"].all], self.grads[L.blocks["conv2"].all], self.grads[L.blocks["conv3"].all]
        self._tail_plan = None
        if on.fused and on.fused_dgrad:
            # both data gradients per observation in one kernel (LDS-resident d2), then the three weight-gradient GEMMs
            ops.encoder_dgrad_fused(self.net, on.wt, ws.d3, ws.act1, ws.act2, B, ws.d2, ws.d1)
            pend, self._pend = self._pend, None
            if (fuse_tail and self.fused_tail and pend is not None and self.grad_hook is None and self.clip_grad_norm <= 0 and self.wd_coef <= 0
                    and not (L.noisy and pend.n > 0)):
                self._tail_plan = ops.encoder_wgrad_tail(self.net, on.encoder_weights(), frames, slot, stride, 0, B, ws.act1, ws.act2, ws.d3, ws.d2, ws.d1, g1, g2, g3,
                                                         self.slabs[self._enc_slab_off:], pend, self.state, self.scalars, self.lr, 0.9, 0.999, self._hard_freq())
                if L.noisy:
                    self._noisy_sigma_grads()
            elif pend is not None:
                ops.encoder_wgrad(self.net, on.encoder_weights(), frames, slot, stride, 0, B, ws.act1, ws.act2, ws.d3, ws.d2, ws.d1, g1, g2, g3, self.slabs[self._enc_slab_off:],
                                  pend=pend)
                if L.noisy:
                    self._noisy_sigma_grads()
            else:
                ops.encoder_wgrad(self.net, on.encoder_weights(), frames, slot, stride, 0, B, ws.act1, ws.act2, ws.d3, ws.d2, ws.d1, g1, g2, g3, self.slabs)
        else:
            ops.encoder_bwd(self.net, on.encoder_weights(), frames, slot, stride, 0, B, ws.act1, ws.act2, ws.d3, ws.d2, ws.d1, g1, g2, g3, self.slabs)

    # ------------------------------------------------------------------ the update
    def update(self, frames, slot, sample_stride, act, rew, done, wgt, rand: Optional[List[torch.Tensor]] = None, tstage: Optional[int] = None):
        """One BaseLearner.train step (agent.py:124-169) on a batch that stays on the device: forward + backward, the data-parallel
        gradient exchange when a ``grad_hook`` is installed, optimizer step.  ``tstage``: the target network's pass on this batch has already
        run into the buffers of that parity (``target_stage``)."""
        out = self.forward_dense(frames, slot, sample_stride, act, rew, done, wgt, rand, tstage=tstage)
        self.exchange_begin()
        self.backward_encoder(fuse_tail=True)
        self.exchange_end()
        self.apply()
        return out

    def _bucketed_hook(self) -> bool:
        return self.grad_hook is not None and getattr(self.grad_hook, "bucketed", False)

    def exchange_begin(self):
        """Data parallelism, first bucket: the dense blocks' gradients are final once forward_dense returns; a hook with a
        ``start_dense`` method (dist.GradAllReduce) reduces them asynchronously while backward_encoder runs."""
        h = self.grad_hook
        if self._bucketed_hook():
            h.start_dense(self.grads, self.L.conv_end, self.L.n_params_padded + 1)

    def exchange_end(self):
        """Second bucket (convolution blocks + the NaN flag) and the join with the first; a plain callable hook gets one call with
        the whole buffer instead."""
        h = self.grad_hook
        if h is None:
            return
        if self._bucketed_hook():
            h.finish(self.grads, None, self.L.conv_end)
        else:
            h(self.grads, self.state)

    def forward_backward(self, frames, slot, sample_stride, act, rew, done, wgt, rand: Optional[List[torch.Tensor]] = None):
        """Losses and every parameter gradient (into ``self.grads``); no parameter is modified (FQF's fraction net aside, which the
        reference also steps separately, agent.py:140-147)."""
        out = self.forward_dense(frames, slot, sample_stride, act, rew, done, wgt, rand)
        self.backward_encoder()
        return out

    def apply(self):
        """Adam on the flat buffer (NaN-skip and step counter on the device), refresh of the fused kernels' weight copies, target sync — with learner.weight_decay on
        behind the decay launch, with learner.target_tau on, the
        blend of the target (``_blend_target``) behind whichever Adam form ran, with learner.rank_freq on the feature-rank launches (``_feature_rank``) and with
        learner.redo_freq on the dormancy launches (``_redo``) behind that, and with
        learner.net_reset_freq on the reset launch (``_reset_net``) last."""
        L, ops, on, tg = self.L, self.ops, self.online, self.target
        if L.algo == "fqf":           # unconditional, like the reference's fqf_optimizer.step() in front of the NaN guard (agent.py:139-148)
            blk = L.blocks["frac"]
            ops.rmsprop_step(on.flat[blk.all], self.grads[blk.all], self.rms_sq, blk.size, self.lr / 2e4, 0.95, 1e-5, self.max_grad_norm, self.clip)
        plan, self._tail_plan = self._tail_plan, None
        adam = (on.flat, self.grads, self.adam_m, self.adam_v, L.n_adam, self.state, self.scalars, self.lr, 0.9, 0.999, self.adam_eps, self._hard_freq(), tg.flat,
                L.n_params_padded, self.grads[L.n_params_padded: L.n_params_padded + 1] if self._bucketed_hook() else None)
        wt = (on.encoder_weights(), L.C, on.wt, tg.wt, self.loss, self.B, self.loss_ring) if on.fused else ()
        if self.wd_coef > 0:
            # learner.weight_decay: everything Adam owns shrinks first, unless this update is NaN-skipped (the launch reads the flags the Adam form behind it reads);
            # the Adam form then files the weight copies and the target from final values
            ops.weight_decay(on.flat, L.n_adam, self.wd_coef, self.state, adam[-1], self.wd_partials)
        if plan is not None:
            # backward_encoder(fuse_tail=True) left the slab sums and the step's bookkeeping to this launch
            ops.update_tail(on.flat, self.grads, self.adam_m, self.adam_v, L.n_adam, self.state, self.scalars, 0.9, 0.999, self.adam_eps, tg.flat, L.n_params_padded, plan, *wt)
        elif self.clip_grad_norm > 0:
            # one launch more: the sum of squares over everything Adam owns (the fqf fraction net lies behind n_adam), taken here — behind the data-parallel
            # exchange — so that every rank derives the same coefficient; the Adam launch finishes the norm, clips and files it (a0_adam_step_sync_clip)
            ops.grad_norm_partials(self.grads, L.n_adam, self.gnorm_partials)
            (ops.adam_step_sync_wt_clip if on.fused else ops.adam_step_sync_clip)(*adam, *wt, self.gnorm_partials, self.clip_grad_norm, self.gnorm_ring)
        else:
            # fused: two launches — Adam with its bookkeeping and the target copy folded in; the online conv copies, mirrored to the target's on a sync
            (ops.adam_step_sync_wt if on.fused else ops.adam_step_sync)(*adam, *wt)
        self._blend_target()
        self._feature_rank()
        self._redo()
        self._reset_net()

    def set_risk(self, risk, eta=0.0, K=None):
        """``learner.iqn.risk`` / ``risk_eta`` (``risk_value``); refused once an update has been issued, like the handle's a0_learner_set_risk."""
        if self._risk_fixed:
            raise ValueError("learner.iqn.risk: the setting is fixed once the learner has run an update")
        kind, eta = risk_value(risk, eta, algo=self.L.algo, munchausen=self.munchausen)
        if kind and not hasattr(self.ops, "risk_distort"):
            raise ValueError(f"learner.iqn.risk={risk}: needs a backend with risk_distort")
        if kind and self.t_risk is None:
            self.t_risk = self.ops.empty(self.B * int(self.K if K is None else K))
        self.risk_kind, self.risk_eta = kind, eta

    # ------------------------------------------------------------------ the target network's pass as a stage of its own
    @property
    def target_stage_supported(self) -> bool:
        """The target network's forward pass on the next observations (encoder + fc1 GEMM: agent.py:176 / 222) depends on neither the online weights nor the
        previous update's gradients, so the Trainer may run it for batch k + 1 on a second stream while update k is in flight — for the paths whose
        tail consumes the target's fc1 slabs (dqn's and c51's fused heads) and without NoisyNet (whose per-update noise draws are ordered on the host)."""
        L = self.L
        return not L.noisy and self.online.fused and ((L.algo == "dqn" and self.family == "scalar") or L.algo == "c51")

    def _tstage_buf(self, p: int):
        if p not in self._tst:
            ns = self.ops.dense_fwd_partial_slabs(self.B, 512, self.L.feat)
            self._tst[p] = (self.ops.empty(self.B * self.L.feat), self.ops.empty(ns * self.B * 512))
        return self._tst[p]

    def target_stage(self, frames, slot, sample_stride, p: int):
        """target(next_obs) up to the fc1 GEMM's split-K slabs, into the buffers of parity ``p`` (what ``forward_dense(..., tstage=p)`` then consumes)."""
        L, ops, B, tg = self.L, self.ops, self.B, self.target
        act3, slabs = self._tstage_buf(p)
        Wf_t, _ = tg.wb("fc1")
        ops.encoder_fwd_fused(tg.net, tg.wt, tg.encoder_weights(), frames, slot, sample_stride, self.obs_bytes, B, None, None, act3)
        ops.dense_fwd_partial(act3, L.feat, Wf_t, B, 512, L.feat, slabs)

    def _qr_fused_ok(self) -> bool:
        """QR's head path from the GEMM slabs to the loss in one launch (a0_qr_head_loss_slabs): the staged head outputs of a sample must fit in LDS."""
        L, ops = self.L, self.ops
        R_on = 2 * self.B if self.double_q else self.B
        return (L.A <= 32 and (3 * L.Npad + (L.T + 3) // 4 * 4) * 4 <= 150 * 1024 and L.Npad % 4 == 0
                and max(ops.dense_fwd_partial_slabs(R_on, L.Npad, 512), ops.dense_fwd_partial_slabs(self.B, L.Npad, 512)) <= 8)

    # ------------------------------------------------------------------ the family: decided once, with its buffers
    def _family(self) -> str:
        """Which forward ``forward_dense`` runs, decided once like the handle's ``a0_family`` (learner_state.h): "scalar" — dqn and mdqn with A + dueling <= 24, from the
        fc1 slabs to the loss in one launch; "dist" — c51, and qr where ``_qr_fused_ok``; "iqn"; "fqf"; "layerwise" — the rest, layer by layer: qr and mdqn beyond those
        limits and — the one difference: the handle refuses it — the wide dqn head."""
        L = self.L
        if L.algo in ("iqn", "fqf"):
            return L.algo
        if L.algo in ("dqn", "mdqn"):
            return "scalar" if L.A + (1 if L.dueling else 0) <= 24 else "layerwise"
        if L.algo not in ("c51", "qr"):
            raise NotImplementedError(f"algo {L.algo} has no device learner yet")
        return "dist" if L.algo == "c51" or self._qr_fused_ok() else "layerwise"

    def _ws_dist(self):
        """The dist family's buffers (a0_ws_dist): the online network's features of s and (double-Q) of s' lie back to back, and so do their fc1 slabs, h and head
        slabs — R_on = B or 2B rows — because fc1 and the head run over both as ONE GEMM each (same weights).  ``ws_o.act3`` and ``ws_o.h`` (h(s) of the online
        network: what the backward pass reads) and ``ws_s.act3`` are views into them."""
        L, ops, B = self.L, self.ops, self.B
        R_on = 2 * B if self.double_q else B
        ns, ns_on = ops.dense_fwd_partial_slabs(B, 512, L.feat), ops.dense_fwd_partial_slabs(R_on, 512, L.feat)
        nh_on, nh_tg = ops.dense_fwd_partial_slabs(R_on, L.Npad, 512), ops.dense_fwd_partial_slabs(B, L.Npad, 512)
        buf = self._dist_buf = dict(fc1_on=ops.empty(ns_on * R_on * 512), fc1_tg=ops.empty(ns * B * 512), h_on=ops.empty(R_on * 512), act3_on=ops.empty(R_on * L.feat),
                                    hs_on=ops.empty(nh_on * R_on * L.Npad), hs_tg=ops.empty(nh_tg * B * L.Npad), R_on=R_on)
        self.ws_o.h, self.ws_o.act3 = buf["h_on"][: B * 512], buf["act3_on"][: B * L.feat]
        if self.double_q:
            self.ws_s.act3 = buf["act3_on"][B * L.feat:]

    # ------------------------------------------------------------------ forward_dense's stages, under the names of the handle's (csrc/learner.hip)
    def _upd_prepare(self, u: _Upd):
        """In front of every forward: what a separately staged target pass cannot go with, learner.aug_shift's shift of the batch into the stage buffer — every pass
        then reads that dense batch — and NoisyNet's compose of both networks' effective weights."""
        L, ops, on, tg = self.L, self.ops, self.online, self.target
        if u.tstage is not None and not self.target_stage_supported:
            raise ValueError("tstage: this learner's target pass cannot run as a separate stage")
        if self.net_reset_freq > 0 and u.tstage is not None:
            raise ValueError("tstage: not together with learner.net_reset_freq (the separately staged target pass has read a target the reset rewrites)")
        if self.munchausen and u.tstage is not None:
            raise ValueError("tstage: not together with learner.iqn.munchausen (the update has two target passes and neither is staged separately)")
        if self.aug_shift > 0:
            if u.tstage is not None:
                raise ValueError("tstage: not together with learner.aug_shift (the separately staged target pass has read the unshifted ring)")
            ops.augment_shift(u.frames, u.slot, u.stride, L.C, L.H, L.W, self.aug_shift, self.B, self.aug_rng.seed, self.state, 0, self.aug_stage)
            u.frames, u.slot, u.stride = self.aug_stage, None, 2 * self.obs_bytes
        if L.noisy:
            mods = on.compose_mods() + tg.compose_mods()
            if len(mods) <= 6:
                ops.noisy_multi(False, mods)            # both networks' effective weights in one launch
            else:
                on.compose_noise()
                tg.compose_noise()

    def _upd_encode(self, u: _Upd, *sel):
        """sel: up to three ``(net, ws, next, keep)`` or None (a pass this update does not have) — the encoder forward passes of one update over the same batch, on the
        next or the current observation; ``keep``: the differentiated pass, whose act1 / act2 the encoder backward reads.  They are independent of one another (the
        reference runs them one after the other, agent.py:176-181 / 222-231): on the fused split-operand kernel they go out, in the order given, as ONE launch
        (a0_net_encoder_fwd_fused_multi)."""
        L, B = self.L, self.B
        passes = [(net, ws, self.obs_bytes if nxt else 0, keep) for net, ws, nxt, keep in filter(None, sel)]
        if len(passes) > 1 and self.online.fused and (L.C, L.H, L.W) == (4, 84, 84):
            self.ops.encoder_fwd_fused_multi(self.net, [(net.wt, net.encoder_weights(), u.frames, u.slot, u.stride, chan_off, B, ws.act1 if keep else None,
                                                         ws.act2 if keep else None, ws.act3) for net, ws, chan_off, keep in passes])
            return
        for net, ws, chan_off, keep in passes:
            net.encode(ws, u.frames, u.slot, u.stride, chan_off, B, keep=keep)

    def _fwd_scalar(self, u: _Upd):
        """dqn (agent.py:173-190) and mdqn (193-215) from the fc1 slabs: the target pass on s' (unless ``tstage`` left it), a third pass — the online network on s'
        under double-Q; mdqn: the TARGET network on the CURRENT observation (agent.py:202-204) — and the online pass on s as one encoder launch, their fc1 GEMMs, and
        one kernel that finishes fc1 from the GEMMs' split-K slabs and runs heads, loss, head gradient and the head's backward-data pass (a0_dqn_head_loss_slabs /
        a0_mdqn_head_loss_slabs): only fc1 runs as a GEMM, and there are no reduction launches."""
        L, ops, B, on, tg = self.L, self.ops, self.B, self.online, self.target
        wo, wt, sl = self.ws_o, self.ws_t, self._fc1_slabs
        mdqn, staged = L.algo == "mdqn", u.tstage is not None
        (Wo, bo), (Wt, bt) = on.wb("head"), tg.wb("head")
        (Wf_o, bf_o), (Wf_t, bf_t) = on.wb("fc1"), tg.wb("fc1")
        w3, W3 = (self.ws_m, Wf_t) if mdqn else (self.ws_s, Wf_o)        # the third pass: ws_s is None without double-Q
        third = w3 is not None
        ns = ops.dense_fwd_partial_slabs(B, 512, L.feat)
        s_tg = sl[1]
        self._upd_encode(u, None if staged else (tg, wt, True, False), (tg if mdqn else on, w3, not mdqn, False) if third else None, (on, wo, False, True))
        if not staged and self._ok["dense_fwd_partial_multi_ok"](len(sl), B, 512, L.feat):
            # the passes' fc1 GEMMs as ONE launch: together they fill the chip with a half / a third of the splits each would need alone
            ns = ops.dense_fwd_partial_multi([wo.act3, wt.act3] + ([w3.act3] if third else []), L.feat, [Wf_o, Wf_t] + ([W3] if third else []), B, 512, L.feat, sl)
        else:
            if staged:
                s_tg = self._tstage_buf(u.tstage)[1]
            else:
                ops.dense_fwd_partial(wt.act3, L.feat, Wf_t, B, 512, L.feat, s_tg)
            if third:
                ops.dense_fwd_partial(w3.act3, L.feat, W3, B, 512, L.feat, sl[2])
            ops.dense_fwd_partial(wo.act3, L.feat, Wf_o, B, 512, L.feat, sl[0])
        if mdqn:
            ops.mdqn_head_loss_slabs(sl[0], s_tg, sl[2], ns, bf_o, bf_t, wo.h, Wo, bo, Wt, bt, L.A, L.dueling, L.Npad, u.act, u.rew, u.done, u.wgt,
                                     self.gamma_n, self.mdqn_tau, self.mdqn_lo, B, self.loss, wo.q, wt.q, self._q_cur, wo.draw, self.state, wo.dh)
        else:
            ops.dqn_head_loss_slabs(sl[0], s_tg, sl[2] if third else None, ns, bf_o, bf_t, wo.h, Wo, bo, Wt, bt,
                                    L.A, L.dueling, L.Npad, u.act, u.rew, u.done, u.wgt, self.gamma_n, B, self.loss, wo.q, wt.q, wo.draw, self.state, wo.dh)
        u.have_draw = u.have_dh = True           # draw, and the head's backward-data pass: dh is written by the same kernel

    def _fwd_dist(self, u: _Upd):
        """c51 (agent.py:218-268) and qr where ``_qr_fused_ok`` (272-293).  The passes (online on s, online on s' under double-Q, target on s') up to the head GEMMs'
        split-K slabs: the encoders as one launch, the fc1 GEMMs as one grouped launch (the online passes' rows interleaved into one [splits][R_on][512] buffer), ONE
        reduction launch (bias + ReLU), the head GEMMs as one grouped launch — buf["hs_on"] holds rows [0, B) = s and, under double-Q, rows [B, 2B) = s'.  Then one
        launch for everything behind them (a0_c51_head_loss_slabs: slab sums, dueling, greedy next action, projection + cross entropy, head gradient;
        a0_qr_head_loss_slabs: the quantile Huber loss in its place)."""
        L, ops, B, on, tg, buf = self.L, self.ops, self.B, self.online, self.target, self._dist_buf
        wo, wt, wsel, dq_, R_on = self.ws_o, self.ws_t, self.ws_s, self.double_q, self._dist_buf["R_on"]
        staged = u.tstage is not None
        ns, ns_on = ops.dense_fwd_partial_slabs(B, 512, L.feat), ops.dense_fwd_partial_slabs(R_on, 512, L.feat)
        (Wf_o, bf_o), (Wf_t, bf_t) = on.wb("fc1"), tg.wb("fc1")
        (Wh_o, bh_o), (Wh_t, bh_t) = on.wb("head"), tg.wb("head")
        s_tg = buf["fc1_tg"]
        self._upd_encode(u, None if staged else (tg, wt, True, False), (on, wsel, True, False) if dq_ else None, (on, wo, False, True))
        npass = 3 if dq_ else 2
        grouped = not staged and self._ok["dense_fwd_partial_multi_ok"](npass, B, 512, L.feat) and self._ok["dense_fwd_partial_multi_ok"](npass, B, L.Npad, 512)
        if grouped:
            # the passes are GEMMs of one shape each for fc1 and for the head: ONE grouped launch per layer, the online passes' rows interleaved into the
            # [splits][R_on][N] buffers the reduction and the loss kernel read
            a3, f1 = buf["act3_on"], buf["fc1_on"]
            Xs = [a3[: B * L.feat]] + ([a3[B * L.feat:]] if dq_ else []) + [wt.act3]
            sl = [f1] + ([f1[B * 512:]] if dq_ else []) + [s_tg]
            st = [R_on * 512] * (npass - 1) + [B * 512]
            ns_on = ns = ops.dense_fwd_partial_multi(Xs, L.feat, [Wf_o] * (npass - 1) + [Wf_t], B, 512, L.feat, sl, st)
        else:
            if staged:
                s_tg = self._tstage_buf(u.tstage)[1]
            else:
                ops.dense_fwd_partial(wt.act3, L.feat, Wf_t, B, 512, L.feat, s_tg)
            ops.dense_fwd_partial(buf["act3_on"], L.feat, Wf_o, R_on, 512, L.feat, buf["fc1_on"])
        ops.reduce_bias_act_multi([(buf["fc1_on"], ns_on, bf_o, buf["h_on"], R_on), (s_tg, ns, bf_t, wt.h, B)], 512, True)
        if grouped:
            h, hs = buf["h_on"], buf["hs_on"]
            Xs = [h[: B * 512]] + ([h[B * 512:]] if dq_ else []) + [wt.h]
            sl = [hs] + ([hs[B * L.Npad:]] if dq_ else []) + [buf["hs_tg"]]
            st = [R_on * L.Npad] * (npass - 1) + [B * L.Npad]
            nh_on = nh_tg = ops.dense_fwd_partial_multi(Xs, 512, [Wh_o] * (npass - 1) + [Wh_t], B, L.Npad, 512, sl, st)
        else:
            nh_on = ops.dense_fwd_partial(buf["h_on"], 512, Wh_o, R_on, L.Npad, 512, buf["hs_on"])
            nh_tg = ops.dense_fwd_partial(wt.h, 512, Wh_t, B, L.Npad, 512, buf["hs_tg"])
        head = (buf["hs_on"], nh_on, R_on, buf["hs_tg"], nh_tg, B if dq_ else -1, bh_o, bh_t, L.Npad, L.A, L.T, L.dueling, u.act, u.rew, u.done, u.wgt)
        if L.algo == "c51" and self.hl_gauss > 0:      # learner.c51.hl_gauss (a0_fwd_dist's branch): the same launch with the Gaussian histogram in the projection's place
            ops.c51_hl_gauss_head_loss_slabs(*head, self.atoms, self.gamma_n, self.vmin, self.vmax, self.hl_gauss_sigma, B, self.loss, wo.draw, self.state, q_on=wo.q,
                                             q_tg=wt.q, m_out=self.m_proj, a_star=self.a_star)
        elif L.algo == "c51":
            ops.c51_head_loss_slabs(*head, self.atoms, self.gamma_n, self.vmin, self.vmax, B, self.loss, wo.draw, self.state, q_on=wo.q, q_tg=wt.q, m_out=self.m_proj,
                                    a_star=self.a_star)
        else:
            ops.qr_head_loss_slabs(*head, self.qr_taus, self.gamma_n, B, self.loss, wo.draw, self.state, q_on=wo.q, q_tg=wt.q, a_star=self.a_star)
        u.have_draw = True

    def _fwd_layerwise(self, u: _Upd):
        """Layer by layer — per pass fc1, head, dueling combine; the loss leaves dq: the wide dqn head, qr and mdqn where the one-launch paths do not take them."""
        L, ops, B, on, tg = self.L, self.ops, self.B, self.online, self.target
        wo, wt, wsel = self.ws_o, self.ws_t, self.ws_s
        if L.algo == "mdqn":
            # target net on the next AND on the current observation (agent.py:202-204), online net on the current one: one launch
            self._upd_encode(u, (tg, wt, True, False), (tg, self.ws_m, False, False), (on, wo, False, True))
            tg.head(wt, B)
            tg.head(self.ws_m, B)
            on.head(wo, B)
            ops.loss_mdqn(wo.q, wt.q, self.ws_m.q, L.A, u.act, u.rew, u.done, u.wgt, self.gamma_n, self.mdqn_tau, self.mdqn_lo, B, self.loss, wo.dq, self.state)
            return
        sel, ws_sel = (on, wsel) if self.double_q else (tg, wt)      # the network that selects the next action, and the pass it does so from
        self._upd_encode(u, (tg, wt, True, False), (on, wsel, True, False) if self.double_q else None, (on, wo, False, True))
        tg.head(wt, B)
        if self.double_q:
            on.head(wsel, B)
        sel.select(ws_sel, B, 1, self.a_star)
        on.head(wo, B)
        if L.algo == "dqn":
            ops.loss_dqn(wo.q, wt.q, L.A, u.act, self.a_star, u.rew, u.done, u.wgt, self.gamma_n, B, self.loss, wo.dq, self.state)
        else:
            ops.quantile_target(wt.q, L.A * L.T, 1, L.T, self.a_star, u.rew, u.done, self.gamma_n, B, L.T, self.y)
            wo.dq.zero_()
            ops.loss_quantile_huber(wo.q, L.A * L.T, 1, L.T, self.y, self.qr_taus, 0, u.act, u.wgt, B, L.T, L.T, self.loss, wo.dq, self.state)

    def _fwd_iqn(self, u: _Upd):
        """IQNLearner.train_step (agent.py:296-331); ``u.rand``: [taus_K [B*K], taus_N' [B*N'], taus_N [B*N]] in the reference's draw order."""
        L, ops, B, on, tg = self.L, self.ops, self.B, self.online, self.target
        wo, wt, wsel = self.ws_o, self.ws_t, self.ws_s
        (t_sel, t_tgt, t_on), (K, Nd, N) = u.rand, (self.K, self.N_dash, self.N)
        if self.munchausen:
            # learner.iqn.munchausen (a0_fwd_iqn's branch, step for step): the target network on s' and on s at the same N' fractions; no greedy next action, so the
            # selection pass is not run and t_sel — drawn so that the stream position stays a plain iqn run's — is left unused
            wm = self.ws_m
            self._upd_encode(u, (tg, wt, True, False), (tg, wm, False, False), (on, wo, False, True))
            tg.head(wt, B, t_tgt, Nd)
            tg.head(wm, B, t_tgt, Nd)
            ops.miqn_target(wt.q, wm.q, Nd * L.A, L.A, 1, u.act, u.rew, u.done, self.gamma_n, self.mdqn_tau, self.mdqn_alpha, self.mdqn_lo, B, Nd, L.A, self.y)
        else:
            sel, ws_sel = (on, wsel) if self.double_q else (tg, wt)      # greedy next action from the K-sample mean, of the online network under double-Q (agent.py:303-306)
            self._upd_encode(u, (tg, wt, True, False), (on, wsel, True, False) if self.double_q else None, (on, wo, False, True))
            if self.risk_kind:      # learner.iqn.risk (a0_fwd_iqn's branch): the policy's K fractions, distorted into the engine's own buffer
                ops.risk_distort(t_sel, self.t_risk, B * K, self.risk_kind, self.risk_eta)
                t_sel = self.t_risk
            sel.head(ws_sel, B, t_sel, K)
            sel.select(ws_sel, B, K, self.a_star)
            tg.head(wt, B, t_tgt, Nd)
            ops.quantile_target(wt.q, Nd * L.A, L.A, 1, self.a_star, u.rew, u.done, self.gamma_n, B, Nd, self.y)
        on.head(wo, B, t_on, N)
        wo.dq.zero_()
        ops.loss_quantile_huber(wo.q, N * L.A, L.A, 1, self.y, t_on, N, u.act, u.wgt, B, N, Nd, self.loss, wo.dq, self.state)

    def _fwd_fqf(self, u: _Upd):
        """FQFLearner.train_step (agent.py:334-388); ``u.rand`` (parity tests only): fractions evaluated elsewhere, written over the fraction net's own (see
        ``forward_dense``).  Leaves the fraction loss in ``u.frac``."""
        L, ops, B, on, tg, F = self.L, self.ops, self.B, self.online, self.target, self.L.F
        wo, wt, wsel, wf = self.ws_o, self.ws_t, self.ws_s, self.ws_f

        def taus(net, ws, k):
            net.fqf_taus(ws, B)
            if u.rand is not None:
                ws.tau_all[: B * (F + 1)].copy_(u.rand[2 * k].reshape(-1)); ws.tau_hat[: B * F].copy_(u.rand[2 * k + 1].reshape(-1))
        sel, ws_sel = (on, wsel) if self.double_q else (tg, wt)      # greedy next action at the selecting network's own fractions
        self._upd_encode(u, (on, wo, False, True), (tg, wt, True, False), (on, wsel, True, False) if self.double_q else None)
        taus(on, wo, 0)
        on.head(wo, B, wo.tau_hat, F)
        taus(sel, ws_sel, 1)
        sel.head(ws_sel, B, ws_sel.tau_hat, F)
        sel.select(ws_sel, B, F, self.a_star)
        tg.head(wt, B, wo.tau_hat, F)           # quirk Q16: target evaluated at the ONLINE tau-hats
        ops.quantile_target(wt.q, F * L.A, L.A, 1, self.a_star, u.rew, u.done, self.gamma_n, B, F, self.y)
        wo.dq.zero_()
        ops.loss_quantile_huber(wo.q, F * L.A, L.A, 1, self.y, wo.tau_hat, F, u.act, u.wgt, B, F, F, self.loss, wo.dq, self.state)
        # fraction loss: q at the interior taus (no grad), its gradient w.r.t. the fraction logits, RMSprop
        ops.fqf_inner_taus(wo.tau_all, wf.taus, B, F)                      # taus[:, 1:-1] -> [B][F-1]
        on.head(wf, B, wf.taus, F - 1, feat=wo.act3)
        ops.fqf_fraction_loss(wf.q, wo.q, wo.tau_all, u.act, u.wgt, B, F, L.A, L.Fpad, self.frac_loss, self.dfrac_logits, wo.frac_logits)
        ops.dense_wgrad(self.dfrac_logits, wo.act3, L.feat, self.grads[L.blocks["frac"].all], B, L.Fpad, L.feat, self.slabs)
        # the fraction net's RMSprop step (agent.py:140-147) runs in apply(): nothing in this update reads the fraction net again, and
        # under data parallelism its gradient has then been reduced with the dense bucket like every other block
        u.frac = self.frac_loss

    def forward_dense(self, frames, slot, sample_stride, act, rew, done, wgt, rand: Optional[List[torch.Tensor]] = None, tstage: Optional[int] = None):
        """Forward passes, losses and the dense half of the backward pass (every gradient but the convolution blocks', which
        backward_encoder adds); no parameter is modified (FQF's fraction net aside, which the reference also steps separately,
        agent.py:140-147).

        frames: u8 replay rows (st || st_next); slot: optional int32 row indices; act int32, rew/done/wgt fp32 [B].
        rand (IQN): [taus_K [B*K], taus_N' [B*N'], taus_N [B*N]] in the reference's draw order.
        rand (FQF, parity tests only): [taus [B*(F+1)], tau_hats [B*F]] of the online net on the observations, then the same pair for the
        action-selection pass on the next observations — fractions evaluated elsewhere (the oracle's), written over the fraction net's own
        so that both sides evaluate q(tau) at bit-identical fractions; the fraction net still runs (its logits feed the fraction loss).
        Returns the per-sample loss tensor (device) — and for FQF also the fraction loss.
        """
        u = self._upd = _Upd(frames, slot, sample_stride, act, rew, done, wgt, rand, tstage)
        self._risk_fixed = True
        self._upd_prepare(u)
        {"scalar": self._fwd_scalar, "dist": self._fwd_dist, "layerwise": self._fwd_layerwise, "iqn": self._fwd_iqn, "fqf": self._fwd_fqf}[self.family](u)
        self._backward_dense(self.ws_o, self.B, u.have_draw, u.have_dh)
        if self._bucketed_hook():      # the NaN flag rides at the tail of the dense gradient bucket
            self.ops.nan_flag_export(self.state, self.grads[self.L.n_params_padded: self.L.n_params_padded + 1])
        u.act = u.rew = u.done = u.wgt = u.rand = None      # backward_encoder reads the batch (frames, slot, stride) again, nothing else
        return (self.loss, u.frac) if u.frac is not None else self.loss
