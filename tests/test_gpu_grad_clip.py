"""GPU (MI355X): global gradient-norm clipping in front of Adam (``learner.clip_grad_norm``).

Kernels: the two-stage norm (a0_grad_norm_partials + the CLIP form of the Adam launch) against ``torch.nn.utils.clip_grad_norm_`` on a float64 CPU copy, and the
clipped step bit for bit against the unclipped entry points on a gradient multiplied by the coefficient beforehand.  Learner: the engine, the a0_learner handle and
the one-rank data-parallel path on the engine tests' smallest geometry.  Loop: the library-handle loop against the Python classes, the setting off, snapshots.

Tolerance of the norm: squares of floats are exact in double and the sums are doubles (relative error ~1e-13 over 1.7 M terms), so the only rounding that shows is
the final cast to fp32 (half an ulp) — bound: 2 fp32 ulp, rtol 2.4e-7.

Work split of stage 1 (csrc/optim.hip): 256 partials; partial b covers [b * chunk, (b + 1) * chunk), chunk = ceil(n / 256) rounded up to a multiple of four; a
workgroup's 256 lanes take four floats each per pass.  Edges: n = 3 / 4 / 5 (vector width), 255 / 256 / 257 (partial count), 1023 / 1024 / 1025 (chunk 4 -> 8: the
last n at which every partial is used by exactly one vector), 262143 / 262144 / 262145 (chunk 1024 -> 1028: a lane's second pass)."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

RTOL = 2.4e-7                      # 2 fp32 ulp
P = 256                            # A0_GRAD_NORM_PARTIALS
N_EDGES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 1686180]
HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-2 / 32, tf=3)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert ops.GRAD_NORM_PARTIALS == P
    return ops


# ------------------------------------------------------------------------------------------------ inputs and the float64 reference, computed once per case
_GRADS = {}


def _grad(n, kind):
    """(fp32 CPU gradient, float64 reference norm by torch.nn.utils.clip_grad_norm_) — cached, never modified."""
    key = (n, kind)
    if key not in _GRADS:
        g = torch.from_numpy(recipe.gen(1000 + n % 9973).standard_normal(n).astype(np.float32))
        if kind == "huge":
            g[n // 3] = 1e30
        elif kind == "zero":
            g.zero_()
        p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p.grad = g.double().clone()
        ref = float(torch.nn.utils.clip_grad_norm_([p], 1.0))
        _GRADS[key] = (g, ref)
    return _GRADS[key]


def _at_offset(hip, t, off):
    """A device copy of ``t`` whose first element lies ``4 * off`` bytes behind a 16-byte boundary."""
    buf = hip.zeros(t.numel() + 8)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


def _coef(norm32, max_norm):
    """The coefficient in fp32, as the kernel forms it."""
    c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return c if c < np.float32(1.0) else np.float32(1.0)


class _Bufs:
    """One starting state of an Adam step over n (of n_total) elements; ``clone`` gives every run the same one."""

    def __init__(self, hip, n, n_total, state, seed=5, off=0):
        r = recipe.gen(seed)
        f = lambda k, scale=1.0: torch.from_numpy((r.standard_normal(k) * scale).astype(np.float32))
        self.p, self.t = _at_offset(hip, f(n_total), off), _at_offset(hip, f(n_total), off)
        self.m, self.v = _at_offset(hip, f(n, 0.1), off), _at_offset(hip, f(n, 0.1).abs(), off)
        self.state = torch.tensor(state, dtype=torch.int32, device=hip.device)
        self.scal = hip.zeros(4)
        self.n, self.n_total, self.off, self.hip = n, n_total, off, hip
        # the fused tail's extras: encoder weights, their k-major copies, the per-sample losses and their ring
        self.w = {k: torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(hip.device) for k, s in
                  (("w1", 32 * 256), ("b1", 32), ("w2", 64 * 512), ("b2", 64), ("w3", 64 * 576), ("b3", 64))}
        self.wt, self.wt_t = hip.zeros(hip.conv_wt_floats(4)), hip.zeros(hip.conv_wt_floats(4))
        self.loss = torch.from_numpy(r.standard_normal(32).astype(np.float32)).to(hip.device)
        self.loss_ring = hip.zeros(7)

    def clone(self):
        c = object.__new__(_Bufs)
        c.__dict__.update(self.__dict__)
        for k in ("p", "t", "m", "v"):
            setattr(c, k, _at_offset(self.hip, getattr(self, k), self.off))
        for k in ("state", "scal", "wt", "wt_t", "loss_ring"):
            setattr(c, k, getattr(self, k).clone())
        return c

    def everything(self):
        return dict(params=self.p, moment1=self.m, moment2=self.v, state=self.state, scalars=self.scal, target=self.t, wt=self.wt, wt_target=self.wt_t,
                    loss_ring=self.loss_ring)


def _step(hip, b, g, fold, clip=None):
    """One optimizer tail on ``b`` (modified in place): the parent's entry points, or with clip = (partials, max_norm, ring) the _clip forms."""
    a = (b.p, g, b.m, b.v, b.n, b.state, b.scal, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["tf"], b.t, b.n_total, None)
    if fold:
        a = a + (b.w, 4, b.wt, b.wt_t, b.loss, 32, b.loss_ring)
        hip.adam_step_sync_wt_clip(*a, *clip) if clip else hip.adam_step_sync_wt(*a)
    else:
        hip.adam_step_sync_clip(*a, *clip) if clip else hip.adam_step_sync(*a)
    torch.cuda.synchronize()


def _clipped_vs_parent(hip, n, n_total, kind, off, fold, state, max_over_norm, cap=5):
    """Stage 1 + the clip form from one starting state; the parent's entry point on g * coef (a torch fp32 multiply) from the same state.  Returns the ring's norm."""
    g_cpu, ref = _grad(n, kind)
    g = _at_offset(hip, g_cpu, off)
    assert g.data_ptr() % 16 == 4 * off
    partials = torch.full((P,), -1.0, dtype=torch.float64, device=hip.device)
    hip.grad_norm_partials(g, n, partials)
    ring = torch.full((cap,), -1.0, device=hip.device)
    max_norm = float(np.float32(ref * max_over_norm)) if ref > 0 else 0.5
    start = _Bufs(hip, n, n_total, state, off=off)
    got = start.clone()
    _step(hip, got, g, fold, (partials, max_norm, ring))
    slot = state[6] % cap
    norm = ring[slot].item()
    print(f"n={n} kind={kind} off={off} fold={fold}: ring {norm!r} float64 {ref!r} rel {abs(norm - ref) / ref if ref else 0.0:.3e}")
    assert abs(norm - ref) <= RTOL * ref, f"norm {norm!r} vs float64 {ref!r}"
    assert all(float(ring[i]) == -1.0 for i in range(cap) if i != slot), "only the slot state[6] % cap is written"
    coef = _coef(norm, max_norm)
    if max_over_norm > 1 or kind == "zero":
        assert coef == np.float32(1.0)
        scaled = g                                           # below the limit: the unclipped call on g itself
    else:
        assert coef < np.float32(1.0)
        scaled = _at_offset(hip, g * torch.tensor(coef, device=hip.device), off)
    want = start.clone()
    _step(hip, want, scaled, fold)
    for (k, x), y in zip(got.everything().items(), want.everything().values()):
        assert torch.equal(x, y), f"{k} differs from the parent's entry point on g * coef"
    return norm, start, got


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", N_EDGES)
def test_norm_and_step_at_the_work_split_edges(hip, n, off):
    """Every edge of the work split, with 16-byte loads and (pointer 4 bytes behind a boundary) on the scalar path: the norm to 2 ulp of float64, the plain form's
    step bit for bit — once clipping (limit = norm / 2), once not (limit = 2 norm: coef is exactly 1)."""
    for mx in (0.5, 2.0):
        _clipped_vs_parent(hip, n, n + (0 if off else (-n) % 4), "normal", off, False, [0, 1, 0, 0, 0, 0, 3, 0], mx)


@pytest.mark.parametrize("kind", ["huge", "zero"])
@pytest.mark.parametrize("n", [5, 1025, 1686180])
def test_a_single_huge_entry_and_an_all_zero_gradient(hip, n, kind):
    norm, _, _ = _clipped_vs_parent(hip, n, n, kind, 0, False, [0, 1, 0, 0, 0, 0, 0, 0], 0.5)
    if kind == "zero":
        assert norm == 0.0                                   # ... and coef 1: asserted inside
    else:
        assert norm >= 1e30


@pytest.mark.parametrize("mx", [0.5, 2.0], ids=["above", "below"])
@pytest.mark.parametrize("n,n_total", [(5, 8), (1025, 1025), (1686180, 1686180), (1686180, 1686180 + 100384)])
def test_fused_tail_bit_for_bit(hip, n, n_total, mx):
    """The FOLD form (a0_adam_step_sync_wt_clip): bookkeeping, loss mean, weight-copy refresh and commit included; the norm lands in the slot the loss mean uses,
    read before the counter advances."""
    norm, start, got = _clipped_vs_parent(hip, n, n_total, "normal", 0, True, [0, 1, 0, 0, 0, 0, 9, 0], mx)
    assert got.state[6].item() == 10 and got.state[1].item() == 2
    assert got.loss_ring[9 % 7].item() != 0.0


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
def test_a_target_sync_step(hip, fold):
    """update_steps 2 -> 3 with target_update_freq 3: the new parameters, blocks behind the Adam range included, go to the target in the same launch."""
    n, n_total = 4100, 4612
    _, start, got = _clipped_vs_parent(hip, n, n_total, "normal", 0, fold, [0, 2, 0, 0, 0, 0, 2, 0], 0.5)
    assert got.state[4].item() == 1 and torch.equal(got.t, got.p) and not torch.equal(got.p, start.p)


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
def test_a_nan_skipped_step_is_still_recorded(hip, fold):
    """NaN flag up: parameters and moments untouched, the skip counted — and the ring written all the same (asserted against float64 inside)."""
    n = 4100
    norm, start, got = _clipped_vs_parent(hip, n, n, "normal", 0, fold, [1, 1, 0, 0, 0, 0, 4, 0], 0.5)
    assert norm > 0.0
    assert torch.equal(got.p, start.p) and torch.equal(got.m, start.m) and torch.equal(got.v, start.v)
    assert got.state[2].item() == 1 and got.state[1].item() == 1 and got.state[3].item() == 1


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", [5, 1025, 1686180])
def test_stage_one_is_deterministic_and_pads_with_zeros(hip, n, off):
    g_cpu, ref = _grad(n, "normal")
    g = _at_offset(hip, g_cpu, off)
    a = torch.full((P,), -1.0, dtype=torch.float64, device=hip.device)
    b = torch.full((P,), -2.0, dtype=torch.float64, device=hip.device)
    hip.grad_norm_partials(g, n, a)
    hip.grad_norm_partials(g, n, b)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs over the same buffer"
    chunk = (-(-n // P) + 3) // 4 * 4
    used = -(-n // chunk)
    assert bool((a[used:] == 0).all()) and bool((a[:used] > 0).all()), "unused partials are zero, whatever the buffer held"
    assert abs(float(a.sum().sqrt()) - ref) <= 1e-12 * ref
    # every partial is the float64 sum of squares of its own range
    want = torch.stack([g_cpu[i * chunk:(i + 1) * chunk].double().square().sum() for i in range(used)])
    assert torch.allclose(a[:used].cpu(), want, rtol=1e-12, atol=0)


def test_bad_arguments_are_refused(hip):
    from agent0_amd._abi import A0Error
    n = 64
    b = _Bufs(hip, n, n, [0, 1, 0, 0, 0, 0, 0, 0])
    g, partials, ring = hip.zeros(n), torch.zeros(P, dtype=torch.float64, device=hip.device), hip.zeros(4)
    with pytest.raises(A0Error):
        _step(hip, b, g, False, (partials, 0.0, ring))       # the clip form needs a positive limit
    with pytest.raises(A0Error):
        _step(hip, b, g, True, (partials, -1.0, ring))
    with pytest.raises(A0Error):
        hip.grad_norm_partials(g, n, partials[:8])


# ------------------------------------------------------------------------------------------------ learner: engine, handle, one-rank data parallelism
B = 8
LEARNERS = {
    "dqn": dict(algo="dqn", A=4),
    "rainbow-lite": dict(algo="c51", A=4, dueling=True, noisy=True, double_q=True),
    "iqn": dict(algo="iqn", A=4, KNN=(8, 16, 24)),
    "fqf-fraction-clip": dict(algo="fqf", A=4, max_grad_norm=0.05),
}
SEED = 42 + 15485863


class _Case:
    def __init__(self, hip, name):
        from agent0_amd.deepq.layout import NetLayout
        c = LEARNERS[name]
        self.hip, self.c = hip, c
        self.spec = recipe.NetSpec(c["algo"], c["A"], dueling=c.get("dueling", False), noisy=c.get("noisy", False))
        self.L = NetLayout.from_spec(self.spec)
        self.K, self.N, self.Nd = c.get("KNN", (32, 64, 64))
        cap = 64
        self.ring = torch.from_numpy(recipe.make_frames(cap, 5, self.spec.obs_shape)).to(hip.device).reshape(-1).contiguous()
        self.cap = cap

    def engine(self, clip=-1.0):
        from agent0_amd.common.utils import DeviceRng
        from agent0_amd.deepq.engine import DeviceLearner
        c = self.c
        dev = DeviceLearner(self.hip, self.L, B, double_q=c.get("double_q", False), target_update_freq=3, K=self.K, N=self.N, N_dash=self.Nd,
                            max_grad_norm=c.get("max_grad_norm", -1.0), clip_grad_norm=clip)
        dev.online.load_state_dict(recipe.make_state_dict(self.spec, 11))
        dev.target.load_state_dict(recipe.make_state_dict(self.spec, 12))
        rng = DeviceRng(self.hip, SEED)
        if self.L.noisy:      # BaseLearner.__init__: both networks' first noise
            rng.reserve(rng.STREAM_NOISE, dev.online.noise_len); rng.reserve(rng.STREAM_NOISE, dev.target.noise_len)
        dev._test_rng = rng
        dev._test_taus = [self.hip.empty(B * k) for k in (self.K, self.Nd, self.N)] if self.L.algo == "iqn" else None
        return dev

    def handle(self, dev, clip):
        c = self.c
        nat = self.hip.native_learner(A=c["A"], dueling=c.get("dueling", False), double_q=c.get("double_q", False), B=B, discount=0.99, lr=5e-4, target_update_freq=3,
                                      algo=c["algo"], num_atoms=self.L.T, vmin=dev.vmin, vmax=dev.vmax, noisy=c.get("noisy", False), seed=SEED, K=self.K, N=self.N,
                                      N_dash=self.Nd, F=self.L.F, max_grad_norm=c.get("max_grad_norm", -1.0))
        nat.set_params(dev.online.flat, dev.target.flat)
        nat.set_grad_clip(clip)
        return nat

    def batch(self, s):
        hip = self.hip
        slot = torch.from_numpy(recipe.gen(40 + s).permutation(self.cap)[:B].astype(np.int32)).to(hip.device)
        a, r, d, w = recipe.make_transitions(B, self.c["A"], 70 + s)
        return (self.ring, slot, 2 * 28224) + tuple(torch.from_numpy(x).to(hip.device) for x in (a.astype(np.int32), r, d.astype(np.float32), w))

    def draws(self, dev):
        """BaseLearner.train_batch's draws in front of an update: the joint NoisyNet fill, the three tau vectors."""
        rng = dev._test_rng
        if self.L.noisy:
            assert dev.noise_joint is not None
            rng.normal(rng.STREAM_NOISE, 0.1, dev.noise_joint, dev.noise_joint.numel())
        if dev._test_taus is not None:
            for t in dev._test_taus:
                rng.uniform(rng.STREAM_TAUS, t, t.numel())
        return dev._test_taus

    def real_mask(self):
        """True at every entry of [0, n_adam) that maps to a reference parameter (head rows are padded to 32)."""
        L = self.L
        m = torch.zeros(L.n_adam, dtype=torch.bool)
        for b in L.blocks.values():
            if b.name == "frac":
                continue
            m[b.offset:b.offset + b.n_real * b.K] = True
            m[b.offset + b.N * b.K:b.offset + b.N * b.K + b.n_real] = True
        return m


def _everything(dev):
    return dict(online=dev.online.flat, target=dev.target.flat, moment1=dev.adam_m, moment2=dev.adam_v, state=dev.state)


def _same(x, y, what):
    for k in x:
        assert torch.equal(x[k], y[k]), f"{what}: {k}"


@pytest.mark.parametrize("name", list(LEARNERS))
def test_learner_norm_and_clipped_update(hip, name):
    """forward_backward without apply gives the gradient; its float64 norm over the REAL entries of grads[:n_adam] is what the ring must hold (so padding does not
    leak in and the fqf fraction block is outside).  apply() with clipping on == apply() with clipping off on host-prescaled gradients; the same update through
    a0_learner_update == the Python classes."""
    cs = _Case(hip, name)
    L = cs.L
    # ---- clipping off: the gradient, its norm on the host, the step on prescaled gradients
    off = cs.engine()
    rand = cs.draws(off)
    off.forward_backward(*cs.batch(0), rand=rand)
    torch.cuda.synchronize()
    g = off.grads[:L.n_adam].cpu()
    mask = cs.real_mask()
    assert 0 < int((~mask).sum()) == sum((b.N - b.n_real) * (b.K + 1) for b in L.blocks.values() if b.name != "frac"), "the head's padding rows"
    ref = float(g[mask].double().square().sum().sqrt())
    assert ref > 0.0
    clip = float(np.float32(0.5 * ref))
    frac = L.blocks.get("frac")
    if frac is not None:
        gf = float(off.grads[frac.all].double().square().sum().sqrt())
        print(f"{name}: fraction-net gradient norm {gf!r} beside {ref!r}")
        assert gf > 0.0
    # ---- clipping on
    on = cs.engine(clip)
    rand = cs.draws(on)
    on.forward_backward(*cs.batch(0), rand=rand)
    assert torch.equal(on.grads, off.grads)
    on.apply()
    torch.cuda.synchronize()
    norm = on.gnorm_ring[0].item()
    print(f"{name}: ring {norm!r} float64 over the real entries {ref!r} rel {abs(norm - ref) / ref:.3e}")
    assert abs(norm - ref) <= RTOL * ref
    assert float(on.gnorm_ring[1:].abs().max()) == 0.0
    coef = _coef(norm, clip)
    assert coef < np.float32(1.0)
    off.grads[:L.n_adam] *= torch.tensor(coef, device=hip.device)
    off.apply()
    torch.cuda.synchronize()
    _same(_everything(on), _everything(off), "clipping on vs clipping off on prescaled gradients")
    if frac is not None:
        assert torch.equal(on.online.flat[frac.all], off.online.flat[frac.all]) and torch.equal(on.rms_sq, off.rms_sq), "the fraction net's own step is untouched"
    # ---- the handle: two updates, the second below the limit of a second handle-free engine run
    py = cs.engine(clip)
    nat = cs.handle(py, clip)
    for s in range(3):
        rand = cs.draws(py)
        py.update(*cs.batch(s), rand=rand)
        nat.update(*cs.batch(s))
        torch.cuda.synchronize()
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, state=st), _everything(py), f"handle, update {s}")
    assert torch.equal(nat.grad_norm_ring(), py.gnorm_ring) and float(py.gnorm_ring[:3].min()) > 0.0
    assert torch.equal(py.gnorm_ring[0], on.gnorm_ring[0])
    nat.close()


@pytest.mark.parametrize("name", list(LEARNERS))
def test_one_rank_data_parallel_update_equals_the_plain_one(hip, name, monkeypatch):
    """A one-rank RCCL group (A0_DP_FORCE=1): the norm is taken behind the exchange's join; engine and handle equal the plain clipped run bit for bit."""
    import socket
    import torch.distributed as dist
    from agent0_amd.deepq.dist import init_process_group, make_grad_hook
    cs = _Case(hip, name)
    probe = cs.engine()
    probe.forward_backward(*cs.batch(0), rand=cs.draws(probe))
    clip = float(np.float32(0.5 * float(probe.grads[:cs.L.n_adam].double().square().sum().sqrt())))
    plain = cs.engine(clip)
    for s in range(2):
        plain.update(*cs.batch(s), rand=cs.draws(plain))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    for k, v in (("A0_DP_FORCE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", port)):
        monkeypatch.setenv(k, v)
    init_process_group()
    hook = None
    try:
        dp = cs.engine(clip)
        hook = dp.grad_hook = make_grad_hook(hip, cs.L.n_adam)
        assert type(hook).__name__ == "RcclGradAllReduce" and hook.active
        nat = cs.handle(dp, clip)
        from agent0_amd._abi import check
        check(hip.lib.a0_learner_set_exchange(nat.h, C.c_longlong(int(hook.comm))), "a0_learner_set_exchange")
        for s in range(2):
            dp.update(*cs.batch(s), rand=cs.draws(dp))
            nat.update(*cs.batch(s))
        torch.cuda.synchronize()
        _same(_everything(dp), _everything(plain), "engine with the exchange")
        assert torch.equal(dp.gnorm_ring, plain.gnorm_ring)
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, state=st), _everything(plain), "handle with the exchange")
        assert torch.equal(nat.grad_norm_ring(), plain.gnorm_ring)
        check(hip.lib.a0_learner_set_exchange(nat.h, C.c_longlong(0)), "a0_learner_set_exchange")
        nat.close()
    finally:
        if hook is not None:
            hook.close()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ loop
TODAYS_HEADER = ["frames", "fraction_loss", "loss", "return_train", "return_train_max", "qmax", "fps"]
ITERS, LS = 3, 4


def _trainer(tmp_path, monkeypatch, native, tag, clip=None, seed=42, extra=()):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = parse_overrides(["learner.algo=dqn", "actor.num_envs=8", "actor.sample_steps=8", "learner.batch_size=32", f"learner.learner_steps={LS}", "replay.size=300",
                           "trainer.training_start_steps=50", "learner.target_update_freq=5", "trainer.test_episodes=2", "wandb=false", "tb=false", f"seed={seed}",
                           f"logdir={tmp_path / tag}"] + ([f"learner.clip_grad_norm={clip!r}"] if clip is not None else []) + list(extra))
    cfg.obs_shape, cfg.action_dim = (4, 84, 84), 4
    return Trainer(cfg)


def _close(tr):
    tr.test = lambda: None
    tr.final(save=False)


def _loop_state(tr):
    torch.cuda.synchronize()
    eng = tr.learner.engine
    return dict(_everything(eng), gnorm_ring=eng.gnorm_ring.clone(), loss_ring=eng.loss_ring.clone())


@pytest.fixture(scope="module")
def loop_clip(tmp_path_factory):
    """A limit between the norms the run meets, taken from an unclipped run's (limit 1e30 clips nothing)."""
    mp = pytest.MonkeyPatch()
    try:
        tr = _trainer(tmp_path_factory.mktemp("probe"), mp, False, "probe", clip=1e30)
        for i in range(ITERS):
            tr.run_iteration()
        torch.cuda.synchronize()
        norms = tr.learner.engine.gnorm_ring[:ITERS * LS].cpu().numpy()
        _close(tr)
    finally:
        mp.undo()
    assert (norms > 0).all(), norms
    # half way up to the first norm that exceeds every norm before it: the updates in front of it stay below the limit, so the clipped run is the unclipped one up
    # to that update — which then clips.  (A run whose norms only fall has no such update: the median then, and the tests assert what they need.)
    k = next((i for i in range(1, len(norms)) if norms[i] > norms[:i].max()), None)
    return float(np.float32(np.median(norms) if k is None else 0.5 * (float(norms[:k].max()) + float(norms[k]))))


def _run(tmp_path, monkeypatch, native, tag, clip):
    from agent0_amd.deepq.native_loop import NativeLoop
    tr = _trainer(tmp_path, monkeypatch, native, tag, clip)
    res = [{k: v for k, v in tr.run_iteration(prefetch=(i == 1)).items() if k != "fps"} for i in range(ITERS)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    st = _loop_state(tr)
    _close(tr)
    return res, st


def test_handle_loop_equals_the_python_classes(loop_clip, tmp_path, monkeypatch):
    res_p, st_p = _run(tmp_path, monkeypatch, False, "py", loop_clip)
    res_n, st_n = _run(tmp_path, monkeypatch, True, "nat", loop_clip)
    norms = st_p["gnorm_ring"][:ITERS * LS].cpu().numpy()
    print("limit", loop_clip, "norms", norms.tolist())
    assert st_p["state"][1].item() == ITERS * LS and float(st_p["gnorm_ring"][ITERS * LS:].abs().max()) == 0.0
    assert (norms > loop_clip).any() and (norms < loop_clip).any(), "some updates clip and some do not"
    assert res_p == res_n
    _same(st_p, st_n, "library handles vs Python classes")
    assert "grad_norm" in res_n[-1] and res_n[-1]["grad_norm"] == pytest.approx(float(norms[-LS:].astype(np.float64).mean()), rel=1e-12)


def test_setting_off_changes_no_key_and_no_header(tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, True, "off")
    eng = tr.learner.engine
    assert eng.gnorm_ring is None and eng.gnorm_partials is None and eng.clip_grad_norm <= 0
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    assert list(res.keys()) == TODAYS_HEADER[:-1] + ["fps"] and res["loss"] is not None
    _close(tr)
    with open(tmp_path / "off" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == TODAYS_HEADER and len(rows) == 3
    assert "grad_norm" not in open(tmp_path / "off" / "msg.log").read()


def test_setting_on_reports_the_norm(loop_clip, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, True, "on", loop_clip)
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    _close(tr)
    with open(tmp_path / "on" / "progress.csv") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == TODAYS_HEADER + ["grad_norm"] and float(rows[-1]["grad_norm"]) == res["grad_norm"] > 0.0
    assert "grad_norm" in open(tmp_path / "on" / "msg.log").read()


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_with_clipping_on_continues_the_same_run(loop_clip, native, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, native, "a", loop_clip)
    res_a = [tr.run_iteration() for i in range(ITERS)]
    want = _loop_state(tr)
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "b", loop_clip)
    tr.run_iteration()
    snap = tr.save_snapshot(str(tmp_path / "snap"))
    assert tr.learner.engine.state[6].item() == LS
    _close(tr)
    st = torch.load(os.path.join(snap, "state.pth"), map_location="cpu", weights_only=True)
    assert float(st["net"]["gnorm_ring"][:LS].min()) > 0.0
    tr = _trainer(tmp_path, monkeypatch, native, "c", loop_clip, seed=7)
    tr.load_snapshot(snap)
    res_b = [tr.run_iteration() for i in range(1, ITERS)]
    got = _loop_state(tr)
    _close(tr)
    _same(got, want, "resumed vs uninterrupted")
    assert [r["grad_norm"] for r in res_b] == [r["grad_norm"] for r in res_a[1:]]
    norms = want["gnorm_ring"][:ITERS * LS]
    assert bool((norms > loop_clip).any()) and bool((norms < loop_clip).any())


def test_a_snapshot_written_without_the_ring_still_loads(loop_clip, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, True, "a")
    tr.run_iteration()
    snap = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    assert "gnorm_ring" not in torch.load(os.path.join(snap, "state.pth"), map_location="cpu", weights_only=True)["net"]
    tr = _trainer(tmp_path, monkeypatch, True, "b", loop_clip)
    tr.load_snapshot(snap)
    res = tr.run_iteration()
    assert res["grad_norm"] > 0.0
    _close(tr)
