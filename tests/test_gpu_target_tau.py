"""GPU (MI355X): soft target updates (``learner.target_tau``): a0_target_blend and everything that issues it.

1. the kernel against float64 (tests/target_tau_ref.py): every output is the float nearest to t + tau32 * fl32(p - t) evaluated in float64, except where that
   reference rounds twice — the suspects ``double_rounding_suspects`` finds from the inputs on the CPU — and there it is at most one ulp away.  The 27 input sets
   below hold 0 suspects (counted on the CPU), so every output has to be the nearest float; the test prints the worst case and the non-nearest count per set.
2. the target's weight copies after a forced blend == a0_net_conv_wt_refresh of the blended target, byte for byte.
3. decision timing behind each tail form (a0_adam_step_sync, a0_adam_step_sync_wt, both also clipped; a0_net_encoder_wgrad_tail + a0_update_tail).
4. DeviceLearner and the a0_learner handle for every learner of tests/test_gpu_grad_clip.py.
5. dqn against the oracle's learner with the Polyak step, free-running, inside tests/test_gpu_trace.py's FREE_BOUNDS.
6. the Trainer: handles == Python classes on main, launch and one-rank data parallelism; snapshots; the setting off.
7. bad arguments.

Work split of the kernel (csrc/optim.hip): 256 lanes per workgroup, 16 bytes per lane when both buffers are 16-byte aligned with a scalar tail of n_total % 4 floats,
else one float per lane; at most 2048 workgroups, grid-stride.  Shapes: 5 (one vector + a tail of one / five scalars), 1025 (two workgroups on the vector path, five on the
scalar one, tail of one), 77 824 + 37 (C = 4's three convolution weight blocks and a ragged tail of n % 4 = 1: 77 workgroups / 305)."""
import csv
import os

import numpy as np
import pytest
import torch

import recipe
import target_tau_ref as R

pytestmark = pytest.mark.gpu

TAUS = [0.005, 0.5, 0.999]
SENTINEL = -7.25


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "target_blend")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
_PAIRS = {}


def _pair(n, kind):
    """(t, p) as fp32 numpy arrays — cached, never modified."""
    if (n, kind) not in _PAIRS:
        g = recipe.gen(2000 + n % 9973)
        t = g.standard_normal(n).astype(np.float32)
        if kind == "random":
            p = g.standard_normal(n).astype(np.float32)
        elif kind == "equal":
            p = t.copy()
        else:      # the difference underflows against t: one or two ulp apart, either side
            p = t.copy()
            for _ in range(2):
                up = g.integers(0, 2, n).astype(bool)
                step = g.integers(0, 2, n).astype(bool)
                q = np.nextafter(p, np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float32)
                p = np.where(step, q, p)
            p[0] = np.nextafter(t[0], np.float32(np.inf))
        _PAIRS[(n, kind)] = (t, p)
    return _PAIRS[(n, kind)]


_REFS = {}


def _ref(n, kind, tau):
    if (n, kind, tau) not in _REFS:
        t, p = _pair(n, kind)
        _REFS[(n, kind, tau)] = (R.blend_nearest(t, p, tau), R.double_rounding_suspects(t, p, tau))
    return _REFS[(n, kind, tau)]


def _guarded(hip, a, off):
    """(whole buffer, the view holding ``a`` 4 * off bytes behind a 16-byte boundary); everything around the view holds SENTINEL."""
    buf = torch.full((a.size + 12,), SENTINEL, device=hip.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[4 + off:4 + off + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return buf, v


def _guards_intact(buf, off, n):
    return bool((buf[:4 + off] == SENTINEL).all()) and bool((buf[4 + off + n:] == SENTINEL).all())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", [5, 1025, 77824 + 37])
def test_kernel_against_float64(hip, n, off, tau):
    for kind in ("random", "equal", "underflow"):
        t, p = _pair(n, kind)
        want, suspects = _ref(n, kind, tau)
        tb, tv = _guarded(hip, t, off)
        pb, pv = _guarded(hip, p, off)
        hip.target_blend(tv, pv, n, tau, None, 0, 1)
        torch.cuda.synchronize()
        got = tv.cpu().numpy()
        dist = R.ulp_distance(got, want)
        off_nearest = dist != 0
        worst = int(dist.argmax())
        print(f"n={n} off={off} tau={tau} {kind}: worst {int(dist.max())} ulp at {worst} (t {t[worst]!r} p {p[worst]!r} got {got[worst]!r} want {want[worst]!r}); "
              f"non-nearest {int(off_nearest.sum())}, double-rounding suspects {int(suspects.sum())}")
        assert int(dist.max()) <= 1
        assert not (off_nearest & ~suspects).any(), "an output that is not the nearest float although the float64 reference rounds once there"
        assert int(suspects.sum()) <= 4, "the inputs keep the reference's double roundings to a handful"
        if kind == "equal":
            assert np.array_equal(got.view(np.int32), t.view(np.int32)), "p == t is a fixed point, bit for bit"
        if kind == "underflow":
            assert np.array_equal(got, t if tau < 0.5 else want) and (tau < 0.5 or not np.array_equal(got, t))
        assert torch.equal(pv.cpu(), torch.from_numpy(p)), "the online buffer is only read"
        assert _guards_intact(tb, off, n) and _guards_intact(pb, off, n), "nothing outside [0, n_total) is touched"


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
def test_no_blend_changes_no_byte(hip, off):
    """force = 0 and state[1] % freq != 0 (or freq = 0): the target and its weight copies keep every byte; state[1] % freq == 0: it blends."""
    w = _conv_world(hip, 4, (0, 0, 0), off, 37)
    t0, wt0 = w.t.clone(), w.wt_t.clone()
    for steps, freq in ((4, 3), (5, 3), (1, 2), (6, 0), (0, 0)):
        state = torch.tensor([0, steps, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=hip.device)
        hip.target_blend(w.t, w.p, w.n, 0.5, state, freq, 0, w.weights(w.t), 4, w.wt_t)
        torch.cuda.synchronize()
        assert torch.equal(_bits(w.t), _bits(t0)) and torch.equal(_bits(w.wt_t), _bits(wt0)), (steps, freq)
    state = torch.tensor([0, 6, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=hip.device)
    hip.target_blend(w.t, w.p, w.n, 0.5, state, 3, 0, w.weights(w.t), 4, w.wt_t)
    torch.cuda.synchronize()
    assert not torch.equal(w.t, t0) and not torch.equal(_bits(w.wt_t), _bits(wt0))
    assert state.tolist() == [0, 6, 0, 0, 0, 0, 0, 0], "the state block is only read"


# ------------------------------------------------------------------------------------------------ 2. weight copies
class _ConvWorld:
    """A target and an online flat buffer laid out [pad0 | w1 b1 | pad1 | w2 b2 | pad2 | w3 b3 | tail], and the target's weight copies."""


def _conv_world(hip, C_, pads, off, tail):
    g = recipe.gen(31 + C_ + sum(pads) + off)
    K1 = 64 * C_
    sizes = [pads[0], 32 * K1, 32, pads[1], 64 * 512, 64, pads[2], 64 * 576, 64, tail]
    at = np.cumsum([0] + sizes)
    w = _ConvWorld()
    w.n = int(at[-1])
    w.o = dict(w1=(at[1], at[2]), b1=(at[2], at[3]), w2=(at[4], at[5]), b2=(at[5], at[6]), w3=(at[7], at[8]), b3=(at[8], at[9]))
    w.tb, w.t = _guarded(hip, (g.standard_normal(w.n) * 0.05).astype(np.float32), off)
    w.pb, w.p = _guarded(hip, (g.standard_normal(w.n) * 0.05).astype(np.float32), off)
    w.off = off
    w.weights = lambda flat: {k: flat[a:b] for k, (a, b) in w.o.items()}
    w.wt_t = hip.empty(hip.conv_wt_floats(C_))
    hip.conv_wt_refresh(w.weights(w.t), C_, w.wt_t)
    torch.cuda.synchronize()
    return w


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("pads", [(0, 0, 0), (4, 0, 8), (1, 0, 0), (0, 2, 0), (0, 0, 3)], ids=lambda p: "pads%d-%d-%d" % p)
@pytest.mark.parametrize("C_", [4, 1])
def test_weight_copies_follow_the_blended_target(hip, C_, pads, off):
    """Convolution blocks at multiples of four floats (four weights of a row per lane) and not (weight by weight), on the 16-byte path and on the scalar one."""
    w = _conv_world(hip, C_, pads, off, 37)
    t0, p0 = w.t.cpu().numpy(), w.p.cpu().numpy()
    wt_online = hip.empty(hip.conv_wt_floats(C_))
    hip.conv_wt_refresh(w.weights(w.p), C_, wt_online)
    wt_online0 = wt_online.clone()
    before = w.wt_t.clone()
    hip.target_blend(w.t, w.p, w.n, 0.25, None, 0, 1, w.weights(w.t), C_, w.wt_t)
    torch.cuda.synchronize()
    want = R.blend_nearest(t0, p0, 0.25)
    assert int(R.ulp_distance(w.t.cpu().numpy(), want).max()) <= 1 and not R.double_rounding_suspects(t0, p0, 0.25).any()
    assert np.array_equal(w.t.cpu().numpy(), want)
    fresh = torch.full_like(w.wt_t, float("nan"))
    hip.conv_wt_refresh(w.weights(w.t), C_, fresh)
    torch.cuda.synchronize()
    bad = (_bits(fresh) != _bits(w.wt_t)).nonzero().flatten().tolist()
    print(f"C={C_} pads={pads} off={off}: {len(bad)} of {fresh.numel()} dwords differ from a refresh, first {bad[:8]}")
    assert not bad
    assert not torch.equal(_bits(before), _bits(w.wt_t))
    assert torch.equal(w.p.cpu(), torch.from_numpy(p0)) and torch.equal(_bits(wt_online), _bits(wt_online0)), "the online side is only read"
    assert _guards_intact(w.tb, off, w.n) and _guards_intact(w.pb, off, w.n)


# ------------------------------------------------------------------------------------------------ 3. decision timing behind each tail form
HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-2 / 32)
TAU3 = 0.25
FORMS3 = ["plain", "plain-clip", "fold", "fold-clip", "tail"]


class _TailRig:
    """Seven updates of one tail form over tests/test_gpu_update_tail.py's world (conv1 | conv2 | conv3 | dense | not Adam's), every run from the same bytes."""

    def __init__(self, hip, form):
        import test_gpu_update_tail as UT
        self.UT, self.hip, self.form = UT, hip, form
        self.shape, self.B = (4, 36, 36), 8
        conv_end = 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64
        self.n, self.n_total = conv_end + 1700, conv_end + 1700 + 260
        gen = recipe.gen(91)
        f = lambda k: torch.from_numpy(gen.standard_normal(k).astype(np.float32)).to(hip.device)
        self.grads = [f(self.n_total + 4) for _ in range(7)]
        if form == "tail":
            net = self.net = hip.net(*self.shape)
            B = self.B
            self.frames = torch.from_numpy(recipe.make_frames(B, 5, self.shape)).to(hip.device).reshape(-1).contiguous()
            self.act1, self.act2 = f(B * net.H1 * net.W1 * 32).abs(), f(B * net.H2 * net.W2 * 64).abs()
            self.d3, self.d2, self.d1 = f(B * net.feat), f(B * net.H2 * net.W2 * 64), f(B * net.H1 * net.W1 * 32)
            self.segs = [(7, "vec"), (9, "count")]
            self.pend_slabs = f(sum((ns * UT.FORMS[fm][2] + 3) // 4 * 4 for ns, fm in self.segs) + 4)
            self.slabs = hip.empty(max(hip.encoder_bwd_scratch(net, B), 4))
        if form.endswith("clip"):
            self.partials = torch.zeros(256, dtype=torch.float64, device=hip.device)
            self.norm_ring = hip.zeros(5)

    def update(self, w, u, freq):
        """Update ``u`` of world ``w`` with the target period ``freq`` handed to the Adam form."""
        hip, UT = self.hip, self.UT
        w.g.copy_(self.grads[u])
        a = (w.p, w.g, w.m, w.v, self.n, w.state, w.scal, HP["lr"], HP["b1"], HP["b2"], HP["eps"], freq, w.t, self.n_total, None)
        fold = (w.weights(w.p), 4, w.wt, w.wt_t, w.loss, 8, w.ring)
        if self.form.endswith("clip"):
            hip.grad_norm_partials(w.g, self.n, self.partials)
            clip = (self.partials, 1.0, self.norm_ring)
            hip.adam_step_sync_clip(*a, *clip) if self.form == "plain-clip" else hip.adam_step_sync_wt_clip(*a, *fold, *clip)
        elif self.form == "plain":
            hip.adam_step_sync(*a)
        elif self.form == "fold":
            hip.adam_step_sync_wt(*a, *fold)
        else:
            o = w.off
            gs = (w.g[o[0]:o[1]], w.g[o[1]:o[2]], w.g[o[2]:w.conv_end])
            pend = UT._pend(w, self.segs, self.pend_slabs)
            plan = hip.encoder_wgrad_tail(self.net, w.weights(w.p), self.frames, None, self.frames.numel() // self.B, 0, self.B, self.act1, self.act2, self.d3, self.d2, self.d1,
                                          *gs, self.slabs, pend, w.state, w.scal, HP["lr"], HP["b1"], HP["b2"], freq)
            hip.update_tail(w.p, w.g, w.m, w.v, self.n, w.state, w.scal, HP["b1"], HP["b2"], HP["eps"], w.t, self.n_total, plan, w.weights(w.p), 4, w.wt, w.wt_t, w.loss, 8, w.ring)

    def blend(self, w, freq, force):
        self.hip.target_blend(w.t, w.p, self.n_total, TAU3, w.state, freq, force, w.weights(w.t), 4, w.wt_t)

    def world(self):
        return self.UT._World(self.hip, 4, self.n, self.n_total, 17)


@pytest.mark.parametrize("scenario", ["period3", "period1", "period3-nan"])
@pytest.mark.parametrize("form", FORMS3)
def test_decision_timing_behind_every_tail_form(hip, form, scenario):
    """The launch decides from the step count the tail form has committed.  period 3: blends after updates 3 and 6 only; period 1: after every update; period 3 with
    the NaN flag raised in front of update 4 (the count stays 3): updates 3, 4 and 7 — and update 4 leaves the parameters alone.  Expected bytes: a second run that
    hands the period 0 to everything and forces the blend by hand at those updates."""
    rig = _TailRig(hip, form)
    freq = 1 if scenario == "period1" else 3
    nan_at = {4} if scenario.endswith("nan") else set()
    blends = {"period3": {3, 6}, "period1": set(range(1, 8)), "period3-nan": {3, 4, 7}}[scenario]
    auto, hand = rig.world(), rig.world()
    changed = set()
    for u in range(1, 8):
        t_before, p_before = auto.t.clone(), auto.p.clone()
        for w in (auto, hand):
            if u in nan_at:
                w.state[0] = 1
            rig.update(w, u - 1, 0)
            if w is auto:
                rig.blend(w, freq, 0)
            elif u in blends:
                rig.blend(w, 0, 1)
        torch.cuda.synchronize()
        a, b = auto.everything(), hand.everything()
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"{form} {scenario}: update {u}: {k}"
        if not torch.equal(_bits(auto.t), _bits(t_before)):
            changed.add(u)
        st = auto.state.tolist()
        assert st[4] == 0 and st[0] == 0, f"update {u}: the Adam forms never hard-copy while tau is on: {st}"
        if u in nan_at:
            assert torch.equal(_bits(auto.p), _bits(p_before)) and st[2] == 1, "a NaN-skipped update leaves the parameters alone"
        else:
            assert not torch.equal(_bits(auto.p), _bits(p_before))
    assert changed == blends, f"{form} {scenario}: the target moved after updates {sorted(changed)}"
    assert auto.state[1].item() == 7 - len(nan_at)
    assert not torch.equal(auto.t, auto.p), "a blend, not a copy"
    fresh = hip.empty(hip.conv_wt_floats(4))
    hip.conv_wt_refresh(auto.weights(auto.t), 4, fresh)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fresh), _bits(auto.wt_t)), "the target's weight copies are those of the blended target"


# ------------------------------------------------------------------------------------------------ 4. learners
B = 8
TAU4 = 0.25


def _gc():
    import test_gpu_grad_clip as GC
    return GC


def _engine(cs, freq, **kw):
    from agent0_amd.common.utils import DeviceRng
    from agent0_amd.deepq.engine import DeviceLearner
    GC, c = _gc(), cs.c
    dev = DeviceLearner(cs.hip, cs.L, B, double_q=c.get("double_q", False), target_update_freq=freq, K=cs.K, N=cs.N, N_dash=cs.Nd, max_grad_norm=c.get("max_grad_norm", -1.0), **kw)
    dev.online.load_state_dict(recipe.make_state_dict(cs.spec, 11))
    dev.target.load_state_dict(recipe.make_state_dict(cs.spec, 12))
    rng = DeviceRng(cs.hip, GC.SEED)
    if cs.L.noisy:
        rng.reserve(rng.STREAM_NOISE, dev.online.noise_len); rng.reserve(rng.STREAM_NOISE, dev.target.noise_len)
    dev._test_rng = rng
    dev._test_taus = [cs.hip.empty(B * k) for k in (cs.K, cs.Nd, cs.N)] if cs.L.algo == "iqn" else None
    return dev


def _handle(cs, dev, freq):
    GC, c = _gc(), cs.c
    nat = cs.hip.native_learner(A=c["A"], dueling=c.get("dueling", False), double_q=c.get("double_q", False), B=B, discount=0.99, lr=5e-4, target_update_freq=freq,
                                algo=c["algo"], num_atoms=cs.L.T, vmin=dev.vmin, vmax=dev.vmax, noisy=c.get("noisy", False), seed=GC.SEED, K=cs.K, N=cs.N,
                                N_dash=cs.Nd, F=cs.L.F, max_grad_norm=c.get("max_grad_norm", -1.0))
    nat.set_params(dev.online.flat, dev.target.flat)
    return nat


def _all_of(dev):
    return dict(online=dev.online.flat, target=dev.target.flat, wt=dev.online.wt, wt_target=dev.target.wt, moment1=dev.adam_m, moment2=dev.adam_v, state=dev.state)


def _same(x, y, what):
    for k in x:
        assert torch.equal(_bits(x[k]), _bits(y[k])), f"{what}: {k}"


@pytest.mark.parametrize("clip", [-1.0, 50.0], ids=["plain", "clipped"])
@pytest.mark.parametrize("name", ["dqn", "rainbow-lite", "iqn", "fqf-fraction-clip"])
def test_learner_blends_where_the_hard_copy_was(hip, name, clip):
    """Four updates at target_update_freq = 2 with tau on == the same learner with the period out of reach and forced blends behind updates 2 and 4; the a0_learner
    handle equals both.  (fqf: the fraction net's block lies behind n_adam and is blended with the rest.)"""
    GC = _gc()
    assert list(GC.LEARNERS) == ["dqn", "rainbow-lite", "iqn", "fqf-fraction-clip"]
    cs = GC._Case(hip, name)
    auto, hand = _engine(cs, 2, target_tau=TAU4, clip_grad_norm=clip), _engine(cs, 10 ** 6, target_tau=TAU4, clip_grad_norm=clip)
    nat = _handle(cs, auto, 2)
    nat.set_target_tau(TAU4)
    nat.set_grad_clip(clip)
    assert auto.target.fused and auto.target_tau == TAU4
    t_start = auto.target.flat.clone()
    for s in range(4):
        t_before = auto.target.flat.clone()
        for dev in (auto, hand):
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        nat.update(*cs.batch(s))
        if s % 2 == 1:
            hand._blend_target(force=True)
        torch.cuda.synchronize()
        _same(_all_of(auto), _all_of(hand), f"{name}: update {s + 1}")
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, state=st), {k: _all_of(auto)[k] for k in ("online", "target", "moment1", "moment2", "state")}, f"{name}: handle, update {s + 1}")
        assert torch.equal(auto.target.flat, t_before) == (s % 2 == 0), f"update {s + 1}"
        assert auto.state[4].item() == 0
    assert auto.state[1].item() == 4
    # the whole module moved, the blocks Adam does not own included, and it is a blend: neither the old target nor the online network
    L = cs.L
    moved = auto.target.flat != t_start
    real = torch.zeros(L.n_params_padded, dtype=torch.bool, device=hip.device)
    for b in L.blocks.values():
        real[b.offset:b.offset + b.n_real * b.K] = True
    assert bool(moved[real].float().mean() > 0.9)
    if "frac" in L.blocks:
        assert bool(moved[L.blocks["frac"].all].any()), "the fraction net's block is blended too"
    assert not torch.equal(auto.target.flat, auto.online.flat)
    # both networks' weight copies are what a refresh builds
    for net in (auto.online, auto.target):
        fresh = hip.empty(net.wt.numel())
        hip.conv_wt_refresh(net.encoder_weights(), L.C, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(net.wt))
    nat.close()


@pytest.mark.parametrize("name", ["dqn", "rainbow-lite", "iqn", "fqf-fraction-clip"])
def test_tau_zero_is_the_learner_without_the_argument(hip, name):
    GC = _gc()
    cs = GC._Case(hip, name)
    off, none = _engine(cs, 2, target_tau=0.0), _engine(cs, 2)
    nat = _handle(cs, none, 2)
    nat.set_target_tau(0.0)
    nat.set_target_tau(-1.0)
    assert off.target_tau == 0.0 and none.target_tau == 0.0
    for s in range(4):
        for dev in (off, none):
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        nat.update(*cs.batch(s))
    torch.cuda.synchronize()
    _same(_all_of(off), _all_of(none), name)
    o, t, m, v, st = nat.get()
    _same(dict(online=o, target=t, moment1=m, moment2=v, state=st), {k: _all_of(none)[k] for k in ("online", "target", "moment1", "moment2", "state")}, f"{name}: handle")
    assert torch.equal(off.target.flat, off.online.flat) and off.state[4].item() == 1, "update 4 is a hard copy"
    nat.close()


# ------------------------------------------------------------------------------------------------ 5. the reference walk
def test_dqn_walks_with_the_oracle_that_takes_the_polyak_step(hip):
    """dqn at tests/test_gpu_trace.py's smallest batch (32), four free-running updates at target_update_freq = 2, tau = 0.25, against oracle.learner.OracleLearner with
    its sync replaced by the Polyak step (tests/target_tau_ref.py).  Bounds: that file's FREE_BOUNDS (18 free-running updates) — loss_rel and param_abs, the latter for
    the target too."""
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    from oracle import learner as olearner
    from oracle.losses import Hyper
    import test_gpu_trace as TR
    Bw, tau = TR.SMALL.B, 0.25
    spec = recipe.NetSpec("dqn", 4)
    L = NetLayout.from_spec(spec)
    dev = DeviceLearner(hip, L, Bw, target_update_freq=2, target_tau=tau)
    sd_o, sd_t = recipe.make_state_dict(spec, 11), recipe.make_state_dict(spec, 12)
    dev.online.load_state_dict(sd_o)
    dev.target.load_state_dict(sd_t)
    ora = R.polyak_oracle(olearner.OracleLearner)(spec, sd_o, sd_t, Hyper(), batch_size=Bw, target_update_freq=2, tau=tau)
    D = lambda x: torch.from_numpy(x).to(hip.device)
    t_first = {k: v.clone() for k, v in ora.pt.items()}
    for s in range(4):
        frames = recipe.make_frames(Bw, 61 + s, spec.obs_shape)
        a, r, d, w = recipe.make_transitions(Bw, spec.action_dim, 62 + s)
        loss = dev.update(D(frames.reshape(-1)), None, 2 * 4 * 84 * 84, D(a.astype(np.int32)), D(r), D(d.astype(np.float32)), D(w))
        torch.cuda.synchronize()
        res = ora.train(frames.reshape(Bw, -1), a, r, d.astype(np.float32), w, np.arange(Bw))
        loss_rel = float(((loss[:Bw].cpu() - res["q_loss"]).abs() / (res["q_loss"].abs() + 1e-3)).max())
        got, got_t = dev.online.state_dict(), dev.target.state_dict()
        param_abs = max(float((got[k].cpu() - ora.po[k].detach()).abs().max()) for k in ora.q_keys)
        target_abs = max(float((got_t[k].cpu() - ora.pt[k].detach()).abs().max()) for k in ora.q_keys)
        print(f"update {s + 1}: loss_rel {loss_rel:.3e} param_abs {param_abs:.3e} target_abs {target_abs:.3e}")
        assert loss_rel <= TR.FREE_BOUNDS["loss_rel"] and param_abs <= TR.FREE_BOUNDS["param_abs"] and target_abs <= TR.FREE_BOUNDS["param_abs"]
    # the walk has teeth: the oracle's target is far (in units of the bound) from both the untouched target and the hard copy
    far = lambda other: max(float((ora.pt[k].detach() - other[k].detach()).abs().max()) for k in ora.q_keys)
    assert far(t_first) > 1e3 * TR.FREE_BOUNDS["param_abs"] and far(ora.po) > 1e3 * TR.FREE_BOUNDS["param_abs"]


# ------------------------------------------------------------------------------------------------ 6. the Trainer
TAU6 = 0.25


def _el():
    import test_gpu_eps_ladder as EL
    return EL


def _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, tau=TAU6, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = parse_overrides([f"learner.algo={algo}", f"seed={seed}", f"logdir={tmp_path / tag}"] + ([f"learner.target_tau={tau}"] if tau is not None else []) + _el().BASE5 + list(extra))
    return Trainer(cfg, use_lp=use_lp)


def _state(tr):
    eng = tr.learner.engine
    return _el()._state(tr) + [eng.online.wt.clone(), eng.target.wt.clone()]


def _run(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, tau=TAU6, iters=6, dp=False):
    from agent0_amd.deepq.native_loop import NativeLoop
    EL = _el()
    tr = _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, tau)
    hook = EL._install_exchange(tr) if dp else None
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    out = _state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count
    assert res[-1]["loss"] is not None, "updates ran"
    EL._close_exchange(tr, hook) if dp else EL._close(tr)
    return out


@pytest.mark.parametrize("mode,algo,extra", [("main", "dqn", []), ("launch", "dqn", []), ("dp", "dqn", []),
                                             ("main", "c51", ["learner.noisy_net=true", "learner.dueling_head=true", "learner.n_step_q=3"])],
                         ids=["main-dqn", "launch-dqn", "dp-dqn", "main-c51-noisy-duel-n3"])
def test_handles_and_python_classes_end_on_the_same_state(mode, algo, extra, tmp_path, monkeypatch):
    """Six iterations, three updates each once training has started, target_update_freq = 4: at least two blends.  ``dp``: a one-rank RCCL group (A0_DP_FORCE=1)."""
    import torch.distributed as dist
    EL = _el()
    dp = mode == "dp"
    if dp:
        EL._one_rank_group(monkeypatch)
    try:
        a = _run(tmp_path, monkeypatch, False, algo, extra, mode == "launch", "py", dp=dp)
        b = _run(tmp_path, monkeypatch, True, algo, extra, mode == "launch", "nat", dp=dp)
    finally:
        if dp:
            dist.destroy_process_group()
    EL._assert_same_run(a, b)
    online, target, state = a[0][0], a[0][1], a[0][4]
    assert state[1].item() >= 8 and state[4].item() == 0 and not torch.equal(online, target)
    if mode == "main" and algo == "dqn":
        hard = _run(tmp_path, monkeypatch, True, algo, extra, False, "hard", tau=None)
        assert hard[0][4][1].item() == state[1].item() and not torch.equal(hard[0][1], target), "the setting changes the target"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    EL = _el()
    want = _run(tmp_path, monkeypatch, native, "dqn", [], False, "a")
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "b")
    for _ in range(3):
        tr.run_iteration()
    assert tr.learner.engine.state[1].item() % 4 != 0, "between two blends"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    EL._close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "c", seed=7)
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(3)]
    got = _state(tr)
    EL._close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][3:]


def test_setting_off_changes_no_key_no_header_and_no_log_line(tmp_path, monkeypatch):
    GC = _gc()
    tr = GC._trainer(tmp_path, monkeypatch, True, "off")
    eng = tr.learner.engine
    assert eng.target_tau == 0.0 and eng._hard_freq() == eng.target_update_freq == 5
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    assert list(res.keys()) == GC.TODAYS_HEADER[:-1] + ["fps"] and res["loss"] is not None
    GC._close(tr)
    with open(tmp_path / "off" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == GC.TODAYS_HEADER and len(rows) == 3
    assert "target_tau" not in open(tmp_path / "off" / "msg.log").read()
    # ... and on: the same keys and header (no new statistic)
    tr = GC._trainer(tmp_path, monkeypatch, True, "on", extra=["learner.target_tau=0.25"])
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    assert list(res.keys()) == GC.TODAYS_HEADER[:-1] + ["fps"]
    GC._close(tr)
    with open(tmp_path / "on" / "progress.csv") as f:
        assert list(csv.reader(f))[0] == GC.TODAYS_HEADER


def test_the_learner_refuses_the_hard_copy_as_tau(hip):
    cs = _gc()._Case(hip, "dqn")
    with pytest.raises(ValueError, match=r"learner\.target_tau"):
        _engine(cs, 2, target_tau=1.0)


# ------------------------------------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_are_refused(hip):
    from agent0_amd import _abi
    from agent0_amd._abi import A0Error
    w = _conv_world(hip, 4, (0, 0, 0), 0, 37)
    t0, wt0 = w.t.clone(), w.wt_t.clone()
    lib = hip.lib
    EINVAL = -1
    tp, pp = w.t.data_ptr(), w.p.data_ptr()
    assert lib.a0_target_blend(None, pp, w.n, 0.5, None, 0, 1, None, 0, None, None) == EINVAL and "a0_target_blend" in _abi.last_error()
    assert lib.a0_target_blend(tp, None, w.n, 0.5, None, 0, 1, None, 0, None, None) == EINVAL
    assert lib.a0_target_blend(tp, pp, w.n, 0.5, None, 3, 0, None, 0, None, None) == EINVAL, "no state block and no force"
    for tau in (1.0, 1.5, float("inf")):
        assert lib.a0_target_blend(tp, pp, w.n, tau, None, 0, 1, None, 0, None, None) == EINVAL and "tau" in _abi.last_error()
        with pytest.raises(A0Error):
            hip.target_blend(w.t, w.p, w.n, tau, None, 0, 1)
    big = hip.empty(hip.conv_wt_floats(4) + 4)
    with pytest.raises(A0Error, match="16-byte aligned"):
        hip.target_blend(w.t, w.p, w.n, 0.5, None, 0, 1, w.weights(w.t), 4, big[1:])
    with pytest.raises(A0Error, match="inside target"):
        hip.target_blend(w.t, w.p, w.n, 0.5, None, 0, 1, w.weights(w.p), 4, w.wt_t)
    torch.cuda.synchronize()
    assert torch.equal(_bits(w.t), _bits(t0)) and torch.equal(_bits(w.wt_t), _bits(wt0)), "a refused call launches nothing"
    # the handle's setter: tau >= 1, and after an update
    GC = _gc()
    cs = GC._Case(hip, "dqn")
    dev = _engine(cs, 2)
    nat = _handle(cs, dev, 2)
    with pytest.raises(A0Error, match="a0_learner_set_target_tau"):
        nat.set_target_tau(1.0)
    nat.set_target_tau(0.25)
    nat.update(*cs.batch(0))
    torch.cuda.synchronize()
    with pytest.raises(A0Error, match="a0_learner_set_target_tau"):
        nat.set_target_tau(0.5)
    assert lib.a0_learner_set_target_tau(nat.h, 0.5) == EINVAL
    nat.close()
