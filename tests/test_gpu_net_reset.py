"""GPU (MI355X): periodic shrink-and-perturb network resets (``learner.net_reset_freq`` / ``learner.net_reset_shrink``): a0_net_reset and everything that issues it.

1. the kernel against the reference (tests/net_reset_ref.py): fresh values from a0_rng_normal / a0_rng_uniform fills of Philox stream 8 at position k * n_total + i;
   replaced and constant elements byte for byte, kept ones untouched, blended ones the float nearest to phi + a32 * fl32(p - phi) in float64 except at that
   reference's double roundings (tests/target_tau_ref.py), where one ulp is allowed; zero moments over [0, n_adam), target == online, state[7] == state[1].
2. no reset changes no byte.   3. both weight copies == a0_net_conv_wt_refresh of the new parameters.   4. the draws.
5. decision timing behind every Adam form, and the t = 1 scalars of the update after a reset.   6. bad arguments.
7. DeviceLearner and the a0_learner handle: the reset at the right update, a fresh optimizer afterwards; off == the learner without the argument.
8. the Trainer: handles == Python classes (eager and hipGraph) on main, launch and one-rank data parallelism; snapshots across a reset; the statistic.

Work split of the kernel (csrc/net_reset.hip): a lane owns four consecutive elements; 16 bytes at once where the buffers are 16-byte aligned and the four lie inside one
segment (or between two) and the reset's first draw position k * n_total is a multiple of four, element by element otherwise.  Shapes: 5 (one group and a tail of one), 1025 (two workgroups, a tail of one), 77 824 + 37 (C = 4's three
convolution blocks and a ragged tail: 77 workgroups); every table below has segment boundaries off the 16-byte grid."""
import csv
import math

import numpy as np
import pytest
import torch

import net_reset_ref as R
import recipe
import target_tau_ref as TT

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SEED = 0x9E3779B1
ALPHAS = [0.0, 0.2, 0.5, 0.8, 1.0]
P_STD, PHI_STD = 0.05, 0.025
UNI_BOUND = PHI_STD * math.sqrt(3.0)      # a uniform in +-b has std b / sqrt(3)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "net_reset")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


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


# ------------------------------------------------------------------------------------------------ 1. the kernel against the reference
def _table(n):
    """(n_adam, segments): every kind with and without the keep flag, boundaries off the 16-byte grid, a noisy-bias pair (13 real entries, 19 padded), a gap without
    a rule inside [0, n_adam) and a range behind n_adam."""
    if n == 5:
        return 4, [(0, 2, R.NORMAL, PHI_STD, 1), (2, 1, R.CONST, 0.125, 0), (3, 1, R.UNIFORM, UNI_BOUND, 1)]
    n_adam = n - n // 8 - 1
    c = [0, 7, n_adam * 2 // 10 + 1, n_adam * 3 // 10 + 2, n_adam * 5 // 10 + 3, n_adam * 6 // 10]
    rules = [(R.NORMAL, PHI_STD, 1), (R.CONST, 0.0, 1), (R.UNIFORM, UNI_BOUND, 1), (R.NORMAL, PHI_STD, 0), (R.CONST, 0.0625, 0)]
    segs = [(c[i], c[i + 1] - c[i]) + rules[i] for i in range(5)]
    at = c[5]
    segs += [(at, 13, R.UNIFORM, UNI_BOUND, 0), (at + 13, 19, R.CONST, 0.0, 0)]
    at += 32
    mid = n_adam * 8 // 10 + 1
    segs += [(at, mid - at, R.UNIFORM, UNI_BOUND, 1), (mid, n_adam - 6 - mid, R.NORMAL, PHI_STD, 1)]      # [n_adam - 6, n_adam): no rule
    return n_adam, segs


_INPUTS = {}


def _inputs(n):
    """(p, m, v) as fp32 numpy arrays — cached, never modified."""
    if n not in _INPUTS:
        g = recipe.gen(3000 + n % 9973)
        _INPUTS[n] = ((g.standard_normal(n) * P_STD).astype(np.float32), (g.standard_normal(n) * 1e-3).astype(np.float32), np.abs(g.standard_normal(n) * 1e-3).astype(np.float32))
    return _INPUTS[n]


_PHI = {}


def _phi(hip, n, segs, seed, k):
    """The fresh values of every normal and uniform segment, from fills at the stated positions (numpy, cached)."""
    key = (n, tuple(segs), seed, k)
    if key not in _PHI:
        phi = np.zeros(n, np.float32)
        for off, cnt, kind, scale, keep in segs:
            if kind == R.CONST:
                continue
            out = hip.empty(cnt)
            if kind == R.NORMAL:
                hip.rng_normal(seed & 0xFFFFFFFF, R.STREAM_RESET, k * n + off, scale, out, cnt)
                phi[off:off + cnt] = out.cpu().numpy()
            else:
                hip.rng_uniform(seed & 0xFFFFFFFF, R.STREAM_RESET, k * n + off, out, cnt)
                phi[off:off + cnt] = R.uniform_fresh(scale, out.cpu().numpy())
        _PHI[key] = phi
    return _PHI[key]


def _check_against_reference(got, p, phi, segs, alpha, what):
    want, exact, suspects = R.expect(p, phi, segs, alpha)
    dist = TT.ulp_distance(got, want)
    worst = int(dist.argmax())
    n_blend = int((~exact).sum())
    print(f"{what}: worst {int(dist.max())} ulp at {worst} (p {p[worst]!r} phi {phi[worst]!r} got {got[worst]!r} want {want[worst]!r}); blended {n_blend}, "
          f"non-nearest {int((dist != 0).sum())}, double-rounding suspects {int(suspects.sum())}")
    assert np.array_equal(got.view(np.int32)[exact], want.view(np.int32)[exact]), "kept elements are untouched bytes, replaced and constant ones are the fill's bytes"
    assert int(dist.max()) <= 1 and not ((dist != 0) & ~suspects).any(), "a blended element that is not the nearest float although the reference rounds once there"
    assert int(suspects.sum()) <= 1e-5 * got.size, "the inputs keep the reference's double roundings out"
    return want


@pytest.mark.parametrize("k", [1, 4], ids=["k1-elementwise", "k4-16-byte-path-where-aligned"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", [5, 1025, 77824 + 37])
def test_kernel_against_the_reference(hip, n, off, alpha, k):
    """Which path a case takes: the kernel moves 16 bytes per lane only where the buffers are 16-byte aligned AND the first draw position k * n_total is a multiple of
    four (the four elements then share one Philox block).  All three lengths are 1 mod 4, so k = 4 on aligned buffers is the 16-byte path — with the off-grid
    boundaries, the 13 / 19 noisy-bias split, the kept uniform segment and the gap that straddles n_adam handled element by element inside it — and k = 1, like every
    offset4 case, is element by element throughout.  Both must give the reference's bytes."""
    assert (k * n) % 4 == (0 if k == 4 else 1)
    n_adam, segs = _table(n)
    p, m, v = _inputs(n)
    phi = _phi(hip, n, segs, SEED, k)
    g = recipe.gen(17)
    pb, pv = _guarded(hip, p, off)
    tb, tv = _guarded(hip, (g.standard_normal(n) * P_STD).astype(np.float32), off)
    mb, mv = _guarded(hip, m, off)
    vb, vv = _guarded(hip, v, off)
    state = torch.tensor([0, 11, 2, 0, 1, 11, 9, 4], dtype=torch.int32, device=hip.device)
    hip.net_reset(pv, tv, mv, vv, n_adam, n, segs, alpha, SEED, state, 0, True, k)
    torch.cuda.synchronize()
    got = pv.cpu().numpy()
    _check_against_reference(got, p, phi, segs, alpha, f"n={n} off={off} alpha={alpha} k={k}")
    assert np.array_equal(got[n_adam:], p[n_adam:]) and (n == 5 or np.array_equal(got[n_adam - 6:n_adam], p[n_adam - 6:n_adam])), "no rule, no change"
    assert torch.equal(_bits(tv), _bits(pv)), "target bytes == online bytes over [0, n_total)"
    assert not mv[:n_adam].any() and not vv[:n_adam].any(), "zero moments over [0, n_adam)"
    assert np.array_equal(mv[n_adam:].cpu().numpy(), m[n_adam:]) and np.array_equal(vv[n_adam:].cpu().numpy(), v[n_adam:]), "... and untouched behind"
    assert state.tolist() == [0, 11, 2, 0, 1, 11, 9, 11], "state[7] <- state[1]; the other words are only read"
    for buf in (pb, tb, mb, vb):
        assert _guards_intact(buf, off, n), "nothing outside the buffers is touched"


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
def test_no_reset_changes_no_byte(hip, off):
    """force = 0 and: the step count not a multiple of N; the step count 0; state[3] == 1 at a multiple; N = 0.  Then a multiple with state[3] == 0 resets."""
    w = _world(hip, 4, (0, 0, 0), off, 37)
    before = {k: x.clone() for k, x in w.everything().items()}
    for steps, skip, freq in ((4, 0, 3), (5, 0, 3), (1, 0, 2), (0, 0, 3), (0, 0, 1), (6, 1, 3), (3, 1, 1), (6, 0, 0)):
        state = torch.tensor([0, steps, 1, skip, 0, steps, 3, 2], dtype=torch.int32, device=hip.device)
        s0 = state.clone()
        w.reset(0.5, state, freq, False, 0)
        torch.cuda.synchronize()
        for k, x in w.everything().items():
            assert torch.equal(_bits(x), _bits(before[k])), (steps, skip, freq, k)
        assert torch.equal(state, s0), "the state block too"
    state = torch.tensor([0, 6, 1, 0, 0, 6, 3, 2], dtype=torch.int32, device=hip.device)
    w.reset(0.5, state, 3, False, 0)
    torch.cuda.synchronize()
    assert state.tolist() == [0, 6, 1, 0, 0, 6, 3, 6] and not torch.equal(w.p, before["params"]) and not w.m[:w.n_adam].any() and w.m[w.n_adam:].any()
    forced = _world(hip, 4, (0, 0, 0), off, 37)
    forced.reset(0.5, None, 0, True, 2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(forced.p), _bits(w.p)), "k = state[1] / N"


# ------------------------------------------------------------------------------------------------ 3. weight copies
class _World:
    """Online and target flat buffers laid out [pad0 | w1 b1 | pad1 | w2 b2 | pad2 | w3 b3 | dense | tail], moments, both networks' weight copies, and the table:
    the convolution blocks keep a share, the dense block is replaced, pads and tail have no rule."""

    def __init__(self, hip, C_, pads, off, tail):
        g = recipe.gen(41 + C_ + sum(pads) + off)
        K1 = 64 * C_
        sizes = [pads[0], 32 * K1, 32, pads[1], 64 * 512, 64, pads[2], 64 * 576, 64, 259, tail]
        at = np.cumsum([0] + sizes)
        self.hip, self.C, self.off = hip, C_, off
        self.n, self.n_adam = int(at[-1]), int(at[-2])
        self.o = dict(w1=(at[1], at[2]), b1=(at[2], at[3]), w2=(at[4], at[5]), b2=(at[5], at[6]), w3=(at[7], at[8]), b3=(at[8], at[9]))
        self.segs = []
        for wk, bk in (("w1", "b1"), ("w2", "b2"), ("w3", "b3")):
            self.segs += [(int(self.o[wk][0]), int(self.o[wk][1] - self.o[wk][0]), R.NORMAL, PHI_STD, 1), (int(self.o[bk][0]), int(self.o[bk][1] - self.o[bk][0]), R.CONST, 0.0, 1)]
        self.segs.append((int(at[9]), 259, R.NORMAL, PHI_STD, 0))
        f = lambda s: (g.standard_normal(self.n) * s).astype(np.float32)
        self.pb, self.p = _guarded(hip, f(P_STD), off)
        self.tb, self.t = _guarded(hip, f(P_STD), off)
        self.mb, self.m = _guarded(hip, f(1e-3), off)
        self.vb, self.v = _guarded(hip, np.abs(f(1e-3)), off)
        self.wt, self.wt_t = hip.empty(hip.conv_wt_floats(C_)), hip.empty(hip.conv_wt_floats(C_))
        hip.conv_wt_refresh(self.weights(self.p), C_, self.wt)
        hip.conv_wt_refresh(self.weights(self.t), C_, self.wt_t)
        torch.cuda.synchronize()

    def weights(self, flat):
        return {k: flat[a:b] for k, (a, b) in self.o.items()}

    def reset(self, alpha, state, freq, force, k, seed=SEED):
        self.hip.net_reset(self.p, self.t, self.m, self.v, self.n_adam, self.n, self.segs, alpha, seed, state, freq, force, k, self.weights(self.p), self.C, self.wt, self.wt_t)

    def everything(self):
        return dict(params=self.p, target=self.t, exp_avg=self.m, exp_avg_sq=self.v, wt=self.wt, wt_target=self.wt_t, guards_p=self.pb, guards_t=self.tb, guards_m=self.mb, guards_v=self.vb)


def _world(hip, C_, pads, off, tail):
    return _World(hip, C_, pads, off, tail)


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("pads", [(0, 0, 0), (4, 0, 8), (1, 0, 0), (0, 2, 0), (0, 0, 3)], ids=lambda p: "pads%d-%d-%d" % p)
@pytest.mark.parametrize("C_", [4, 1])
def test_both_weight_copies_are_those_of_the_new_parameters(hip, C_, pads, off, alpha):
    """Convolution blocks at multiples of four floats (four weights of a row per lane) and not (weight by weight), on the 16-byte path and on the element path.
    alpha = 1: the online parameters and their copies keep their bytes, and the target's copies still become the online network's."""
    w = _world(hip, C_, pads, off, 37)
    p0, wt0, wt_t0 = w.p.cpu().numpy(), w.wt.clone(), w.wt_t.clone()
    w.reset(alpha, None, 0, True, 3)
    torch.cuda.synchronize()
    _check_against_reference(w.p.cpu().numpy(), p0, _phi(hip, w.n, w.segs, SEED, 3), w.segs, alpha, f"C={C_} pads={pads} off={off} alpha={alpha}")
    fresh = torch.full_like(w.wt, float("nan"))
    hip.conv_wt_refresh(w.weights(w.p), C_, fresh)
    torch.cuda.synchronize()
    for name, got in (("wt", w.wt), ("wt_target", w.wt_t)):
        bad = (_bits(fresh) != _bits(got)).nonzero().flatten().tolist()
        print(f"C={C_} pads={pads} off={off} alpha={alpha} {name}: {len(bad)} of {fresh.numel()} dwords differ from a refresh, first {bad[:8]}")
        assert not bad
    assert torch.equal(_bits(w.wt), _bits(wt0)) == (alpha == 1.0) and not torch.equal(_bits(w.wt_t), _bits(wt_t0))
    assert torch.equal(_bits(w.t), _bits(w.p)) and not w.m[:w.n_adam].any() and not w.v[:w.n_adam].any()
    for buf in (w.pb, w.tb, w.mb, w.vb):
        assert _guards_intact(buf, off, w.n)


# ------------------------------------------------------------------------------------------------ 4. the draws
def test_draws_are_a_function_of_seed_and_reset_number(hip):
    n = 77824 + 37
    n_adam, segs = _table(n)
    p, m, v = _inputs(n)

    def run(seed, k, alpha=0.0):
        D = lambda a: torch.from_numpy(a.copy()).to(hip.device)
        pv, tv, mv, vv = D(p), D(p), D(m), D(v)
        hip.net_reset(pv, tv, mv, vv, n_adam, n, segs, alpha, seed, None, 0, True, k)
        torch.cuda.synchronize()
        return pv.cpu().numpy()

    a = run(SEED, 2)
    assert np.array_equal(a.view(np.int32), run(SEED, 2).view(np.int32)), "the same (seed, k): the same bytes"
    assert np.array_equal(a.view(np.int32), run(SEED | (0xABC << 32), 2).view(np.int32)), "seed bits above 32 are ignored"
    drawn = np.zeros(n, bool)
    for off, cnt, kind, scale, keep in segs:
        if kind != R.CONST:
            drawn[off:off + cnt] = True
    for other in (run(SEED, 3), run(SEED + 1, 2)):
        assert float((other[drawn] != a[drawn]).mean()) > 0.99, "another k, another seed: other draws"
        assert np.array_equal(other[~drawn], a[~drawn])
    for off, cnt, kind, scale, keep in segs:
        x = a[off:off + cnt].astype(np.float64)
        if kind == R.NORMAL and cnt >= 64:
            rms = math.sqrt(float((x * x).mean()))
            print(f"normal segment at {off} ({cnt}): sample RMS {rms:.6f}, std {scale}")
            assert abs(rms / scale - 1.0) <= 5.0 / math.sqrt(2.0 * cnt)
        elif kind == R.UNIFORM and cnt >= 64:
            assert np.abs(x).max() <= scale and np.abs(x).max() > 0.9 * scale and abs(x.mean()) < 5.0 * scale / math.sqrt(3.0 * cnt)


# ------------------------------------------------------------------------------------------------ 5. decision timing behind every Adam form
FORMS5 = ["plain", "plain-clip", "fold", "fold-clip", "tail", "adam"]


def _rig(hip, form):
    import test_gpu_target_tau as T

    class Rig(T._TailRig):
        def update(self, w, u, freq):
            if self.form != "adam":
                return super().update(w, u, freq)
            w.g.copy_(self.grads[u])
            hip.adam_step(w.p, w.g, w.m, w.v, self.n, w.state, w.scal, T.HP["lr"], T.HP["b1"], T.HP["b2"], T.HP["eps"], freq)

        def table(self, w):
            o = w.off + [w.conv_end]
            K = [64 * 4, 512, 576]
            N = [32, 64, 64]
            segs = []
            for i in range(3):
                segs += [(o[i], N[i] * K[i], R.NORMAL, PHI_STD, 1), (o[i] + N[i] * K[i], N[i], R.CONST, 0.0, 1)]
            return segs + [(w.conv_end, self.n - w.conv_end, R.NORMAL, PHI_STD, 0)]

        def reset(self, w, freq, force, k):
            hip.net_reset(w.p, w.t, w.m, w.v, self.n, self.n_total, self.table(w), 0.5, SEED, w.state, freq, force, k, w.weights(w.p), 4, w.wt, w.wt_t)

    return Rig(hip, form), T.HP


@pytest.mark.parametrize("scenario", ["period3", "period1", "period3-nan"])
@pytest.mark.parametrize("form", FORMS5)
def test_decision_timing_behind_every_adam_form(hip, form, scenario):
    """The launch decides from what the Adam form has committed.  period 3: resets after updates 3 and 6 only; period 1: after every update; period 3 with the NaN
    flag raised in front of update 4 (the count stays 3, state[3] is 1): after update 3, NOT again after update 4, then after update 7 (count 6).  Expected bytes: a
    second run that never resets by itself and is reset by hand (force, k) at those updates.  The update after a reset derives the scalars of t = 1."""
    rig, HP = _rig(hip, form)
    freq = 1 if scenario == "period1" else 3
    nan_at = {4} if scenario.endswith("nan") else set()
    resets = {"period3": {3: 1, 6: 2}, "period1": {u: u for u in range(1, 8)}, "period3-nan": {3: 1, 7: 2}}[scenario]
    auto, hand = rig.world(), rig.world()
    fired = set()
    t1 = (HP["lr"] / (1.0 - HP["b1"]), math.sqrt(1.0 - HP["b2"]))
    last_reset = 0
    for u in range(1, 8):
        for w in (auto, hand):
            if u in nan_at:
                w.state[0] = 1
            rig.update(w, u - 1, 0)
            if w is auto:
                rig.reset(w, freq, False, 0)
            elif u in resets:
                rig.reset(w, 0, True, resets[u])
        torch.cuda.synchronize()
        a, b = auto.everything(), hand.everything()
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"{form} {scenario}: update {u}: {k}"
        st = auto.state.tolist()
        if u not in nan_at:
            # the scalars this update stepped with: t counts from the last reset (state[7] as the Adam form read it); pow() on the device against Python's: 1e-6
            t = st[1] - last_reset
            want = (HP["lr"] / (1.0 - HP["b1"] ** t), math.sqrt(1.0 - HP["b2"] ** t))
            got = tuple(float(x) for x in auto.scal[:2].cpu())
            assert got == pytest.approx(want, rel=1e-6), f"update {u}: t = {t}: scalars {got}, expected {want}"
            if last_reset and st[1] == last_reset + 1:
                assert got == pytest.approx(t1, rel=1e-6), "the update after a reset steps with the scalars of t = 1"
        if st[7] != last_reset:
            fired.add(u)
            assert st[7] == st[1] and not auto.m.any() and not auto.v.any() and torch.equal(_bits(auto.t), _bits(auto.p))
            last_reset = st[7]
        else:
            assert auto.m.any() or u in nan_at
    assert fired == set(resets), f"{form} {scenario}: resets after updates {sorted(fired)}"
    assert auto.state[1].item() == 7 - len(nan_at) and auto.state[2].item() == len(nan_at)
    if form in ("plain", "plain-clip", "adam") and 7 not in resets:
        return          # these Adam forms keep no weight copies: only a reset writes them, and update 7 moved the parameters afterwards
    for wt, flat in ((auto.wt, auto.p), (auto.wt_t, auto.t)):
        fresh = hip.empty(hip.conv_wt_floats(4))
        hip.conv_wt_refresh(auto.weights(flat), 4, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(wt)), "the weight copies are those of the parameters"


# ------------------------------------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_are_refused(hip):
    from agent0_amd._abi import A0Error
    w = _world(hip, 4, (0, 0, 0), 0, 37)
    before = {k: x.clone() for k, x in w.everything().items()}
    a = (w.p, w.t, w.m, w.v, w.n_adam, w.n)
    with pytest.raises(A0Error, match="state"):
        hip.net_reset(*a, w.segs, 0.5, SEED, None, 3, False, 0)          # neither a state block nor force: the binding asks for the tensor ...
    assert hip.lib.a0_net_reset(w.p.data_ptr(), w.t.data_ptr(), w.m.data_ptr(), w.v.data_ptr(), w.n_adam, w.n, None, 0, 0.5, SEED, None, 3, 0, 0, None, 0, None, None, None) == -1
    from agent0_amd import _abi
    assert "a0_net_reset" in _abi.last_error()                           # ... and so does the library
    for alpha in (-0.5, 1.5, float("nan")):
        with pytest.raises(A0Error, match="alpha"):
            hip.net_reset(*a, w.segs, alpha, SEED, None, 0, True, 0)
    with pytest.raises(A0Error, match="ascending"):
        hip.net_reset(*a, list(reversed(w.segs)), 0.5, SEED, None, 0, True, 0)
    with pytest.raises(A0Error, match="ascending"):
        hip.net_reset(*a, [(0, w.n_adam + 1, R.NORMAL, 0.1, 0)], 0.5, SEED, None, 0, True, 0)
    with pytest.raises(A0Error, match="kind"):
        hip.net_reset(*a, [(0, 8, 7, 0.1, 0)], 0.5, SEED, None, 0, True, 0)
    with pytest.raises(A0Error):
        hip.net_reset(*a, [(i, 1, R.CONST, 0.0, 0) for i in range(33)], 0.5, SEED, None, 0, True, 0)
    with pytest.raises(A0Error, match="a0_net_reset"):
        hip.net_reset(*a, w.segs, 0.5, SEED, None, 0, True, -1)
    big = hip.empty(hip.conv_wt_floats(4) + 4)
    with pytest.raises(A0Error, match="16-byte aligned"):
        hip.net_reset(*a, w.segs, 0.5, SEED, None, 0, True, 0, w.weights(w.p), 4, big[1:], w.wt_t)
    with pytest.raises(A0Error, match="inside params"):
        hip.net_reset(*a, w.segs, 0.5, SEED, None, 0, True, 0, w.weights(w.t), 4, w.wt, w.wt_t)
    torch.cuda.synchronize()
    for k, x in w.everything().items():
        assert torch.equal(_bits(x), _bits(before[k])), f"a refused call launches nothing: {k}"
    # the handle's setter: range checks, and the setting is fixed once an update has run
    import test_gpu_target_tau as T
    cs = T._gc()._Case(hip, "dqn")
    dev = T._engine(cs, 2)
    nat = T._handle(cs, dev, 2)
    for freq, shrink in ((-1, 0.5), (3, -0.1), (3, 1.5), (3, float("nan"))):
        with pytest.raises(A0Error, match="a0_learner_set_net_reset"):
            nat.set_net_reset(freq, shrink, SEED)
    nat.set_net_reset(3, 0.5, SEED)
    nat.set_net_reset(0, 1.0, SEED)
    nat.update(*cs.batch(0))
    torch.cuda.synchronize()
    with pytest.raises(A0Error, match="a0_learner_set_net_reset"):
        nat.set_net_reset(3, 0.5, SEED)
    nat.close()


# ------------------------------------------------------------------------------------------------ 7. learners
B = 8
NAMES = ["dqn", "rainbow-lite", "iqn", "fqf-fraction-clip"]
FAR = 10 ** 6      # a target period out of reach: no copy interferes


def _tt():
    import test_gpu_target_tau as T
    return T


def _engine(cs, **kw):
    from agent0_amd.common.utils import DeviceRng
    T = _tt()
    rng = DeviceRng(cs.hip, T._gc().SEED)
    return T._engine(cs, FAR, aug_rng=rng, **kw)


@pytest.mark.parametrize("clip", [-1.0, 50.0], ids=["plain", "clipped"])
@pytest.mark.parametrize("name", NAMES)
def test_reset_at_the_right_update_then_a_fresh_optimizer(hip, name, clip):
    """net_reset_freq = 3, shrink = 0.5 beside a twin without the setting and the a0_learner handle with it: equal bytes through update 2; after update 3 the learner
    is the reference reset of the twin; update 4 is, bit for bit, the first update of a new learner holding the reset parameters, zero moments and a zero step count."""
    T = _tt()
    GC = T._gc()
    assert list(GC.LEARNERS) == NAMES and GC.B == B
    cs = GC._Case(hip, name)
    auto, twin = _engine(cs, clip_grad_norm=clip, net_reset_freq=3, net_reset_shrink=0.5), _engine(cs, clip_grad_norm=clip)
    nat = T._handle(cs, auto, FAR)
    nat.set_grad_clip(clip)
    nat.set_net_reset(3, 0.5, auto.reset_seed())
    L = cs.L
    assert nat.net_reset_segs() == [(o, c, k, float(np.float32(s)), kp) for o, c, k, s, kp in L.reset_segments()], "the handle builds the same table"
    assert auto.reset_seed() == GC.SEED & 0xFFFFFFFF and twin.reset_segs is None

    def handle_equals(dev, what, skip_state=False):
        o, t, m, v, st = nat.get()
        mine = {k: T._all_of(dev)[k] for k in ("online", "target", "moment1", "moment2", "state")}
        T._same({k: x for k, x in dict(online=o, target=t, moment1=m, moment2=v, state=st).items() if not (skip_state and k == "state")},
                {k: x for k, x in mine.items() if not (skip_state and k == "state")}, what)

    for s in range(2):
        for dev in (auto, twin):
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        nat.update(*cs.batch(s))
        torch.cuda.synchronize()
        T._same(T._all_of(auto), T._all_of(twin), f"{name}: update {s + 1}")
        handle_equals(auto, f"{name}: handle, update {s + 1}")
        assert auto.state[7].item() == 0
    for dev in (auto, twin):
        dev.update(*cs.batch(2), rand=cs.draws(dev))
    nat.update(*cs.batch(2))
    torch.cuda.synchronize()
    # ---- update 3: the reference reset applied to the twin
    segs = L.reset_segments()
    p_twin = twin.online.flat.cpu().numpy()
    phi = _phi(hip, L.n_params_padded, segs, auto.reset_seed(), 1)
    got = auto.online.flat.cpu().numpy()
    _check_against_reference(got, p_twin, phi, segs, 0.5, f"{name} clip={clip}")
    assert not np.array_equal(got[:L.conv_end], p_twin[:L.conv_end]) and np.array_equal(got[L.n_adam:], p_twin[L.n_adam:]), "the encoder moved; the fraction net did not"
    assert torch.equal(_bits(auto.target.flat), _bits(auto.online.flat)) and not auto.adam_m[:L.n_adam].any() and not auto.adam_v[:L.n_adam].any()
    assert twin.adam_m[:L.n_adam].any() and auto.state.tolist()[:4] == twin.state.tolist()[:4] and auto.state[7].item() == 3 and twin.state[7].item() == 0
    if "frac" in L.blocks:
        assert torch.equal(auto.rms_sq, twin.rms_sq) and auto.rms_sq.any(), "the fraction net's RMSprop state is not touched"
    for net in (auto.online, auto.target):
        fresh = hip.empty(net.wt.numel())
        hip.conv_wt_refresh(net.encoder_weights(), L.C, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(net.wt))
    handle_equals(auto, f"{name}: handle, update 3")
    # ---- update 4 == update 1 of a new learner
    new = _engine(cs, clip_grad_norm=clip)
    new.online.flat.copy_(auto.online.flat); new.target.flat.copy_(auto.target.flat)
    new.online.refresh_wt(); new.target.refresh_wt()
    new._test_rng.offsets = dict(auto._test_rng.offsets)          # the fourth update's noise and fractions
    if "frac" in L.blocks:
        new.rms_sq.copy_(auto.rms_sq)
    assert not new.adam_m.any() and not new.state.any()
    for dev in (auto, new):
        dev.update(*cs.batch(3), rand=cs.draws(dev))
    nat.update(*cs.batch(3))
    torch.cuda.synchronize()
    x, y = T._all_of(auto), T._all_of(new)
    for k in x:
        if k != "state":
            assert torch.equal(_bits(x[k]), _bits(y[k])), f"{name}: update 4 against a new learner's first: {k}"
    assert torch.equal(auto.scalars[:2], new.scalars[:2]) and auto.state[1].item() == 4 and new.state[1].item() == 1 and auto.state[7].item() == 3
    handle_equals(auto, f"{name}: handle, update 4")
    nat.close()


@pytest.mark.parametrize("name", NAMES)
def test_freq_zero_is_the_learner_without_the_argument(hip, name, monkeypatch):
    T = _tt()
    cs = T._gc()._Case(hip, name)
    calls = []
    real = type(hip).net_reset
    monkeypatch.setattr(type(hip), "net_reset", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    off, none = _engine(cs, net_reset_freq=0, net_reset_shrink=0.5), T._engine(cs, FAR)
    nat = T._handle(cs, none, FAR)
    nat.set_net_reset(0, 0.5, SEED)
    assert off.net_reset_freq == 0 and off.reset_segs is None and none.reset_segs is None and none.net_reset_freq == 0
    # every library call an update makes, by entry point: what a captured hipGraph of the update would hold as nodes
    from collections import Counter

    class Counting:
        def __init__(self, lib):
            self._lib, self.seen = lib, Counter()

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("a0_"):
                return fn

            def call(*a, **k):
                self.seen[name] += 1
                return fn(*a, **k)
            return call

    counting = Counting(hip.lib)
    monkeypatch.setattr(hip, "lib", counting)
    seen = {}
    for s in range(4):
        for tag, dev in (("off", off), ("none", none)):
            counting.seen = Counter()
            dev.update(*cs.batch(s), rand=cs.draws(dev))
            seen[tag] = counting.seen
        assert seen["off"] == seen["none"] and sum(seen["off"].values()) > 5 and "a0_net_reset" not in seen["off"], f"update {s + 1}: {seen}"
        nat.update(*cs.batch(s))
    torch.cuda.synchronize()
    assert not calls, "no launch"
    # collectable garbage of earlier tests (frames kept alive by caught exceptions hold whole learners) must not be freed in the middle of a measurement
    import gc
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = _engine(cs, net_reset_freq=0, net_reset_shrink=0.5)
    used_off = torch.cuda.memory_allocated() - mem
    del more
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = T._engine(cs, FAR)
    assert torch.cuda.memory_allocated() - mem == used_off, "no extra allocation"
    del more
    T._same(T._all_of(off), T._all_of(none), name)
    o, t, m, v, st = nat.get()
    T._same(dict(online=o, target=t, moment1=m, moment2=v, state=st), {k: T._all_of(none)[k] for k in ("online", "target", "moment1", "moment2", "state")}, f"{name}: handle")
    assert off.state[7].item() == 0 and off.state[1].item() == 4
    nat.close()


def test_a_separately_staged_target_pass_is_refused(hip):
    T = _tt()
    cs = T._gc()._Case(hip, "dqn")
    dev = _engine(cs, net_reset_freq=3)
    with pytest.raises(ValueError, match="tstage"):
        dev.update(*cs.batch(0), tstage=0)
    with pytest.raises(ValueError, match=r"learner\.net_reset_shrink"):
        _engine(cs, net_reset_freq=3, net_reset_shrink=1.5)
    with pytest.raises(ValueError, match=r"learner\.net_reset_freq"):
        _engine(cs, net_reset_freq=-3)


# ------------------------------------------------------------------------------------------------ 8. the Trainer
def _el():
    import test_gpu_eps_ladder as EL
    return EL


def _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, freq=4, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    on = [f"learner.net_reset_freq={freq}", "learner.net_reset_shrink=0.5"] if freq else []
    cfg = parse_overrides([f"learner.algo={algo}", f"seed={seed}", f"logdir={tmp_path / tag}"] + on + _el().BASE5 + list(extra))
    return Trainer(cfg, use_lp=use_lp)


def _state(tr):
    eng = tr.learner.engine
    return _el()._state(tr) + [eng.online.wt.clone(), eng.target.wt.clone()]


def _run(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, freq=4, iters=6, dp=False):
    from agent0_amd.deepq.native_loop import NativeLoop
    EL = _el()
    tr = _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, freq)
    hook = EL._install_exchange(tr) if dp else None
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    out = _state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count
    assert res[-1]["loss"] is not None, "updates ran"
    EL._close_exchange(tr, hook) if dp else EL._close(tr)
    return out


@pytest.mark.parametrize("mode,algo,extra,freq", [("main", "dqn", [], 4), ("main", "dqn", [], 3), ("launch", "dqn", [], 4), ("dp", "dqn", [], 4),
                                                  ("main", "c51", ["learner.noisy_net=true", "learner.dueling_head=true", "learner.n_step_q=3"], 4)],
                         ids=["main-dqn", "main-dqn-period3", "launch-dqn", "dp-dqn", "main-c51-noisy-duel-n3"])
def test_handles_and_python_classes_end_on_the_same_state(mode, algo, extra, freq, tmp_path, monkeypatch):
    """Six iterations of three updates once training has started.  Period 4: the resets fall on the first, the second and the last update of an iteration; period 3:
    always on the last.  The Python classes run their first updates eagerly and the rest from a hipGraph.  ``dp``: a one-rank RCCL group (A0_DP_FORCE=1)."""
    import torch.distributed as dist
    EL = _el()
    dp = mode == "dp"
    if dp:
        EL._one_rank_group(monkeypatch)
    try:
        a = _run(tmp_path, monkeypatch, False, algo, extra, mode == "launch", "py", freq, dp=dp)
        b = _run(tmp_path, monkeypatch, True, algo, extra, mode == "launch", "nat", freq, dp=dp)
    finally:
        if dp:
            dist.destroy_process_group()
    EL._assert_same_run(a, b)
    state = a[0][4]
    steps = state[1].item()
    assert steps >= 2 * freq and state[7].item() == steps // freq * freq and a[1][-1]["net_resets"] == steps // freq
    if mode == "main" and algo == "dqn" and freq == 4:
        plain = _run(tmp_path, monkeypatch, True, algo, extra, False, "plain", 0)
        assert plain[0][4][1].item() == steps and plain[0][4][7].item() == 0 and not torch.equal(plain[0][0], a[0][0]), "the setting changes the network"
        assert "net_resets" not in plain[1][-1]


@pytest.mark.parametrize("save_native,load_native", [(True, True), (False, False), (True, False), (False, True)], ids=["handles", "python-classes", "handles-to-python", "python-to-handles"])
def test_a_snapshot_between_two_resets_resumes_across_the_next(save_native, load_native, tmp_path, monkeypatch):
    EL = _el()
    want = _run(tmp_path, monkeypatch, load_native, "dqn", [], False, "a")
    tr = _trainer(tmp_path, monkeypatch, save_native, "dqn", [], False, "b")
    for _ in range(3):
        tr.run_iteration()
    at = tr.learner.engine.state[1].item()
    assert at % 4 != 0, "between two resets"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    EL._close(tr)
    tr = _trainer(tmp_path, monkeypatch, load_native, "dqn", [], False, "c", seed=7)
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(3)]
    got = _state(tr)
    EL._close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][3:]
    assert got[4][7].item() > at, "a reset happened after the snapshot"


def test_the_statistic_and_the_setting_off(tmp_path, monkeypatch):
    GC = _tt()._gc()
    tr = GC._trainer(tmp_path, monkeypatch, True, "off")
    eng = tr.learner.engine
    assert eng.net_reset_freq == 0 and eng.reset_segs is None
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    assert list(res.keys()) == GC.TODAYS_HEADER[:-1] + ["fps"] and res["loss"] is not None
    GC._close(tr)
    with open(tmp_path / "off" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == GC.TODAYS_HEADER and len(rows) == 3
    assert "net_reset" not in open(tmp_path / "off" / "msg.log").read()
    tr = GC._trainer(tmp_path, monkeypatch, True, "on", extra=["learner.net_reset_freq=2", "learner.net_reset_shrink=0.5"])
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    steps = tr.learner.engine.state[1].item()
    assert list(res.keys()) == GC.TODAYS_HEADER[:-1] + ["net_resets", "fps"] and steps >= 2 and res["net_resets"] == steps // 2
    GC._close(tr)
    with open(tmp_path / "on" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == GC.TODAYS_HEADER + ["net_resets"] and rows[-1][-1] == str(steps // 2)
    assert f"net_resets: {steps // 2}" in open(tmp_path / "on" / "msg.log").read()
