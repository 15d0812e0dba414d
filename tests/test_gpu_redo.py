"""GPU (MI355X): the dormant-neuron statistic and ReDo recycling (``learner.redo_freq`` / ``learner.redo_tau`` / ``learner.redo_recycle``): a0_redo_score,
a0_redo_recycle and everything that issues them, against the numpy restatement tests/redo_ref.py.

1. the scoring kernels on synthetic buffers against float64: scores within one fp32 ulp of the rounded float64 value (double summation in any order is off by at
   most rows * 2^-53 relative, far below the rounding to fp32), mask and counts exact — after the reference side has shown that no score lies within 1e-6
   relative of tau.
2. the recycle kernel alone with a hand-made mask, byte for byte: fresh values from a0_rng_normal fills of Philox stream 9 at k * n_total + e; untouched bytes,
   zero moments exactly where touched, the weight copy == a0_net_conv_wt_refresh of the result; the self-deciding gate of both entry points.
3. DeviceLearner and the a0_learner handle beside a twin without the setting.   4. the Trainer on both loops, a snapshot across a recycle, every setting at once.

Work split of the kernels (csrc/net_reset.hip): scoring — a lane owns four channels of every (1024 / n)-th row of its workgroup's rows, four rows in flight; a
layer engages one workgroup per eight workgroup steps (32 / 16 / 2 rows each) of its rows, at most 512, and the finish adds that many partials in eight slices.
So the row counts below cover one row (one workgroup, one slice), counts below and off a step, 130 rows of 512 (9 workgroups: slices of 2, the last ones
empty), 567 rows of 64 (5 workgroups) and 2000 rows of 32 (8 workgroups, one per slice); the learner tests add 3200 / 648 / 392 / 128 rows.  Recycling — element
by element over [0, n_adam), 4-byte aligned."""
import math

import numpy as np
import pytest
import torch

import net_reset_ref as R
import recipe
import redo_ref as RD

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SEED = 0x9E3779B1
WIDTHS = (32, 64, 64, 512)
LO = (0, 32, 96, 160)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "redo_score") and hasattr(ops, "redo_recycle")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _outputs(hip):
    return (hip.zeros(hip.REDO_PARTIALS * hip.REDO_NEURONS, dtype=torch.float64), torch.full((672,), SENTINEL, device=hip.device),
            torch.full((672,), -5, dtype=torch.int32, device=hip.device), torch.full((8,), -1, dtype=torch.int32, device=hip.device))


# ------------------------------------------------------------------------------------------------ 1. scoring
ROWS = [(1, 1, 1, 1), (3, 7 * 81, 1, 2), (5 * 20 * 20, 1, 7 * 81, 130), (3, 7 * 81, 7 * 81, 130), (5 * 20 * 20, 7 * 81, 7 * 81, 1)]
_ACTS = {}


def _acts(rows, zero_layer):
    """Four fp32 arrays, cached and never modified: magnitudes 0.5 + |N(0, 1)| with random signs (the scores then lie in about [0.3, 3], far from every tau);
    planted: two channels that are exactly zero, one channel at 1e-3 of the layer's mean, and with ``zero_layer`` one layer that is zero altogether."""
    key = (rows, zero_layer)
    if key not in _ACTS:
        g = recipe.gen(900 + sum(rows) + 7 * (zero_layer + 1))
        acts = []
        for l, (r, n) in enumerate(zip(rows, WIDTHS)):
            x = (0.5 + np.abs(g.standard_normal((r, n)))) * np.where(g.random((r, n)) < 0.5, -1.0, 1.0)
            x[:, 1] = 0.0
            x[:, n - 1] = 0.0
            x[:, 5] = 1e-3 * np.abs(x).mean() * np.where(np.arange(r) % 2, -1.0, 1.0)
            if l == zero_layer:
                x[:] = 0.0
            acts.append(x.astype(np.float32))
        _ACTS[key] = acts
    return _ACTS[key]


@pytest.mark.parametrize("tau", [0.0, 0.025, 0.1])
@pytest.mark.parametrize("zero_layer", [-1, 0, 3], ids=["", "conv1-silent", "fc1-silent"])
@pytest.mark.parametrize("rows", ROWS, ids=lambda r: "rows%d-%d-%d-%d" % r)
def test_scores_mask_and_counts_against_float64(hip, rows, zero_layer, tau):
    acts = _acts(rows, zero_layer)
    want, mask, counts = RD.evaluate(acts, tau)
    assert RD.margin(want, tau) > 1e-6, "the inputs keep every score away from tau"
    for l, (lo, n) in enumerate(zip(LO, WIDTHS)):
        if l == zero_layer:
            assert not want[lo:lo + n].any() and counts[l] == n
        else:
            assert want[lo + 1] == 0.0 and want[lo + n - 1] == 0.0 and 0 < want[lo + 5] < 2e-3 and counts[l] == (2 if tau == 0.0 else 3)
    dev = [torch.from_numpy(a).to(hip.device).reshape(-1) for a in acts]
    partials, scores, mk, ct = _outputs(hip)
    state = torch.tensor([0, 12, 0, 0, 0, 0, 12, 0], dtype=torch.int32, device=hip.device)
    hip.redo_score(*dev, tau, state, 4, False, partials, scores, mk, ct)
    torch.cuda.synchronize()
    got = scores.cpu().numpy()
    ref32 = want.astype(np.float32)
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30))).astype(np.float64)
    print(f"rows={rows} zero_layer={zero_layer} tau={tau}: max error {err.max():.3f} ulp, counts {ct.tolist()}")
    assert err.max() <= 1.0
    assert np.array_equal(mk.cpu().numpy(), mask) and ct.tolist() == counts + [12, -1, -1], "mask, counts, the evaluation's update count; the spare words are not written"
    # reproducible: a second run gives the same bytes
    p2, s2, m2, c2 = _outputs(hip)
    hip.redo_score(*dev, tau, None, 0, True, p2, s2, m2, c2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s2), _bits(scores)) and torch.equal(m2, mk) and c2.tolist() == counts + [0, -1, -1] and torch.equal(p2, partials)


@pytest.mark.parametrize("state,freq", [([0, 4, 0, 0, 0, 0, 4, 0], 3), ([0, 3, 1, 1, 0, 0, 3, 0], 3), ([0, 0, 0, 0, 0, 0, 0, 0], 3), ([0, 3, 0, 0, 0, 0, 3, 0], 0)],
                         ids=["freq-mismatch", "nan-skipped", "no-update-yet", "freq-zero"])
def test_the_scoring_launches_decide_for_themselves(hip, state, freq):
    dev = [torch.from_numpy(a).to(hip.device).reshape(-1) for a in _acts(ROWS[1], -1)]
    partials, scores, mk, ct = _outputs(hip)
    partials.fill_(3.0)
    st = torch.tensor(state, dtype=torch.int32, device=hip.device)
    hip.redo_score(*dev, 0.1, st, freq, False, partials, scores, mk, ct)
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all()) and bool((mk == -5).all()) and ct.tolist() == [-1] * 8 and bool((partials == 3.0).all()) and st.tolist() == state


# ------------------------------------------------------------------------------------------------ 2. recycling
def _guarded(hip, a, off):
    buf = torch.full((a.size + 12,), SENTINEL, device=hip.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[4 + off:4 + off + a.size]
    v.copy_(torch.from_numpy(a))
    return buf, v


def _guards_intact(buf, off, n):
    return bool((buf[:4 + off] == SENTINEL).all()) and bool((buf[4 + off + n:] == SENTINEL).all())


class _World:
    """A flat buffer [pad0 | conv1 | pad1 | conv2 | pad2 | conv3 | pad3 | fc1 | pad4 | head | extra | tail]: feat = 128, a head of 5 real and 27 padded rows, an
    ``extra`` block inside the Adam range that a recycle must leave alone (the cosine embedding's place) and a tail behind it (the fraction net's); pads and tail
    have no rule.  Moments, the online weight copy, and the rule table with the encoder's keep flags set (a recycle ignores them)."""
    FEAT, NPAD, REAL = 128, 32, 5

    def __init__(self, hip, C_, pads, off, tail):
        g = recipe.gen(77 + C_ + sum(pads) + off)
        K1 = 64 * C_
        shapes = [(32, K1), (64, 512), (64, 576), (512, self.FEAT), (self.NPAD, 512)]
        names = ("conv1", "conv2", "conv3", "fc1", "head")
        at, self.blocks, self.segs = 0, {}, []
        for name, (N, K), pad in zip(names, shapes, pads):
            at += pad
            self.blocks[name] = (at, N, K)
            if name == "head":
                self.segs += [(at, self.REAL * K, R.NORMAL, 0.01, 0), (at + self.REAL * K, (N - self.REAL) * K, R.CONST, 0.0, 0), (at + N * K, N, R.CONST, 0.0, 0)]
            else:
                self.segs += [(at, N * K, R.NORMAL, 0.02 + 0.01 * len(self.segs), int(name != "fc1")), (at + N * K, N, R.CONST, 0.0, int(name != "fc1"))]
            at += N * K + N
        self.segs.append((at, 200, R.NORMAL, 0.5, 0))
        self.n_adam = at + 203
        self.n = self.n_adam + tail
        self.hip, self.C, self.off = hip, C_, off
        f = lambda s: (g.standard_normal(self.n) * s).astype(np.float32)
        self.p0, self.m0, self.v0 = f(0.05), f(1e-3), np.abs(f(1e-3)) + np.float32(1e-9)
        self.pb, self.p = _guarded(hip, self.p0, off)
        self.mb, self.m = _guarded(hip, self.m0, off)
        self.vb, self.v = _guarded(hip, self.v0, off)
        self.wt = hip.empty(hip.conv_wt_floats(C_))
        hip.conv_wt_refresh(self.weights(self.p), C_, self.wt)
        torch.cuda.synchronize()
        self.wt0 = self.wt.clone()

    def weights(self, flat):
        out = {}
        for i, name in enumerate(("conv1", "conv2", "conv3"), 1):
            o, N, K = self.blocks[name]
            out[f"w{i}"], out[f"b{i}"] = flat[o:o + N * K], flat[o + N * K:o + N * K + N]
        return out

    def layout_blocks(self):
        return tuple(self.blocks[n][0] for n in ("conv1", "conv2", "conv3", "fc1", "head")) + (64 * self.C, self.FEAT, self.NPAD)

    def recycle(self, mask, state, freq, force, k, seed=SEED, wt=True):
        mk = torch.from_numpy(np.asarray(mask, np.int32)).to(self.hip.device)
        self.hip.redo_recycle(self.p, self.m, self.v, self.n_adam, self.n, self.segs, self.layout_blocks(), mk, seed, state, freq, force, k,
                              *((self.weights(self.p), self.C, self.wt) if wt else ()))
        torch.cuda.synchronize()

    def phi(self, seed, k):
        """The fresh values of the normal segments, from fills of stream 9 at the stated positions."""
        phi = np.zeros(self.n, np.float32)
        for off, cnt, kind, scale, keep in self.segs:
            if kind == R.NORMAL:
                out = self.hip.empty(cnt)
                self.hip.rng_normal(seed & 0xFFFFFFFF, RD.STREAM_REDO, k * self.n + off, scale, out, cnt)
                phi[off:off + cnt] = out.cpu().numpy()
        return phi

    def check(self, mask, k, what, seed=SEED, wt=True):
        want_p, want_m, want_v, both = RD.expect(self.p0, self.m0, self.v0, self.blocks, self.segs, mask, self.phi(seed, k))
        for name, got, want in (("params", self.p, want_p), ("exp_avg", self.m, want_m), ("exp_avg_sq", self.v, want_v)):
            bad = np.nonzero(got.cpu().numpy().view(np.int32) != want.view(np.int32))[0]
            print(f"{what} {name}: {bad.size} of {want.size} elements differ from the restatement, first {bad[:8].tolist()}; {both.size} touched")
            assert not bad.size
        for buf in (self.pb, self.mb, self.vb):
            assert _guards_intact(buf, self.off, self.n)
        if wt:
            fresh = torch.full_like(self.wt, float("nan"))
            self.hip.conv_wt_refresh(self.weights(self.p), self.C, fresh)
            torch.cuda.synchronize()
            assert torch.equal(_bits(fresh), _bits(self.wt)), f"{what}: the weight copy is a refresh of the new parameters"
        else:
            assert torch.equal(_bits(self.wt), _bits(self.wt0))
        return both


def _mask(kind):
    m = np.zeros(672, np.int32)
    if kind == "one-per-layer":
        m[[7, 32 + 63, 96 + 0, 160 + 300]] = 1
    elif kind == "all-of-conv2":
        m[32:96] = 1
    elif kind == "all-of-fc1":
        m[160:] = 1
    elif kind == "first-and-last":
        m[[0, 31, 32, 95, 96, 159, 160, 671]] = 1
    elif kind == "everything":
        m[:] = 1
    else:
        assert kind == "none"
    return m


@pytest.mark.parametrize("kind", ["none", "one-per-layer", "all-of-conv2", "all-of-fc1", "first-and-last", "everything"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("C_,pads,tail", [(4, (0, 0, 0, 0, 0), 0), (4, (1, 0, 2, 0, 3), 37), (1, (0, 0, 0, 0, 0), 38), (1, (4, 3, 0, 1, 0), 2)],
                         ids=["C4", "C4-pads-tail37", "C1-tail38", "C1-pads-tail2"])
def test_recycle_against_the_restatement(hip, C_, pads, tail, off, kind):
    """Convolution blocks on and off multiples of four floats, 16-byte aligned buffers and buffers 4 bytes behind, n_total % 4 of 1, 2 and 0; a head with 27 padded
    rows whose column is zeroed in all 32."""
    w = _World(hip, C_, pads, off, tail)
    mask = _mask(kind)
    w.recycle(mask, None, 0, True, 3)
    both = w.check(mask, 3, f"C={C_} pads={pads} tail={tail} off={off} {kind}")
    assert (both.size == 0) == (kind == "none") and (w.n % 4 != 0 or tail == 0)
    if kind == "none":
        assert torch.equal(_bits(w.wt), _bits(w.wt0))
    if kind == "all-of-fc1":
        assert torch.equal(_bits(w.wt), _bits(w.wt0)), "no convolution weight moved"
        ho, hN, hK = w.blocks["head"]
        assert not w.p[ho:ho + hN * hK].any() and torch.equal(w.p[ho + hN * hK:], torch.from_numpy(w.p0[ho + hN * hK:]).to(hip.device)), "all head weights 0, biases and the rest kept"


def test_recycle_without_weight_copies_and_the_draws(hip):
    """No ``wt``: the parameters alone.  A value is a function of (seed, k, e): another k or another seed gives other values at the same places, the same pair the
    same bytes; 32 bits of the seed count."""
    mask = _mask("first-and-last")
    a = _World(hip, 4, (0, 0, 0, 0, 0), 0, 37)
    a.recycle(mask, None, 0, True, 3, wt=False)
    a.check(mask, 3, "no wt", wt=False)
    res = {}
    for tag, seed, k in (("same", SEED | (5 << 32), 3), ("k", SEED, 4), ("seed", SEED + 1, 3)):
        b = _World(hip, 4, (0, 0, 0, 0, 0), 0, 37)
        b.recycle(mask, None, 0, True, k, seed=seed, wt=False)
        res[tag] = b.p.clone()
    inc, out = RD.touched(a.blocks, mask)
    drawn = torch.from_numpy(np.setdiff1d(inc, out)[:512]).to(hip.device)          # conv1 row 0: normal draws
    assert torch.equal(_bits(res["same"]), _bits(a.p))
    for tag in ("k", "seed"):
        assert not (res[tag][drawn] == a.p[drawn]).any(), tag


@pytest.mark.parametrize("state,freq,fires", [([0, 4, 0, 0, 0, 0, 4, 0], 3, False), ([0, 3, 1, 1, 0, 0, 3, 0], 3, False), ([0, 0, 0, 0, 0, 0, 0, 0], 3, False),
                                              ([0, 6, 0, 0, 0, 0, 6, 0], 3, True)], ids=["freq-mismatch", "nan-skipped", "no-update-yet", "second-recycle"])
def test_the_recycle_launch_decides_for_itself(hip, state, freq, fires):
    w = _World(hip, 4, (1, 0, 2, 0, 3), 1, 37)
    st = torch.tensor(state, dtype=torch.int32, device=hip.device)
    mask = _mask("one-per-layer")
    w.recycle(mask, st, freq, False, 99)
    assert st.tolist() == state, "the status words are only read: Adam's bias correction is not restarted"
    if fires:
        w.check(mask, 2, "k = state[1] / freq")
    else:
        w.check(_mask("none"), 0, "nothing written")
        assert torch.equal(_bits(w.wt), _bits(w.wt0))


# ------------------------------------------------------------------------------------------------ 3. learners
B = 8
FAR = 10 ** 6
LEARNERS = {"dqn": dict(algo="dqn", A=4), "c51-duel": dict(algo="c51", A=4, dueling=True, double_q=True), "iqn": dict(algo="iqn", A=4, KNN=(8, 16, 24)),
            "fqf-fraction-clip": dict(algo="fqf", A=4, max_grad_norm=0.05)}
FORCED = {"conv1": [3], "conv2": [63], "conv3": [0], "fc1": [0, 5, 511]}      # biases set to -1000 in front of update 3: those neurons are exactly silent


def _tt():
    import test_gpu_target_tau as T
    return T


def _case(hip, name):
    """test_gpu_grad_clip's case at the small geometry of the learner tests, for this file's learner table (c51 without NoisyNet: recycling is refused with it)."""
    from agent0_amd.deepq.layout import NetLayout
    GC = _tt()._gc()
    c = LEARNERS[name]
    cs = GC._Case.__new__(GC._Case)
    cs.hip, cs.c = hip, c
    cs.spec = recipe.NetSpec(c["algo"], c["A"], dueling=c.get("dueling", False), noisy=False)
    cs.L = NetLayout.from_spec(cs.spec)
    cs.K, cs.N, cs.Nd = c.get("KNN", (32, 64, 64))
    cs.cap = 64
    cs.ring = torch.from_numpy(recipe.make_frames(cs.cap, 5, cs.spec.obs_shape)).to(hip.device).reshape(-1).contiguous()
    return cs


def _engine(cs, **kw):
    from agent0_amd.common.utils import DeviceRng
    T = _tt()
    return T._engine(cs, FAR, aug_rng=DeviceRng(cs.hip, T._gc().SEED), **kw)


def _silence(L, flat):
    for name, idx in FORCED.items():
        b = L.blocks[name]
        for i in idx:
            flat[b.offset + b.N * b.K + i] = -1000.0


def _acts_of(dev):
    L, ws = dev.L, dev.ws_o
    rows = (B * L.H1 * L.W1, B * L.H2 * L.W2, B * L.H3 * L.W3)
    return [ws.act1[:rows[0] * 32].cpu().numpy().reshape(-1, 32), ws.act2[:rows[1] * 64].cpu().numpy().reshape(-1, 64), ws.act3[:rows[2] * 64].cpu().numpy().reshape(-1, 64),
            ws.h.cpu().numpy().reshape(-1, 512)]


def _phi(hip, L, seed, k):
    n = L.n_params_padded
    phi = np.zeros(n, np.float32)
    for off, cnt, kind, scale, keep in L.reset_segments():
        if kind == R.NORMAL:
            out = hip.empty(cnt)
            hip.rng_normal(seed & 0xFFFFFFFF, RD.STREAM_REDO, k * n + off, scale, out, cnt)
            phi[off:off + cnt] = out.cpu().numpy()
    return phi


@pytest.mark.parametrize("name", list(LEARNERS))
def test_learner_recycles_at_the_right_update_and_nothing_else_moves(hip, name):
    """redo_freq = 3 beside a twin without the setting, a learner that only measures, and the a0_learner handle: equal bytes through update 2; after update 3 the
    learner is the restatement's recycle of the twin, by the mask the restatement derives from the peeked activations."""
    T = _tt()
    cs = _case(hip, name)
    L, tau = cs.L, 0.1
    auto, twin, meas = _engine(cs, redo_freq=3, redo_tau=tau), _engine(cs), _engine(cs, redo_freq=3, redo_tau=tau, redo_recycle=False)
    nat = T._handle(cs, auto, FAR)
    nat.set_redo(3, tau, True, auto.reset_seed())
    assert twin.redo_counts is None and twin.redo_freq == 0 and auto.redo_counts.tolist()[5] == -1 and meas.redo_segs is None
    assert nat.redo_buffers()[2].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]

    def handle_equals(dev, what):
        o, t, m, v, st = nat.get()
        T._same(dict(online=o, target=t, moment1=m, moment2=v, state=st), {k: T._all_of(dev)[k] for k in ("online", "target", "moment1", "moment2", "state")}, what)

    for s in range(2):
        for dev in (auto, twin, meas):
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        nat.update(*cs.batch(s))
        torch.cuda.synchronize()
        T._same(T._all_of(auto), T._all_of(twin), f"{name}: update {s + 1}")
        T._same(T._all_of(meas), T._all_of(twin), f"{name}: measuring, update {s + 1}")
        handle_equals(auto, f"{name}: handle, update {s + 1}")
        assert auto.redo_counts.tolist()[5] == -1, "no evaluation yet"
    for dev in (auto, twin, meas):
        _silence(L, dev.online.flat)
    nat.set_params(auto.online.flat, auto.target.flat)
    for dev in (auto, twin, meas):
        dev.update(*cs.batch(2), rand=cs.draws(dev))
    nat.update(*cs.batch(2))
    torch.cuda.synchronize()
    # ---- the evaluation: the restatement on the activations the update left
    acts = _acts_of(auto)
    for x, y in zip(acts, _acts_of(twin)):
        assert np.array_equal(x, y)
    assert acts[3].shape[0] == (B * (cs.N if L.algo == "iqn" else L.F) if L.quantile else B), "iqn / fqf: the B * N rows of the differentiated pass"
    want, mask, counts = RD.evaluate(acts, tau)
    assert RD.margin(want, tau) > 1e-6
    for (lname, lo, n), c in zip(RD.LAYERS, counts):
        assert all(mask[lo + i] for i in FORCED[lname]) and len(FORCED[lname]) <= c < n, f"{lname}: the silenced neurons are dormant, the layer is not"
    got = auto.redo_scores.cpu().numpy()
    ref32 = want.astype(np.float32)
    assert (np.abs(got.astype(np.float64) - ref32) <= np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30)))).all()
    assert np.array_equal(auto.redo_mask.cpu().numpy(), mask) and auto.redo_counts.tolist() == counts + [3, 0, 0]
    print(f"{name}: dormant per layer {counts}")
    # ---- the recycle: the twin's buffers through the restatement
    blocks, segs = RD.blocks_of(L), L.reset_segments()
    p, m, v, both = RD.expect(twin.online.flat.cpu().numpy(), twin.adam_m.cpu().numpy(), twin.adam_v.cpu().numpy(), blocks, segs, mask, _phi(hip, L, auto.reset_seed(), 1))
    for what, got_t, want_a in (("online", auto.online.flat, p), ("moment1", auto.adam_m, m), ("moment2", auto.adam_v, v)):
        bad = np.nonzero(got_t.cpu().numpy().view(np.int32) != want_a.view(np.int32))[0]
        print(f"{name} {what}: {bad.size} elements differ from the restatement, first {bad[:8].tolist()}; {both.size} touched")
        assert not bad.size
    assert both.size and not np.array_equal(p, twin.online.flat.cpu().numpy())
    x, y = T._all_of(auto), T._all_of(twin)
    for k in ("target", "wt_target", "state"):
        assert torch.equal(_bits(x[k]), _bits(y[k])), f"{name}: {k} is untouched (state[7] included)"
    fresh = hip.empty(auto.online.wt.numel())
    hip.conv_wt_refresh(auto.online.encoder_weights(), L.C, fresh)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fresh), _bits(auto.online.wt)) and not torch.equal(_bits(auto.online.wt), _bits(twin.online.wt))
    if "frac" in L.blocks:
        assert torch.equal(auto.rms_sq, twin.rms_sq)
    # ---- the handle: the same bytes, the same evaluation
    handle_equals(auto, f"{name}: handle, update 3")
    sc, mk, ct = nat.redo_buffers()
    assert torch.equal(_bits(sc), _bits(auto.redo_scores)) and torch.equal(mk, auto.redo_mask) and torch.equal(ct, auto.redo_counts)
    # ---- measuring only: the twin's parameters, the same evaluation
    T._same(T._all_of(meas), T._all_of(twin), f"{name}: measuring, update 3")
    assert torch.equal(_bits(meas.redo_scores), _bits(auto.redo_scores)) and torch.equal(meas.redo_mask, auto.redo_mask) and torch.equal(meas.redo_counts, auto.redo_counts)
    # ---- update 4: no evaluation; learner and handle go on together
    auto.update(*cs.batch(3), rand=cs.draws(auto))
    nat.update(*cs.batch(3))
    torch.cuda.synchronize()
    handle_equals(auto, f"{name}: handle, update 4")
    assert auto.redo_counts.tolist() == counts + [3, 0, 0] and auto.state.tolist()[1] == 4 and auto.state.tolist()[7] == 0
    nat.close()


def test_noisy_net_measures_and_refuses_to_recycle(hip):
    T = _tt()
    cs = T._gc()._Case(hip, "rainbow-lite")
    with pytest.raises(ValueError, match=r"learner\.redo_freq.*learner\.noisy_net"):
        _engine(cs, redo_freq=3)
    meas, twin = _engine(cs, redo_freq=2, redo_recycle=False), _engine(cs)
    nat = T._handle(cs, meas, FAR)
    with pytest.raises(Exception, match="NoisyNet"):
        nat.set_redo(2, 0.1, True, 1)
    with pytest.raises(Exception, match="tau = 1"):
        nat.set_redo(2, 1.0, False, 1)
    nat.set_redo(2, 0.1, False, 0)
    for s in range(2):
        for dev in (meas, twin):
            dev.update(*cs.batch(s), rand=cs.draws(dev))
        nat.update(*cs.batch(s))
    torch.cuda.synchronize()
    T._same(T._all_of(meas), T._all_of(twin), "measuring changes no parameter")
    want, mask, counts = RD.evaluate(_acts_of(meas), 0.1)
    assert RD.margin(want, 0.1) > 1e-6 and meas.redo_counts.tolist() == counts + [2, 0, 0]
    assert torch.equal(nat.redo_buffers()[2], meas.redo_counts) and torch.equal(nat.redo_buffers()[1], meas.redo_mask)
    with pytest.raises(Exception, match="first update|has run an update"):
        nat.set_redo(3, 0.1, False, 0)
    nat.close()


def test_freq_zero_is_the_learner_without_the_argument(hip, monkeypatch):
    T = _tt()
    cs = _case(hip, "dqn")
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

    off, none = _engine(cs, redo_freq=0, redo_tau=0.5, redo_recycle=True), T._engine(cs, FAR)
    nat = T._handle(cs, none, FAR)
    nat.set_redo(0, 0.5, True, SEED)
    assert nat.redo_buffers() is None and off.redo_partials is None and off.redo_counts is None and off.redo_segs is None
    counting = Counting(hip.lib)
    monkeypatch.setattr(hip, "lib", counting)
    seen = {}
    for s in range(3):
        for tag, dev in (("off", off), ("none", none)):
            counting.seen = Counter()
            dev.update(*cs.batch(s), rand=cs.draws(dev))
            seen[tag] = counting.seen
        assert seen["off"] == seen["none"] and sum(seen["off"].values()) > 5 and not any("redo" in k for k in seen["off"]), f"update {s + 1}: {seen}"
        nat.update(*cs.batch(s))
    torch.cuda.synchronize()
    T._same(T._all_of(off), T._all_of(none), "off")
    o, t, m, v, st = nat.get()
    T._same(dict(online=o, target=t, moment1=m, moment2=v, state=st), {k: T._all_of(none)[k] for k in ("online", "target", "moment1", "moment2", "state")}, "off: handle")
    import gc
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = _engine(cs, redo_freq=0)
    used_off = torch.cuda.memory_allocated() - mem
    del more
    gc.collect()
    mem = torch.cuda.memory_allocated()
    more = T._engine(cs, FAR)
    assert torch.cuda.memory_allocated() - mem == used_off, "no extra allocation"
    nat.close()


# ------------------------------------------------------------------------------------------------ 4. the Trainer
TAU_LOOP = 0.5                      # high enough that a young network has dormant neurons: the runs below really recycle
REDO_KEYS = ["dormant_frac", "dormant_frac_conv1", "dormant_frac_conv2", "dormant_frac_conv3", "dormant_frac_fc1"]
ON = ["learner.redo_freq=3", f"learner.redo_tau={TAU_LOOP}"]


def _nr():
    import test_gpu_net_reset as NR
    return NR


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for k in x:
            assert x[k] == y[k] or (isinstance(x[k], float) and isinstance(y[k], float) and math.isnan(x[k]) and math.isnan(y[k])), (k, x[k], y[k])


def _assert_same_run(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    _same_results(a[1], b[1])
    assert a[2:] == b[2:]


def _handle_acts(tr):
    """The activations the handle's last update left (A0_PEEK_ACT1 / 2 / 3 / FC1), as the restatement takes them."""
    import ctypes as C
    nl = tr._nl
    out = []
    for what, n in ((1, 32), (2, 64), (3, 64), (4, 512)):
        ptr, cnt = C.c_void_p(), C.c_longlong()
        assert nl.lib.a0_learner_peek(nl.learner, what, C.addressof(ptr), C.addressof(cnt)) == 0
        view = type("_Peek", (), {"__cuda_array_interface__": {"shape": (int(cnt.value),), "typestr": "<f4", "data": (int(ptr.value), False), "version": 3}})()
        out.append(torch.as_tensor(view, device="cuda").cpu().numpy().reshape(-1, n))
    return out


@pytest.mark.parametrize("native", [False, True], ids=["python-classes", "handles"])
def test_the_statistic_is_the_restatements(native, tmp_path, monkeypatch):
    """redo_freq = 3 = learner_steps: every evaluation falls on an iteration's last update, whose activations are still there when the iteration returns.  Measuring
    only, so that the columns are what the test is about; the result, progress.csv and msg.log carry them."""
    import csv
    NR = _nr()
    tr = NR._trainer(tmp_path, monkeypatch, native, "dqn", ON + ["learner.redo_recycle=false"], False, "run", freq=0)
    seen = 0
    for i in range(4):
        res = tr.run_iteration()
        tr.logging(res)
        assert list(res)[-6:] == REDO_KEYS + ["fps"]
        eng = tr.learner.engine
        steps = eng.state[1].item()
        if steps == 0:
            assert all(math.isnan(res[k]) for k in REDO_KEYS), "NaN until the first evaluation"
            continue
        assert steps % 3 == 0
        torch.cuda.synchronize()
        dev_b = eng.B
        acts = _handle_acts(tr) if native else [a[:r * n].reshape(-1, n) for a, r, n in zip(
            [eng.ws_o.act1.cpu().numpy(), eng.ws_o.act2.cpu().numpy(), eng.ws_o.act3.cpu().numpy(), eng.ws_o.h.cpu().numpy()],
            (dev_b * eng.L.H1 * eng.L.W1, dev_b * eng.L.H2 * eng.L.W2, dev_b * eng.L.H3 * eng.L.W3, dev_b), WIDTHS)]
        want, mask, counts = RD.evaluate(acts, TAU_LOOP)
        assert RD.margin(want, TAU_LOOP) > 1e-6
        assert [res[k] for k in REDO_KEYS] == [counts[4] / 672, counts[0] / 32, counts[1] / 64, counts[2] / 64, counts[3] / 512], f"iteration {i}: {counts}"
        seen += 1
    assert seen >= 2 and (tr._nl is not False) == native
    NR._el()._close(tr)
    with open(tmp_path / "run" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0][-5:] == REDO_KEYS and len(rows) == 5 and float(rows[-1][-5]) == res["dormant_frac"]
    assert "dormant_frac_fc1: " in open(tmp_path / "run" / "msg.log").read()


def test_handles_and_python_classes_end_on_the_same_state(tmp_path, monkeypatch):
    """Six iterations of three updates once training has started; the Python classes run their first updates eagerly and the rest from a hipGraph, which holds the
    three launches like every other of the update."""
    NR = _nr()
    a = NR._run(tmp_path, monkeypatch, False, "dqn", ON, False, "py", freq=0)
    b = NR._run(tmp_path, monkeypatch, True, "dqn", ON, False, "nat", freq=0)
    _assert_same_run(a, b)
    steps = a[0][4][1].item()
    assert steps >= 6 and a[0][4][7].item() == 0 and a[1][-1]["dormant_frac"] > 0, "recycles happened"
    plain = NR._run(tmp_path, monkeypatch, True, "dqn", [], False, "plain", freq=0)
    assert plain[0][4][1].item() == steps and not torch.equal(plain[0][0], a[0][0]), "the setting changes the network"
    assert not any(k.startswith("dormant") for k in plain[1][-1])


@pytest.mark.parametrize("save_native,load_native", [(True, True), (False, True)], ids=["handles", "python-to-handles"])
def test_a_snapshot_between_two_recycles_resumes_across_the_next(save_native, load_native, tmp_path, monkeypatch):
    NR = _nr()
    on = ["learner.redo_freq=4", f"learner.redo_tau={TAU_LOOP}"]          # period 4 against three updates per iteration: the snapshot falls between two recycles
    want = NR._run(tmp_path, monkeypatch, load_native, "dqn", on, False, "a", freq=0)
    tr = NR._trainer(tmp_path, monkeypatch, save_native, "dqn", on, False, "b", freq=0)
    for _ in range(4):
        tr.run_iteration()
    at = tr.learner.engine.state[1].item()
    assert at >= 4 and at % 4 != 0, "behind a recycle, in front of the next"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    NR._el()._close(tr)
    tr = NR._trainer(tmp_path, monkeypatch, load_native, "dqn", on, False, "c", freq=0, seed=7)
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = NR._state(tr)
    assert tr.learner.engine.state[1].item() // 4 > at // 4, "a recycle happened after the snapshot"
    NR._el()._close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    _same_results(res[-1:], want[1][-1:])


def test_every_learner_setting_at_once(tmp_path, monkeypatch):
    """clip_grad_norm, target_tau, weight_decay, aug_shift and net_reset_freq = 6 beside redo_freq = 3: at update 6 a recycle and a reset coincide (the reset
    overwrites), at updates 3, 9, ... the recycle stands alone."""
    NR = _nr()
    extra = ON + ["learner.clip_grad_norm=5.0", "learner.target_tau=0.25", "learner.weight_decay=0.01", "learner.aug_shift=4"]
    a = NR._run(tmp_path, monkeypatch, False, "dqn", extra, False, "py", freq=6)
    b = NR._run(tmp_path, monkeypatch, True, "dqn", extra, False, "nat", freq=6)
    _assert_same_run(a, b)
    state = a[0][4]
    assert state[1].item() >= 9 and state[7].item() == state[1].item() // 6 * 6 and a[1][-1]["net_resets"] >= 1 and not math.isnan(a[1][-1]["dormant_frac"])
