"""GPU (MI355X): the optimizer and step-state kernels (csrc/optim.hip, csrc/update_tail.h) against float64 at their edges.

The other optimizer suites hold the Adam forms to each other; this one holds each of them to tests/optim_ref.py, an independent float64 evaluation of
oracle/learner.py's Adam and RMSprop on the fp32 inputs and fp32 constants the kernels receive (tests/test_optim_reference_helpers.py anchors it to
torch.optim in float64).  The scalars the kernels step with are checked first — within one fp32 ulp of the Python model: device pow and sqrt in double err
far below an fp32 ulp, so only the cast can land on the other side — and the element references are then evaluated on the scalars the device published.

Bounds (U = 2^-24 one fp32 rounding, TINY = 2^-126 the absolute allowance where a term can underflow or be flushed; every bound is then doubled, MARGIN,
so that a literal fp32 evaluation sits within half of it, which the helper test checks for both arithmetic forms — fused and rounded-product — on every
case run here; SECOND_ORDER covers products of two first-order terms):
  * m' = m + (g - m) w1: the difference, the product (or nothing, fused) and the sum round, each at no more than |m| + |g|: 3 U (|m| + |g|) + 2 TINY.
  * v' = v b2 + (w2 g) g: v b2 rounds once, (w2 g) g twice, the sum once, and every term is non-negative and at most v': 3 U v' + 3 TINY.  At a denormal or
    zero v the absolute allowance is all there is.
  * denom = sqrt(v') / bc2_sqrt + eps: sqrtf and the division are correctly rounded (hipcc's default).  The square root maps the interval
    [v' - e_v, v' + e_v] (its lower end held at 0) to an interval around sqrt(v'): e_root is its wider half plus one rounding.  Near v' = 0 that is
    sqrt(e_v), not e_v / sqrt(v'): the bound carries it and small v is not avoided.  e_denom = e_root / bc2_sqrt + U sqrt(v') / bc2_sqrt + U denom + TINY.
  * r = m' / denom: (e_m + |r| e_denom) / (denom - e_denom) + U |r| + TINY.
  * p' = p - step_size r, one fused multiply-add: step_size e_r + U (|p'| + step_size |r|) + TINY.  With p = 0 the step is tested at its own precision.
  * the clip form: g c is one rounded product of g and the fp32 coefficient, U |g c| (plus CLIP_ROUNDINGS for the coefficient itself, formed here in numpy
    fp32 from the partials' sum), which enters m' with the factor w1 and v' with 2 w2 |g c|.
  * RMSprop likewise: s' = s alpha + (w g) g with 3 U s' + 3 TINY, the root as above, denom = root + eps one rounding, r = g / denom, then lr r and the
    difference: lr e_r + U lr |r| + TINY + U |p'|.  Contracted, two of these roundings vanish: one bound serves both contractions.
  * a0_clip_coef_kernel: an fp32 sum of n non-negative squares, ceil(n / 256) sequential adds per lane, then an eight-step tree: (ceil(n / 256) + 8 + 1) U
    relative on the sum, half of that on the norm, and three more roundings (the root, + 1e-6, the quotient) for the coefficient.
  * the loss mean: mean_rows_tol of actor_tail_cases (a lane's strided sum, the tree over 256, the division).
Everything that is not arithmetic is compared as bit patterns: elements in [n, n_total), guard floats in front of and behind every buffer, the target on and
off a sync step, a skipped step's parameters and moments, the status words."""
import numpy as np
import pytest
import torch

import optim_ref as R
import recipe
from test_gpu_update_tail import _World

pytestmark = pytest.mark.gpu

F32 = np.float32
LR, B1, B2 = R.HP["lr"], R.HP["b1"], R.HP["b2"]
GUARD = 8
CONV_END = 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64          # C = 4: the convolution floats of _World
SECOND_TRIP = 4 * 2048 * 256 + 4


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _Buf:
    """A device buffer [lead | values | GUARD] of floats: ``lead`` = 4 keeps the values 16-byte aligned, 1 puts them 4 bytes behind a 16-byte boundary."""

    def __init__(self, hip, values, lead=4):
        values = np.ascontiguousarray(values, F32)
        host = np.full(lead + values.size + GUARD, -7.25, F32)
        host[lead:lead + values.size] = values
        self.full = torch.from_numpy(host).to(hip.device)
        assert self.full.data_ptr() % 16 == 0
        self.lead, self.n = lead, values.size
        self.view = self.full[lead:lead + values.size]
        self.before = self.full.clone()

    def snapshot(self):
        self.before = self.full.clone()

    def host(self):
        return self.view.cpu().numpy()

    def untouched_outside(self, lo, hi, what):
        """Every word of the buffer outside values[lo, hi) — the guards included — holds the bits it held at the last snapshot."""
        a, b = _bits(self.full), _bits(self.before)
        for s in (slice(0, self.lead + lo), slice(self.lead + hi, None)):
            same = torch.equal(a[s], b[s])
            if not same:
                bad = (a[s] != b[s]).nonzero().flatten().tolist()
                print(f"{what}: {len(bad)} words outside [{lo}, {hi}) were written, first {bad[:8]} of slice {s}")
            assert same, f"{what}: written outside [{lo}, {hi})"


def _state(hip, steps=0, reset=0, flag=0):
    return torch.tensor([flag, steps, 0, 0, 0, 0, 0, reset], dtype=torch.int32, device=hip.device)


def _check_scalars(scal, S, what):
    got = scal[:2].tolist()
    assert R.within_one_ulp(got[0], S["step_size"]) and R.within_one_ulp(got[1], S["bc2_sqrt"]), f"{what}: scalars {got}, model {S}"
    return got


def _compare(ref, got, inputs, what):
    """Print the worst fraction of each bound, then assert; a failure names the worst element and its inputs."""
    res = {k: R.worst(k, got[k], ref[k], ref["e_" + k], inputs) for k in "pmv"}
    print(f"{what}: worst fraction of the bound: " + ", ".join(f"{k}' {res[k][0]:.3f}" for k in "pmv"))
    for k in "pmv":
        if res[k][0] > 1.0:
            print(f"{what}: {res[k][1]}")
        assert res[k][0] <= 1.0, f"{what}: {res[k][1]}"


def _tiled_table(n):
    T = R.adam_table()
    return {k: np.resize(T[k], n) for k in "pmvg"}


# ------------------------------------------------------------------------------------------------ Adam, the plain forms
# form -> (entry, n, n_total, lead, clip)
PLAIN = {
    "adam_step": ("step", R.TABLE_N, R.TABLE_N, 4, None),
    "sync-16B": ("sync", R.TABLE_N, R.TABLE_N + 260, 4, None),
    "sync-scalar-n%4==3": ("sync", R.TABLE_N - 1, R.TABLE_N + 4, 4, None),
    "sync-scalar-misaligned": ("sync", R.TABLE_N, R.TABLE_N + 260, 1, None),
    "clip-coef<1": ("clip", R.TABLE_N, R.TABLE_N + 260, 4, "coef<1"),
    "clip-coef==1": ("clip", R.TABLE_N, R.TABLE_N + 260, 4, "coef==1"),
    "sync-16B-second-trip": ("sync", SECOND_TRIP, SECOND_TRIP, 4, None),
}


def _plain_update(hip, form, tname, eps, tf, flag=0):
    entry, n, n_total, lead, clip = PLAIN[form]
    T = _tiled_table(n)
    gen = recipe.gen(77)
    behind = (0.05 * gen.standard_normal(n_total - n)).astype(F32)
    p, m, v, g = _Buf(hip, np.concatenate([T["p"], behind]), lead), _Buf(hip, T["m"], lead), _Buf(hip, T["v"], lead), _Buf(hip, T["g"], lead)
    t = _Buf(hip, (0.05 * gen.standard_normal(n_total)).astype(F32), lead)
    steps, reset = R.T_CASES[tname]
    state, scal = _state(hip, steps, reset, flag), hip.zeros(2)
    model = state.tolist()
    args = (LR, B1, B2, eps, tf)
    coef = None
    if entry == "step":
        hip.adam_step(p.view, g.view, m.view, v.view, n, state, scal, *args)
    elif entry == "sync":
        hip.adam_step_sync(p.view, g.view, m.view, v.view, n, state, scal, *args, t.view, n_total)
    else:
        partials = torch.zeros(256, dtype=torch.float64, device=hip.device)
        partials[3] = R.CLIP_SUMSQ[clip]
        ring = _Buf(hip, np.zeros(3, F32))
        coef, norm = R.clip_coef32(R.CLIP_SUMSQ[clip], R.CLIP_MAX_NORM)
        assert (coef == 1.0) == (clip == "coef==1")
        hip.adam_step_sync_clip(p.view, g.view, m.view, v.view, n, state, scal, *args, t.view, n_total, None, partials, R.CLIP_MAX_NORM, ring.view)
    torch.cuda.synchronize()
    what = f"{form} {tname} eps {eps} tf {tf} flag {flag}"
    S = R.step_update(model, None, LR, B1, B2, tf, "plain")
    assert state.tolist() == model, f"{what}: status words {state.tolist()}, model {model}"
    ss, bc2 = _check_scalars(scal, S, what)
    if entry == "clip":
        assert ring.host().tolist() == [norm, 0.0, 0.0], f"{what}: the norm's ring"
        ring.untouched_outside(0, 1, what + " norm ring")
    g.untouched_outside(0, 0, what + " g")
    if S["skip"]:
        for b, name in ((p, "p"), (m, "m"), (v, "v")):
            b.untouched_outside(0, 0, f"{what} skipped {name}")
    else:
        ref = R.adam64(T["p"], T["m"], T["v"], T["g"], R.hyper(B1, B2, eps), ss, bc2, coef=coef, coef_roundings=R.CLIP_ROUNDINGS)
        _compare(ref, dict(p=p.host()[:n], m=m.host(), v=v.host()), T, what)
        p.untouched_outside(0, n, what + " p")
        m.untouched_outside(0, n, what + " m")
        v.untouched_outside(0, n, what + " v")
    if entry != "step" and S["sync"]:
        assert torch.equal(_bits(t.view), _bits(p.view)), f"{what}: on a sync step the target equals p' over [0, n_total)"
        t.untouched_outside(0, n_total, what + " target")
    else:
        t.untouched_outside(0, 0, what + " target")
    return S


@pytest.mark.parametrize("form", [f for f in PLAIN if f != "sync-16B-second-trip"])
def test_adam_forms_against_float64(hip, form):
    seen = set()
    for tname in R.T_CASES:
        for eps in R.EPS_VALUES:
            S = _plain_update(hip, form, tname, eps, 2)
            seen.add(S["sync"])
    assert seen == {0, 1}
    for tf in (1, 2):           # a raised flag: nothing moves; with tf = 1 the target is still copied (the count stays at 9)
        S = _plain_update(hip, form, "t=10", R.EPS_VALUES[0], tf, flag=1)
        assert S["skip"] == 1 and S["sync"] == (tf == 1)


def test_adam_sync_second_grid_stride_trip(hip):
    """n = n_total = 4 * 2048 * 256 + 4: the 16-byte path's 2048 workgroups of 256 lanes take a second trip for the last group of four."""
    assert _plain_update(hip, "sync-16B-second-trip", "t=2", R.EPS_VALUES[0], 2)["sync"] == 1
    _plain_update(hip, "sync-16B-second-trip", "t=10", R.EPS_VALUES[1], 3)


# ------------------------------------------------------------------------------------------------ Adam on the world of the update's tail
N_WORLD, N_TOTAL_WORLD = CONV_END + R.TABLE_N, CONV_END + R.TABLE_N + 260


class _Prep:
    """The tail-prep launch: a0_net_encoder_wgrad_tail at the smallest geometry, its gradients and its plan thrown away — what stays is the bookkeeping it
    ran on ``state`` and ``scal``."""

    def __init__(self, hip):
        from agent0_amd._abi import PendingReduce
        self.hip, self.B, shape = hip, 8, (4, 36, 36)
        self.net = net = hip.net(*shape)
        gen = recipe.gen(41)
        f = lambda k, s=1.0: torch.from_numpy((gen.standard_normal(k) * s).astype(F32)).to(hip.device)
        self.frames = torch.from_numpy(recipe.make_frames(self.B, 5, shape)).to(hip.device).reshape(-1).contiguous()
        self.act1, self.act2 = f(self.B * net.H1 * net.W1 * 32).abs(), f(self.B * net.H2 * net.W2 * 64).abs()
        self.d3, self.d2, self.d1 = f(self.B * net.feat), f(self.B * net.H2 * net.W2 * 64), f(self.B * net.H1 * net.W1 * 32)
        self.flat, self.grad = f(CONV_END, 0.05), hip.empty(CONV_END)
        self.slabs = hip.empty(max(hip.encoder_bwd_scratch(net, self.B), 4))
        self.pend = PendingReduce()

    def __call__(self, state, scal, tf):
        o = (0, 32 * 256 + 32, 32 * 256 + 32 + 64 * 512 + 64, CONV_END)
        w = dict(w1=self.flat[o[0]:o[0] + 32 * 256], b1=self.flat[o[0] + 32 * 256:o[1]], w2=self.flat[o[1]:o[1] + 64 * 512], b2=self.flat[o[1] + 64 * 512:o[2]],
                 w3=self.flat[o[2]:o[2] + 64 * 576], b3=self.flat[o[2] + 64 * 576:o[3]])
        self.pend.n = 0
        self.hip.encoder_wgrad_tail(self.net, w, self.frames, None, self.frames.numel() // self.B, 0, self.B, self.act1, self.act2, self.d3, self.d2, self.d1,
                                    self.grad[o[0]:o[1]], self.grad[o[1]:o[2]], self.grad[o[2]:o[3]], self.slabs, self.pend, state, scal, LR, B1, B2, tf)


@pytest.fixture(scope="module")
def prep(hip):
    return _Prep(hip)


def _edge_world(hip, n_dense_values=None, extra=260):
    """_World at C = 4 with the case table as its dense range, every buffer re-seated between guard floats."""
    T = R.adam_table() if n_dense_values is None else n_dense_values
    nd = T["p"].size
    n, n_total = CONV_END + nd, CONV_END + nd + extra
    w = _World(hip, 4, n, n_total, 4242)
    gen = recipe.gen(4243)
    host = {"p": w.p.cpu().numpy(), "t": w.t.cpu().numpy(), "m": w.m.cpu().numpy(), "v": w.v.cpu().numpy(),
            "g": (0.1 * gen.standard_normal(n_total)).astype(F32)}
    for k in "pmvg":
        host[k][CONV_END:n] = T[k]
    w.buf = {k: _Buf(hip, host[k]) for k in host}
    w.p, w.t, w.m, w.v, w.g = (w.buf[k].view for k in "ptmvg")
    hip.conv_wt_refresh(w.weights(w.p), 4, w.wt)
    hip.conv_wt_refresh(w.weights(w.t), 4, w.wt_t)
    w.host = host
    return w


def _fold(hip, w, eps, tf, extra=None, loss=None, loss_n=0, ring=None):
    hip.adam_step_sync_wt(w.p, w.g, w.m, w.v, w.n, w.state, w.scal, LR, B1, B2, eps, tf, w.t, w.n_total, extra, w.weights(w.p), 4, w.wt, w.wt_t, loss, loss_n, ring)


def _tail(hip, prep, w, eps, tf, loss=None, loss_n=0, ring=None):
    from agent0_amd._abi import UpdateTailPlan
    prep(w.state, w.scal, tf)
    plan = UpdateTailPlan()
    plan.n = 0
    hip.update_tail(w.p, w.g, w.m, w.v, w.n, w.state, w.scal, B1, B2, eps, w.t, w.n_total, plan, w.weights(w.p), 4, w.wt, w.wt_t, loss, loss_n, ring)


def _set_state(w, steps, reset, flag=0):
    w.state.copy_(torch.tensor([flag, steps, 0, 0, 0, 0, 0, reset], dtype=torch.int32))


@pytest.mark.parametrize("eps", R.EPS_VALUES)
def test_adam_step_sync_wt_against_float64(hip, eps):
    for tname in R.T_CASES:
        w = _edge_world(hip)
        n, n_total = w.n, w.n_total
        _set_state(w, *R.T_CASES[tname])
        model = w.state.tolist()
        _fold(hip, w, eps, 2)
        torch.cuda.synchronize()
        what = f"a0_adam_step_sync_wt {tname} eps {eps}"
        S = R.step_update(model, None, LR, B1, B2, 2, "folded")
        assert w.state.tolist() == model, f"{what}: status words {w.state.tolist()}, model {model}"
        ss, bc2 = _check_scalars(w.scal, S, what)
        h = w.host
        ins = {k: h[k][:n] for k in "pmvg"}
        ref = R.adam64(ins["p"], ins["m"], ins["v"], ins["g"], R.hyper(B1, B2, eps), ss, bc2)
        _compare(ref, dict(p=w.buf["p"].host()[:n], m=w.buf["m"].host(), v=w.buf["v"].host()), ins, what)
        for k in "pmv":
            w.buf[k].untouched_outside(0, n, f"{what} {k}")
        w.buf["g"].untouched_outside(0, 0, what + " g")
        if S["sync"]:
            assert torch.equal(_bits(w.t), _bits(w.p)) and torch.equal(_bits(w.wt_t), _bits(w.wt)), f"{what}: the target and its weight copies on a sync step"
            w.buf["t"].untouched_outside(0, n_total, what + " target")
        else:
            w.buf["t"].untouched_outside(0, 0, what + " target")
        fresh = hip.empty(hip.conv_wt_floats(4))
        hip.conv_wt_refresh(w.weights(w.p), 4, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(w.wt)), f"{what}: the weight copies are a refresh from the new weights"


@pytest.mark.parametrize("tname,tf,flag", [("t=1", 2, 0), ("t=2", 2, 0), ("t=1e7", 3, 0), ("steps==reset", 2, 0), ("t=10", 1, 1)])
def test_update_tail_with_an_empty_plan_equals_adam_step_sync_wt(hip, prep, tname, tf, flag):
    eps = R.EPS_VALUES[0]
    old, new = _edge_world(hip), _edge_world(hip)
    loss = torch.from_numpy(recipe.gen(5).standard_normal(8).astype(F32)).to(hip.device)
    for w in (old, new):
        _set_state(w, *R.T_CASES[tname], flag)
    _fold(hip, old, eps, tf, None, loss, 8, old.ring)
    _tail(hip, prep, new, eps, tf, loss, 8, new.ring)
    torch.cuda.synchronize()
    a, b = old.everything(), new.everything()
    a.update({k: old.buf[k].full for k in old.buf})
    b.update({k: new.buf[k].full for k in new.buf})
    for k in a:
        same = torch.equal(_bits(a[k]), _bits(b[k]))
        if not same:
            bad = (_bits(a[k]) != _bits(b[k])).nonzero().flatten().tolist()
            print(f"{tname}: {k}: {len(bad)} of {a[k].numel()} words differ, first {bad[:12]}, folded {a[k][bad[:4]].tolist()} tail {b[k][bad[:4]].tolist()}")
        assert same, f"{tname}: {k}"
    assert (old.state[3].item(), old.state[4].item()) == (flag, int((R.T_CASES[tname][0] + 1 - flag) % tf == 0))


# ------------------------------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("form", ["adam_step", "sync-16B", "sync-scalar-misaligned"])
def test_a_non_finite_gradient_stays_in_its_element(hip, form):
    T = R.nonfinite_table()
    n, lead = 64, 1 if form.endswith("misaligned") else 4
    eps = R.EPS_VALUES[0]
    H = R.hyper(B1, B2, eps)

    def run(g_host):
        b = {k: _Buf(hip, T[k] if k != "g" else g_host, lead) for k in "pmvg"}
        t = _Buf(hip, np.zeros(n, F32), lead)
        state, scal = _state(hip, 9), hip.zeros(2)
        if form == "adam_step":
            hip.adam_step(b["p"].view, b["g"].view, b["m"].view, b["v"].view, n, state, scal, LR, B1, B2, eps, 2)
        else:
            hip.adam_step_sync(b["p"].view, b["g"].view, b["m"].view, b["v"].view, n, state, scal, LR, B1, B2, eps, 2, t.view, n)
        torch.cuda.synchronize()
        assert state[4].item() == 1
        if form != "adam_step":
            assert torch.equal(_bits(t.view), _bits(b["p"].view))
        return {k: b[k].full.cpu().numpy().view(np.int32) for k in "pmv"}, {k: b[k].host() for k in "pmv"}, scal.tolist()

    for idx, val in R.NONFINITE:
        g_bad, g_zero = T["g"].copy(), T["g"].copy()
        g_bad[idx], g_zero[idx] = val, 0.0
        bad_bits, bad, scal = run(g_bad)
        zero_bits, _, _ = run(g_zero)
        ref = R.adam64(T["p"], T["m"], T["v"], g_bad, H, scal[0], scal[1])
        for k in "pmv":
            other = np.ones(bad_bits[k].size, bool)
            other[lead + idx] = False
            assert (bad_bits[k][other] == zero_bits[k][other]).all(), f"{form}: g[{idx}] = {val}: {k} leaks into {np.nonzero(bad_bits[k] != zero_bits[k])[0].tolist()}"
            want, got = int(R.value_class(ref[k][idx])), int(R.value_class(bad[k][idx]))
            assert want == got, f"{form}: g[{idx}] = {val}: {k}' = {bad[k][idx]}, float64 gives {ref[k][idx]}"


# ------------------------------------------------------------------------------------------------ the bookkeeping
@pytest.mark.parametrize("family", ["adam_step", "adam_step_sync", "adam_step_sync_wt", "tail_prep+update_tail"])
def test_twelve_updates_of_bookkeeping(hip, prep, family):
    dev = hip.device
    has_extra = family in ("adam_step_sync", "adam_step_sync_wt")
    form = {"adam_step": "plain", "adam_step_sync": "plain", "adam_step_sync_wt": "folded", "tail_prep+update_tail": "tail"}[family]
    gen = recipe.gen(12)
    small = {k: (0.05 * gen.standard_normal(8)).astype(F32) for k in "pmvg"}
    small["v"] = np.abs(small["v"])
    if family.startswith("adam_step_sync_wt") or family.startswith("tail"):
        w = _edge_world(hip, small, extra=4)
        p, m, v, g, t, state, scal, n, n_total = w.p, w.m, w.v, w.g, w.t, w.state, w.scal, w.n, w.n_total
    else:
        p, m, v, g, t = (_Buf(hip, small[k]).view for k in "pmvgp")
        state, scal, n, n_total = _state(hip), hip.zeros(2), 8, 8
    flag_out = hip.zeros(1)
    extra_t = hip.zeros(1)
    model = [0] * 8
    eps = R.EPS_VALUES[0]

    def exported():
        hip.nan_flag_export(state, flag_out)
        torch.cuda.synchronize()
        return flag_out.item()

    for u, (kind, reset, tf) in enumerate(R.SCHEDULE):
        up, extra = R.schedule_flags(kind, has_extra)
        if up:
            state[0] = 1
            model[0] = 1
        if reset is not None:
            state[7] = reset
            model[7] = reset
        assert exported() == (1.0 if up else 0.0), f"update {u}: a0_nan_flag_export in front of the update"
        if has_extra:
            extra_t.fill_(extra)
        p0, m0 = p.clone(), m.clone()
        if family == "adam_step":
            hip.adam_step(p, g, m, v, n, state, scal, LR, B1, B2, eps, tf)
        elif family == "adam_step_sync":
            hip.adam_step_sync(p, g, m, v, n, state, scal, LR, B1, B2, eps, tf, t, n_total, extra_t)
        elif family == "adam_step_sync_wt":
            _fold(hip, w, eps, tf, extra_t)
        else:
            _tail(hip, prep, w, eps, tf)
        torch.cuda.synchronize()
        S = R.step_update(model, extra, LR, B1, B2, tf, form)
        what = f"{family} update {u} {R.SCHEDULE[u]}"
        assert state.tolist() == model, f"{what}: status words {state.tolist()}, model {model}"
        _check_scalars(scal, S, what)
        assert exported() == 0.0, f"{what}: a0_nan_flag_export behind the update"
        moved = not (torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(m), _bits(m0)))
        assert moved == (not S["skip"]), f"{what}: a step moves the parameters and moments, a skipped one leaves them alone"
        if S["sync"] and family != "adam_step":
            assert torch.equal(_bits(t), _bits(p)), f"{what}: target"
    assert model[:6] == [0, 9, 3, 0, 1, 0 if form == "plain" else 9]


# ------------------------------------------------------------------------------------------------ RMSprop
@pytest.mark.parametrize("n", R.RMSPROP_NS)
def test_rmsprop_against_float64(hip, n):
    for zero_p in (True, False):
        for zero_sq in (True, False):
            for clip in R.RMSPROP_CLIPS:
                p0, s0, gs = R.rmsprop_case(n, zero_p, zero_sq)
                p, sq, scratch = _Buf(hip, p0), _Buf(hip, s0), _Buf(hip, np.full(1, 3.5, F32))
                for step, gh in enumerate(gs):
                    g = _Buf(hip, gh)
                    max_norm = R.rmsprop_max_norm(gh, clip)
                    for b in (p, sq, scratch):
                        b.snapshot()
                    p0, s0 = p.host(), sq.host()
                    hip.rmsprop_step(p.view, g.view, sq.view, n, R.RMS["lr"], R.RMS["alpha"], R.RMS["eps"], max_norm, None if clip == "off" else scratch.view)
                    torch.cuda.synchronize()
                    what = f"n {n} p = 0 {zero_p} sq = 0 {zero_sq} clip {clip} step {step}"
                    coef = None
                    if clip == "off":
                        scratch.untouched_outside(0, 0, what + " scratch")
                    else:
                        coef = float(scratch.host()[0])
                        c64, _, rel, raw = R.clip_coef64(gh, max_norm)
                        print(f"{what}: coefficient {coef!r}, float64 {c64!r}, {abs(coef - c64) / (rel * c64):.3f} of its bound")
                        assert (c64 == 1.0) == (clip == "inactive") and (raw < 0.5 or raw > 1.5)
                        assert coef == 1.0 if clip == "inactive" else abs(coef - c64) <= rel * c64, f"{what}: coefficient {coef!r}, float64 {c64!r}, relative bound {rel:.3e}"
                        scratch.untouched_outside(0, 1, what + " scratch")
                    ref = R.rmsprop64(p0, s0, gh, **R.RMS, coef=coef)
                    for name, got, key in (("p", p.host(), "p"), ("sq", sq.host(), "sq")):
                        frac, msg = R.worst(name, got, ref[key], ref["e_" + key], dict(p=p0, sq=s0, g=gh, coef=1.0 if coef is None else coef))
                        print(f"{what}: {name}' worst fraction of the bound {frac:.3f}")
                        if frac > 1.0:
                            print(f"{what}: {msg}")
                        assert frac <= 1.0, f"{what}: {msg}"
                    p.untouched_outside(0, n, what + " p")
                    sq.untouched_outside(0, n, what + " sq")
                    g.untouched_outside(0, 0, what + " g")


# ------------------------------------------------------------------------------------------------ the hard target copy
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4 * 2048 * 256 + 5])
def test_target_sync_bit_exact_and_in_bounds(hip, n):
    gen = recipe.gen(700 + n % 1000)
    src_host = gen.standard_normal(n).astype(F32)
    src_host[0], src_host[-1] = np.nan, -0.0
    src_host[n // 2] = F32(2.0 ** -140)
    for force, word, copies in ((1, 0, True), (0, 1, True), (0, 0, False), (1, None, True)):
        src, dst = _Buf(hip, src_host), _Buf(hip, gen.standard_normal(n).astype(F32))
        state = None if word is None else torch.tensor([0, 0, 0, 0, word, 0, 0, 0], dtype=torch.int32, device=hip.device)
        hip.target_sync(dst.view, src.view, n, state, force)
        torch.cuda.synchronize()
        what = f"n {n} force {force} state[4] {word}"
        if copies:
            assert torch.equal(_bits(dst.view), _bits(src.view)), what
            dst.untouched_outside(0, n, what + " target")
        else:
            dst.untouched_outside(0, 0, what + " target")
        src.untouched_outside(0, 0, what + " online")


# ------------------------------------------------------------------------------------------------ the loss mean's ring slot
@pytest.mark.parametrize("loss_n", [1, 8, 255, 256, 257, 512])
def test_loss_mean_to_ring(hip, loss_n):
    gen = recipe.gen(800 + loss_n)
    small = {k: (0.05 * gen.standard_normal(8)).astype(F32) for k in "pmvg"}
    small["v"] = np.abs(small["v"])
    w = _edge_world(hip, small, extra=4)
    for cap in (1, 7):
        for count, with_nan in ((1000003, False), (5, False), (2 ** 31 - 9, True)):
            x = (gen.standard_normal(loss_n) * (1.0 + gen.random())).astype(F32)
            if with_nan:
                x[loss_n // 2] = np.nan
            loss = _Buf(hip, x)
            ring = _Buf(hip, gen.standard_normal(cap).astype(F32))
            w.state[6] = count
            _fold(hip, w, R.EPS_VALUES[0], 0, None, loss.view, loss_n, ring.view)
            torch.cuda.synchronize()
            what = f"loss_n {loss_n} ring {cap} state[6] {count}"
            slot = count % cap
            got = float(ring.host()[slot])
            assert w.state[6].item() == count + 1, what
            if with_nan:
                assert np.isnan(got), f"{what}: a NaN loss is recorded as NaN, got {got}"
            else:
                mean, tol = R.loss_mean64(x)
                print(f"{what}: mean {got!r}, float64 {mean!r}, {abs(got - mean) / tol:.3f} of its bound")
                assert abs(got - mean) <= tol, f"{what}: mean {got!r}, float64 {mean!r}, bound {tol:.3e}"
            ring.untouched_outside(slot, slot + 1, what + " ring")
            loss.untouched_outside(0, 0, what + " loss")
