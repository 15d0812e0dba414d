"""GPU (MI355X): the convolution kernels against float64, layer by layer, at the batch sizes where their work splits change.

Kernels: the learner's forward (encoder_fwd_fused: a0_encoder_fused_kernel, one observation per workgroup up to 256 and looping beyond;
encoder_fwd_fused_multi: a0_encoder_fused_multi_kernel; encoder_fwd: the implicit GEMMs), its data gradient (encoder_dgrad_fused:
a0_encoder_dgrad_fused_x9_kernel, gridx = min(B, 256); encoder_bwd), its weight gradients (encoder_wgrad: conv23_wgrad.hip with G = min(B, 72) groups,
conv1_wgrad.hip with min(B, 256) slabs; encoder_bwd: the implicit GEMMs and conv1_wgrad.hip) and the encoder inside the merged actor step
(a0_actor_*_env_step_enc).

Tolerance model: every output element against its float64 value, the error divided by that element's accumulated magnitude (the same convolution on
|a| and |b|, plus |bias| where one applies; tests/util.py).  Each layer's reference takes the device's own inputs to that layer (its act1 for conv2,
its act1 / act2 > 0 as the data gradients' masks, its d2 for conv2's weight gradient, ...), so the error is local to the layer and no ReLU decision
at a rounding-level pre-activation enters the comparison.  The kernels accumulate exact products (three-term bf16 splits, bytes exact in bf16) in
fp32: a few 1e-7 of the scale; the bound is 2e-6 (test_gpu_gemm.py's).  Every output is prefilled with NaN and followed by 64 sentinel elements:
each element must be written and finite, each sentinel must survive.  Negative controls build, on the CPU, the result of a lost observation and of a
lost split term, and assert that the same bound rejects them."""
import numpy as np
import pytest
import torch

import recipe
from util import (CONV_STRIDES, conv_dgrad64, conv_fwd64, conv_params64, conv_w_from_kernel, conv_wgrad64, encoder_chain64, nchw_from_nhwc,
                  record_stats, round_bf16, scale_err)

pytestmark = pytest.mark.gpu

TOL = 2e-6
GUARD = 64
SENTINEL = -1.25e38                      # exact in fp32
SENTINEL_U8 = 0xA5
G84, G36, G4452 = (4, 84, 84), (4, 36, 36), (4, 44, 52)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


# ------------------------------------------------------------------------------------------------ helpers
_NETS, _BWD, _C1 = {}, {}, {}


def _net(hip, shape):
    if shape not in _NETS:
        from agent0_amd.deepq.engine import DeviceNet
        from agent0_amd.deepq.layout import NetLayout
        spec = recipe.NetSpec("dqn", 4, obs_shape=shape)
        L = NetLayout.from_spec(spec)
        net = DeviceNet(hip, L, hip.net(*shape))
        sd = recipe.make_state_dict(spec, 11)
        net.load_state_dict(sd)
        _NETS[shape] = (net, L, conv_params64(sd))
    return _NETS[shape]


def _geo(shape):
    C, H, W = shape
    H1, W1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
    H2, W2 = (H1 - 4) // 2 + 1, (W1 - 4) // 2 + 1
    return (H1, W1), (H2, W2), (H2 - 2, W2 - 2)


def _guarded(hip, n, dtype=torch.float32):
    buf = hip.empty(n + GUARD, dtype=dtype)
    if dtype == torch.uint8:
        buf.fill_(SENTINEL_U8)
    else:
        buf[:n].fill_(float("nan"))
        buf[n:].fill_(SENTINEL)
    return buf


def _check_guard(buf, n, what, written=True):
    """``written=False``: scratch (slab regions are sized for the largest plan; only the slabs a launch uses are written): the guard band only."""
    if buf.dtype == torch.uint8 or not written:
        assert bool((buf[n:] == (SENTINEL_U8 if buf.dtype == torch.uint8 else SENTINEL)).all()), f"{what}: write past the end"
        return
    assert bool(torch.isfinite(buf[:n]).all()), f"{what}: {int((~torch.isfinite(buf[:n])).sum())} of {n} elements unwritten or not finite"
    assert bool((buf[n:] == SENTINEL).all()), f"{what}: write past the end"


def _check(got, want, scale, what, tol=TOL):
    err = scale_err(got, want, scale)
    worst = float(np.abs(err).max())
    assert worst < tol, f"{what}: {worst:.3e} of the accumulated magnitude (bound {tol:g})"
    return err


def _rejected(got, want, scale, what, tol=TOL):
    worst = float(np.abs(scale_err(got, want, scale)).max())
    assert worst >= tol, f"negative control {what}: the bound {tol:g} does not reject it ({worst:.3e})"


def _ring(shape, B, seed):
    """Replay ring of B + 5 samples st || st_next [2C][H][W] (u8) with whole rows of 0 and of 255 among random ones, and the slots of a batch."""
    C, H, W = shape
    cap = B + 5
    ring = recipe.make_frames(cap, seed, shape)
    g = recipe.gen(seed + 1)
    slot = g.permutation(cap)[:B].astype(np.int32)
    ring[slot[0], :, :4, :] = 0
    ring[slot[B // 2], :, H // 2:H // 2 + 3, :] = 255
    ring[slot[-1], :, H - 2:, :] = 255
    ring[slot[-1], :, 5, :] = 0
    return ring, slot


def _obs64(ring, slot, chan_off, C, hw):
    c0 = chan_off // hw
    return torch.from_numpy(ring[slot, c0:c0 + C].astype(np.float64)) / 255.0


def _conv1_ref(key, x, params):
    if key not in _C1:
        _C1[key] = conv_fwd64(x, *params[0], CONV_STRIDES[0])
    return _C1[key]


# ------------------------------------------------------------------------------------------------ 1. learner forward
FWD_CASES = [(G84, b) for b in (1, 2, 255, 256, 257, 513)] + [(G36, 3), (G36, 300), (G4452, 9), (G4452, 257)]


@pytest.mark.parametrize("shape,B", FWD_CASES)
def test_forward_layers_against_float64(hip, shape, B):
    """act1, act2, act3 of encoder_fwd_fused, encoder_fwd and (84 x 84) both passes of encoder_fwd_fused_multi, each layer on the device's input to it;
    frames through a replay-slot gather, st (chan_off 0) and st_next (chan_off = ob)."""
    net, L, params = _net(hip, shape)
    C, H, W = shape
    ob, hw = C * H * W, H * W
    (H1, W1), (H2, W2), (H3, W3) = _geo(shape)
    n1, n2, n3 = B * H1 * W1 * 32, B * H2 * W2 * 64, B * H3 * W3 * 64
    ring_np, slot_np = _ring(shape, B, 100 + B)
    ring = torch.from_numpy(ring_np.reshape(-1)).to(hip.device)
    slot = torch.from_numpy(slot_np).to(hip.device)
    off = ob if B % 2 else 0
    runs = []
    for kind in ("fused", "unfused"):
        a = [_guarded(hip, n) for n in (n1, n2, n3)]
        if kind == "fused":
            hip.encoder_fwd_fused(net.net, net.wt, net.encoder_weights(), ring, slot, 2 * ob, off, B, *a)
        else:
            hip.encoder_fwd(net.net, net.encoder_weights(), ring, slot, 2 * ob, off, B, *a)
        runs.append((kind, off, a))
    if shape == G84:
        passes = []
        for o in (0, ob):
            a = [_guarded(hip, n) for n in (n1, n2, n3)]
            passes.append((net.wt, net.encoder_weights(), ring, slot, 2 * ob, o, B, *a))
            runs.append((f"multi@{o}", o, a))
        hip.encoder_fwd_fused_multi(net.net, passes)
    torch.cuda.synchronize()
    stats = {}
    for kind, o, a in runs:
        for t, n, name in zip(a, (n1, n2, n3), ("act1", "act2", "act3")):
            _check_guard(t, n, f"{kind} {name}")
        x = _obs64(ring_np, slot_np, o, C, hw)
        acts = [nchw_from_nhwc(a[0][:n1], B, H1, W1, 32), nchw_from_nhwc(a[1][:n2], B, H2, W2, 64), nchw_from_nhwc(a[2][:n3], B, H3, W3, 64)]
        for layer in range(3):
            want, scale = _conv1_ref((shape, B, o), x, params) if layer == 0 else conv_fwd64(acts[layer - 1], *params[layer], CONV_STRIDES[layer])
            err = _check(acts[layer], want, scale, f"{kind} conv{layer + 1} {shape} B={B}")
            stats[f"{kind}.conv{layer + 1}"] = float(np.abs(err).max())
            if kind == "fused" and layer == 1 and (shape, B) == (G84, 256):
                # negative control: conv2 with both operands cut to their leading bf16 term (a lost split term)
                lost, _ = conv_fwd64(round_bf16(acts[0]), round_bf16(params[1][0]), params[1][1], CONV_STRIDES[1])
                _rejected(lost, want, scale, "conv2 forward on single bf16 terms")
    record_stats(f"conv_fwd_{'x'.join(map(str, shape))}_B{B}", stats)


# ------------------------------------------------------------------------------------------------ 2./3. learner backward
BWD_BS = (1, 2, 72, 73, 145, 256, 257, 512)
BWD_CASES = [(s, b) for s in (G84, G36, G4452) for b in BWD_BS]


def _bwd(hip, shape, B):
    """One backward case, run once per module: the device's forward (fused), a d3 masked by its act3 > 0 with whole observations and positions of zeros,
    then encoder_bwd and (84 x 84) encoder_dgrad_fused + encoder_wgrad, every output guarded.  Host copies of everything the checks read."""
    key = (shape, B)
    if key in _BWD:
        return _BWD[key]
    net, L, params = _net(hip, shape)
    C, H, W = shape
    ob, hw = C * H * W, H * W
    (H1, W1), (H2, W2), (H3, W3) = _geo(shape)
    n1, n2, n3 = B * H1 * W1 * 32, B * H2 * W2 * 64, B * H3 * W3 * 64
    K1, K2, K3 = C * 64, 512, 576
    ng = (32 * K1 + 32, 64 * K2 + 64, 64 * K3 + 64)
    ring_np, slot_np = _ring(shape, B, 200 + B)
    ring = torch.from_numpy(ring_np.reshape(-1)).to(hip.device)
    slot = torch.from_numpy(slot_np).to(hip.device)
    off = ob if B % 2 else 0
    act1, act2, act3 = (hip.empty(n) for n in (n1, n2, n3))
    hip.encoder_fwd_fused(net.net, net.wt, net.encoder_weights(), ring, slot, 2 * ob, off, B, act1, act2, act3)
    g = recipe.gen(300 + B)
    d3 = torch.from_numpy(g.standard_normal(n3).astype(np.float32)).to(hip.device) * (act3 > 0)
    d3v = d3.view(B, H3 * W3, 64)
    if B > 1:
        d3v[1].zero_()                         # an observation without any gradient
    d3v[:, 3::7].zero_()                       # and rows of positions without one
    d3 = d3.contiguous()
    need = hip.encoder_bwd_scratch(net.net, B)
    paths = {}
    outs = {k: _guarded(hip, n) for k, n in (("d2", n2), ("d1", n1), ("g1", ng[0]), ("g2", ng[1]), ("g3", ng[2]), ("slabs", need))}
    hip.encoder_bwd(net.net, net.encoder_weights(), ring, slot, 2 * ob, off, B, act1, act2, d3, outs["d2"], outs["d1"], outs["g1"], outs["g2"], outs["g3"],
                    outs["slabs"])
    paths["encoder_bwd"] = outs
    if shape == G84:
        outs = {k: _guarded(hip, n) for k, n in (("d2", n2), ("d1", n1), ("g1", ng[0]), ("g2", ng[1]), ("g3", ng[2]), ("slabs", need))}
        hip.encoder_dgrad_fused(net.net, net.wt, d3, act1, act2, B, outs["d2"], outs["d1"])
        hip.encoder_wgrad(net.net, net.encoder_weights(), ring, slot, 2 * ob, off, B, act1, act2, d3, outs["d2"], outs["d1"], outs["g1"], outs["g2"], outs["g3"],
                          outs["slabs"])
        paths["fused"] = outs
    torch.cuda.synchronize()
    sizes = {"d2": n2, "d1": n1, "g1": ng[0], "g2": ng[1], "g3": ng[2], "slabs": need}
    host = {}
    for p, outs in paths.items():
        for k, buf in outs.items():
            _check_guard(buf, sizes[k], f"{p} {k} {shape} B={B}", written=(k != "slabs"))
        host[p] = {k: outs[k][:sizes[k]].cpu() for k in ("d2", "d1", "g1", "g2", "g3")}
    r = dict(shape=shape, B=B, params=params, dims=((H1, W1), (H2, W2), (H3, W3)), K=(K1, K2, K3),
             x=_obs64(ring_np, slot_np, off, C, hw), act1=nchw_from_nhwc(act1, B, H1, W1, 32), act2=nchw_from_nhwc(act2, B, H2, W2, 64),
             d3=nchw_from_nhwc(d3, B, H3, W3, 64), paths=host)
    _BWD.clear()                               # one case at a time: both tests of a case run back to back
    _BWD[key] = r
    return r


@pytest.mark.parametrize("shape,B", BWD_CASES)
def test_data_gradients_against_float64(hip, shape, B):
    """d2 and d1 of encoder_dgrad_fused (84 x 84) and encoder_bwd: float64 conv-transpose of the device's d3 (for d1: of the path's own d2), masked by the
    device's act2 / act1 > 0; where that mask is 0 the gradient must be exactly 0."""
    r = _bwd(hip, shape, B)
    (H1, W1), (H2, W2), _ = r["dims"]
    m2, m1 = r["act2"] > 0, r["act1"] > 0
    want2, scale2 = conv_dgrad64(r["d3"], r["params"][2][0], 1, (B, 64, H2, W2), m2)
    stats = {}
    for p, o in r["paths"].items():
        d2 = nchw_from_nhwc(o["d2"], B, H2, W2, 64)
        d1 = nchw_from_nhwc(o["d1"], B, H1, W1, 32)
        assert bool((d2[~m2] == 0).all()), f"{p}: d2 nonzero where act2 <= 0"
        assert bool((d1[~m1] == 0).all()), f"{p}: d1 nonzero where act1 <= 0"
        e2 = _check(d2, want2, scale2, f"{p} d2 {shape} B={B}")
        want1, scale1 = conv_dgrad64(d2, r["params"][1][0], 2, (B, 32, H1, W1), m1)
        e1 = _check(d1, want1, scale1, f"{p} d1 {shape} B={B}")
        stats[p] = {"d2": float(np.abs(e2).max()), "d1": float(np.abs(e1).max())}
    record_stats(f"conv_dgrad_{'x'.join(map(str, shape))}_B{B}", stats)


def _bias_bound(K_chain, err):
    rms = float(np.sqrt(np.mean(err ** 2)))
    return 2.5e-8 * np.sqrt(K_chain / 32768.0) + 4.0 * rms / np.sqrt(err.size), float(err.mean()), rms


@pytest.mark.parametrize("shape,B", BWD_CASES)
def test_weight_gradients_against_float64(hip, shape, B):
    """conv1 / conv2 / conv3 weights and biases, each on its own scale, of encoder_wgrad (84 x 84: conv23_wgrad.hip, conv1_wgrad.hip) and encoder_bwd
    (implicit GEMMs; conv1_wgrad.hip at 84 x 84), from the device's inputs to each layer (x, act1, act2) and the path's own gradients (d1, d2, d3).
    At B = 512 the signed mean error of the weight gradients (units of sum |a||b|) must stay within the bf16 pipe's measured accumulation bias,
    2.5e-8 sqrt(K / 32768) (profiles/r06_x6_accuracy.txt), plus 4 rms / sqrt(n); K is the whole reduction (B x positions) — the kernels' longest fp32
    chain is shorter, so the allowance is generous; the figure was unmeasured before these tests' first GPU run."""
    r = _bwd(hip, shape, B)
    (H1, W1), (H2, W2), (H3, W3) = r["dims"]
    positions = (H1 * W1, H2 * W2, H3 * W3)
    w3ref = conv_wgrad64(r["act2"], r["d3"], r["params"][2][0].shape, 1)
    stats = {}
    for p, o in r["paths"].items():
        d2 = nchw_from_nhwc(o["d2"], B, H2, W2, 64)
        d1 = nchw_from_nhwc(o["d1"], B, H1, W1, 32)
        ins = ((r["x"], d1), (r["act1"], d2), (r["act2"], r["d3"]))
        for layer in range(3):
            w_shape = r["params"][layer][0].shape
            N, K = w_shape[0], int(np.prod(w_shape[1:]))
            dw, db, sw, sb = w3ref if layer == 2 else conv_wgrad64(*ins[layer], w_shape, CONV_STRIDES[layer])
            g = o[f"g{layer + 1}"]
            got_w, got_b = conv_w_from_kernel(g[:N * K], layer, shape[0]), g[N * K:N * K + N].double()
            ew = _check(got_w, dw, sw, f"{p} conv{layer + 1}.weight {shape} B={B}")
            eb = _check(got_b, db, sb, f"{p} conv{layer + 1}.bias {shape} B={B}")
            st = {"weight": float(np.abs(ew).max()), "bias": float(np.abs(eb).max())}
            if B == 512:
                bound, mean, rms = _bias_bound(B * positions[layer], ew)
                st.update(signed_mean=mean, rms=rms, n=int(ew.size), K=B * positions[layer], bias_bound=bound)
                assert abs(mean) < bound, f"{p} conv{layer + 1}.weight: signed mean error {mean:.3e} (bound {bound:.3e}, rms {rms:.3e})"
                # negative control: observation 0's contribution lost (or counted twice) by a looping workgroup / an empty group
                assert float(ins[layer][1][0].abs().sum()) > 0
                dw0, db0, _, _ = conv_wgrad64(ins[layer][0][:1], ins[layer][1][:1], w_shape, CONV_STRIDES[layer])
                _rejected(dw - dw0, dw, sw, f"conv{layer + 1}.weight without one observation")
                _rejected(db - db0, db, sb, f"conv{layer + 1}.bias without one observation")
                if layer == 2 and p == "encoder_bwd":
                    # negative control: the weight gradient on single bf16 terms of both operands (a lost split term)
                    lost = conv_wgrad64(round_bf16(r["act2"]), round_bf16(r["d3"]), w_shape, 1)[0]
                    _rejected(lost, dw, sw, "conv3 weight gradient on single bf16 terms")
            stats[f"{p}.conv{layer + 1}"] = st
    record_stats(f"conv_wgrad_{'x'.join(map(str, shape))}_B{B}", stats)


def test_conv1_weight_gradient_at_an_unaligned_sample_stride(hip):
    """A sample stride that is not a multiple of 4: the fused forward refuses it, a0_conv1_wgrad_fused_launch returns 0 and encoder_wgrad takes conv1's
    implicit-GEMM fallback, which must meet the same float64 bound.  The same bytes at an aligned stride take the per-observation kernel: a different
    summation (the results differ somewhere), conv2 / conv3 unchanged bit for bit."""
    from agent0_amd._abi import A0Error
    shape, B = G84, 300
    net, L, params = _net(hip, shape)
    C, H, W = shape
    ob = C * H * W
    (H1, W1), (H2, W2), (H3, W3) = _geo(shape)
    n1, n2, n3 = B * H1 * W1 * 32, B * H2 * W2 * 64, B * H3 * W3 * 64
    K1 = C * 64
    obs_np = recipe.make_frames(B, 17, shape)[:, :C].reshape(B, ob)
    odd = 2 * ob + 2
    assert odd % 4 != 0
    rows = np.zeros((B, odd), np.uint8)
    rows[:, :ob] = obs_np
    frames_odd = torch.from_numpy(rows.reshape(-1)).to(hip.device)
    frames_al = torch.from_numpy(np.ascontiguousarray(obs_np).reshape(-1)).to(hip.device)
    act1, act2, act3 = (hip.empty(n) for n in (n1, n2, n3))
    with pytest.raises(A0Error):
        hip.encoder_fwd_fused(net.net, net.wt, net.encoder_weights(), frames_odd, None, odd, 0, B, act1, act2, act3)
    hip.encoder_fwd(net.net, net.encoder_weights(), frames_odd, None, odd, 0, B, act1, act2, act3)
    d3 = (torch.from_numpy(recipe.gen(18).standard_normal(n3).astype(np.float32)).to(hip.device) * (act3 > 0)).contiguous()
    d2, d1 = hip.empty(n2), hip.empty(n1)
    hip.encoder_dgrad_fused(net.net, net.wt, d3, act1, act2, B, d2, d1)
    need = hip.encoder_bwd_scratch(net.net, B)
    ng = (32 * K1 + 32, 64 * 512 + 64, 64 * 576 + 64)
    res = {}
    for name, frames, stride in (("unaligned", frames_odd, odd), ("aligned", frames_al, ob)):
        gs = [_guarded(hip, n) for n in ng]
        slabs = _guarded(hip, need)
        hip.encoder_wgrad(net.net, net.encoder_weights(), frames, None, stride, 0, B, act1, act2, d3, d2, d1, *gs, slabs)
        torch.cuda.synchronize()
        for gbuf, n, k in zip(gs, ng, ("g1", "g2", "g3")):
            _check_guard(gbuf, n, f"{name} {k}")
        _check_guard(slabs, need, f"{name} slabs", written=False)
        res[name] = [gbuf[:n].clone() for gbuf, n in zip(gs, ng)]
    x = torch.from_numpy(obs_np.reshape(B, C, H, W).astype(np.float64)) / 255.0
    dw, db, sw, sb = conv_wgrad64(x, nchw_from_nhwc(d1, B, H1, W1, 32), params[0][0].shape, 4)
    for name, g in res.items():
        _check(conv_w_from_kernel(g[0][:32 * K1], 0, C), dw, sw, f"{name} conv1.weight")
        _check(g[0][32 * K1:].double(), db, sb, f"{name} conv1.bias")
    assert not torch.equal(res["unaligned"][0], res["aligned"][0]), "the unaligned stride takes a different conv1 kernel"
    assert torch.equal(res["unaligned"][1], res["aligned"][1]) and torch.equal(res["unaligned"][2], res["aligned"][2])


@pytest.mark.parametrize("B", [72, 73, 256, 257])
def test_the_fused_kernels_are_the_ones_that_run(hip, B):
    """The launches the tests above compare are the per-observation kernels where their plans accept the shape (84 x 84), counted by the timing probe
    in calls of their own (an active probe changes the dense kernels' selection, not these): the fused forward and its multi-pass form (tag
    encoder_fused), the fused data gradient (encoder_dgrad_fused), conv23_wgrad.hip in encoder_wgrad (tag conv2_wgrad, with no conv3_wgrad GEMM beside it;
    encoder_bwd launches that GEMM)."""
    shape = G84
    net, L, _ = _net(hip, shape)
    C, H, W = shape
    ob = C * H * W
    (H1, W1), (H2, W2), (H3, W3) = _geo(shape)
    n1, n2, n3 = B * H1 * W1 * 32, B * H2 * W2 * 64, B * H3 * W3 * 64
    frames = torch.from_numpy(recipe.make_frames(B, 23, shape).reshape(-1)).to(hip.device)
    act1, act2, act3 = (hip.empty(n) for n in (n1, n2, n3))
    d2, d1 = hip.empty(n2), hip.empty(n1)
    g1, g2, g3 = hip.empty(32 * 256 + 32), hip.empty(64 * 512 + 64), hip.empty(64 * 576 + 64)
    slabs = hip.empty(max(hip.encoder_bwd_scratch(net.net, B), 4))

    def count(tag, fn):
        torch.cuda.synchronize()
        hip.probe_begin(tag, 8)
        try:
            fn()
        finally:
            out = hip.probe_end()
        return out["launches"]

    fwd = lambda: hip.encoder_fwd_fused(net.net, net.wt, net.encoder_weights(), frames, None, 2 * ob, 0, B, act1, act2, act3)
    multi = lambda: hip.encoder_fwd_fused_multi(net.net, [(net.wt, net.encoder_weights(), frames, None, 2 * ob, o, B, None, None, act3) for o in (0, ob)])
    assert count("encoder_fused", fwd) == 1
    assert count("encoder_fused", multi) == 1
    d3 = (torch.randn(n3, device=hip.device) * (act3 > 0)).contiguous()
    assert count("encoder_dgrad_fused", lambda: hip.encoder_dgrad_fused(net.net, net.wt, d3, act1, act2, B, d2, d1)) == 1
    wgrad = lambda: hip.encoder_wgrad(net.net, net.encoder_weights(), frames, None, 2 * ob, 0, B, act1, act2, d3, d2, d1, g1, g2, g3, slabs)
    bwd = lambda: hip.encoder_bwd(net.net, net.encoder_weights(), frames, None, 2 * ob, 0, B, act1, act2, d3, d2, d1, g1, g2, g3, slabs)
    assert count("conv2_wgrad", wgrad) == 1 and count("conv3_wgrad", wgrad) == 0
    assert count("conv3_wgrad", bwd) == 1
    assert count("conv1_wgrad", wgrad) == 1


# ------------------------------------------------------------------------------------------------ 4. merged actor step
def _terminal_step(env_seed, E):
    from oracle import core
    term = core.env_terminals(env_seed, 0, E, 20000)
    rows = np.nonzero(term.any(1))[0]
    assert rows.size, "no terminal step found"
    return int(rows[0]) + 1, term[rows[0]]


@pytest.mark.parametrize("E", [1, 5, 256, 300])
@pytest.mark.parametrize("kind", ["qhead", "dist", "quantile"])
def test_actor_step_encoder_against_float64(hip, kind, E):
    """One step of a0_actor_{qhead,dist_tail,quantile_tail}_env_step_enc at an env step g where at least one env terminates: act3_next against the float64
    three-layer encoder of the step's obs_out, per element at 3e-6 of act3's scale (the layers' |w| propagated from |x|, tests/util.py encoder_chain64),
    and against encoder_fwd_fused on the same bytes within 2e-6 of conv3's own scale on that pass's act2 (case 1's bound).  obs_out and act3_next are guarded; terminal envs' new observations are four copies of
    the new frame.  The action / Q half is the rollout parity tests' (test_gpu_trainer.py)."""
    net, L, params = _net(hip, G84)
    ob, K, A = 4 * 84 * 84, 3136, 4
    env_seed = 4321
    gstep, term = _terminal_step(env_seed, E)
    rg = recipe.gen(500 + E)
    obs_in_np = rg.integers(0, 256, (E, 4, 84, 84), dtype=np.uint8)
    obs_in_np[0, :, :3] = 0
    obs_in_np[-1, :, 40:43] = 255
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)
    obs_in = dev(obs_in_np.reshape(-1))
    obs_out = _guarded(hip, E * ob, torch.uint8)
    act3 = _guarded(hip, E * K)
    zeros = lambda n, dt=torch.float32: hip.zeros(n, dtype=dt)
    action, qmax = zeros(E, torch.int32), zeros(E)
    cap = E
    env = (env_seed, 0, gstep, obs_in, obs_out, zeros(E), zeros(E), zeros(E), 1, 0, 0.99, zeros(E, torch.int32), zeros(E), zeros(E), obs_in,
           zeros(cap * 8 * 84 * 84, torch.uint8), cap, 0, zeros(cap, torch.int32), zeros(cap), zeros(cap))
    rng = (7, 1, 2, 0, 0, 0.3, action, qmax, None, None)
    enc = dict(task=0, wt=net.wt, enc_w=net.encoder_weights(), act3_next=act3)

    def step():
        if kind == "qhead":
            feat = dev(np.maximum(rg.standard_normal((E, K)), 0).astype(np.float32).reshape(-1))
            W1 = dev((rg.standard_normal((512, K)) * 0.02).astype(np.float32).reshape(-1))
            b1, W2, b2 = dev(rg.standard_normal(512).astype(np.float32)), dev((rg.standard_normal((A, 512)) * 0.05).astype(np.float32).reshape(-1)), zeros(A)
            hip.actor_qhead_env_step_enc(feat, E, K, W1, b1, W2, b2, A, False, hip.empty(max(hip.actor_qhead_scratch(E, K), 4)), *rng, *env, **enc)
        elif kind == "dist":
            T = 51
            ld = A * T
            slabs = dev(rg.standard_normal(E * ld).astype(np.float32))
            atoms = dev(np.linspace(-10, 10, T, dtype=np.float32))
            hip.actor_dist_tail_env_step_enc(slabs, 1, zeros(ld), ld, A, T, False, 2, atoms, E, *rng, *env, **enc)
        else:
            T, ld = 32, 32
            slabs = dev(rg.standard_normal(E * T * ld).astype(np.float32))
            hip.actor_quantile_tail_env_step_enc(slabs, 1, zeros(ld), ld, A, T, False, 1, None, E, *rng, *env, **enc)

    step()
    torch.cuda.synchronize()
    _check_guard(obs_out, E * ob, "obs_out")
    _check_guard(act3, E * K, "act3_next")
    out_np = obs_out[:E * ob].cpu().numpy().reshape(E, 4, 84, 84)
    for e in np.nonzero(term)[0]:
        assert all(np.array_equal(out_np[e, c], out_np[e, 3]) for c in range(3)), f"terminal env {e}: a fresh observation"
    chain = encoder_chain64(torch.from_numpy(out_np.astype(np.float64)) / 255.0, params)
    want, scale = chain[2]
    got = nchw_from_nhwc(act3[:E * K], E, 7, 7, 64)
    err = _check(got, want, scale, f"{kind} act3_next E={E}", tol=3e-6)
    ref1, ref2, ref = hip.empty(E * 400 * 32), hip.empty(E * 81 * 64), hip.empty(E * K)
    hip.encoder_fwd_fused(net.net, net.wt, net.encoder_weights(), obs_out, None, ob, 0, E, ref1, ref2, ref)
    _, scale3 = conv_fwd64(nchw_from_nhwc(ref2, E, 9, 9, 64), *params[2], 1)        # conv3's own scale on the fused pass's act2: case 1's bound
    cross = _check(got, nchw_from_nhwc(ref, E, 7, 7, 64), scale3, f"{kind} act3_next vs encoder_fwd_fused E={E}")
    # the probe sees the merged step's kernel under its own tag (a call of its own)
    torch.cuda.synchronize()
    hip.probe_begin("actor_step_enc", 8)
    try:
        step()
    finally:
        launches = hip.probe_end()["launches"]
    assert launches == 1
    record_stats(f"conv_actor_step_{kind}_E{E}", {"act3_vs_fp64": float(np.abs(err).max()), "act3_vs_fused": float(np.abs(cross).max()),
                                                  "terminal_envs": int(term.sum())})
