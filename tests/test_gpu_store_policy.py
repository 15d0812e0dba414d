"""GPU (MI355X): the kernels whose bulk outputs take, or were measured for, a cache policy (agent0_amd/csrc/store_policy.h), at the edges a store form can get wrong: a replay row
beyond byte 2^32 of the ring and rows that straddle its wrap, activation blocks of single observations with guard bands on both sides, output buffers 4 and 16
bytes into their allocation, a parameter count that is no multiple of four.  A policy changes neither a value nor an address, so every comparison is on bit
patterns against a second path of the library that forms the same numbers (the data gradient, which has none, at test_gpu_engine.py's tolerance); nothing here
depends on which policy a site was built with."""
import numpy as np
import pytest
import torch

import recipe
from agent0_amd._abi import A0Error

pytestmark = pytest.mark.gpu

OB = 4 * 84 * 84
GUARD = 64                       # floats (256 bytes) on each side of an output
SENT = -12345.0


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


@pytest.fixture(scope="module")
def net(hip):
    from agent0_amd.deepq.engine import DeviceNet
    from agent0_amd.deepq.layout import NetLayout
    spec = recipe.NetSpec("dqn", 4)
    L = NetLayout.from_spec(spec)
    n = DeviceNet(hip, L, hip.net(4, 84, 84))
    n.load_state_dict(recipe.make_state_dict(spec, 11))
    return n, L


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _banded(hip, n, lead=0):
    """NaN where the kernel writes, sentinels on both sides; ``lead`` more floats in front shift the output inside its allocation.  -> (whole buffer, the output)"""
    buf = hip.empty(GUARD + lead + n + GUARD)
    buf.fill_(SENT)
    out = buf[GUARD + lead:GUARD + lead + n]
    out.fill_(float("nan"))
    return buf, out


def _bands_intact(buf, n, what, lead=0):
    assert bool((buf[:GUARD + lead] == SENT).all()), f"{what}: write in front of the output"
    assert bool((buf[GUARD + lead + n:] == SENT).all()), f"{what}: write past the end of the output"
    assert not bool(torch.isnan(buf[GUARD + lead:GUARD + lead + n]).any()), f"{what}: unwritten elements"


# ------------------------------------------------------------------------------------------------ 1. actor step: replay rows beyond 2^32 bytes, rows across the wrap
CAP = 80000                      # 80 000 rows of 56 448 bytes: 4.5 GB, allocated and never filled


@pytest.fixture(scope="module")
def big_ring(hip):
    return torch.empty(CAP * 2 * OB, dtype=torch.uint8, device=hip.device)


@pytest.mark.parametrize("start", [76100, CAP - 2], ids=["above-2^32", "wrap"])
def test_actor_step_rows_in_a_large_ring(hip, net, big_ring, start):
    """The scalar-head step with the next encoder (one launch behind fc1) against a0_actor_qhead_env_step followed by the encoder on its own: the three envs' replay
    rows, their new stacks, actions, statistics and the next step's features.  Rows next to the written ones keep their sentinel bytes."""
    dn, _ = net
    E, K, A = 3, 3136, 4
    slots = [(start + e) % CAP for e in range(E)]
    if start == 76100:
        assert min(slots) * 2 * OB > 2 ** 32
    near = sorted({(s + d) % CAP for s in slots for d in (-1, 0, 1)})
    rg = recipe.gen(900 + start)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)
    obs_in = dev(rg.integers(0, 256, E * OB, dtype=np.uint8))
    feat = dev(np.maximum(rg.standard_normal(E * K), 0).astype(np.float32))
    W1, b1 = dev((rg.standard_normal(512 * K) * 0.02).astype(np.float32)), dev(rg.standard_normal(512).astype(np.float32))
    W2, b2 = dev((rg.standard_normal(A * 512) * 0.05).astype(np.float32)), dev(rg.standard_normal(A).astype(np.float32))
    rows = big_ring.view(CAP, 2 * OB)
    got = {}
    for kind in ("merged", "pair"):
        z = lambda n, dt=torch.float32: hip.zeros(n, dtype=dt)
        for s in near:
            rows[s].fill_(0xA5)
        obs_out = torch.full((GUARD + E * OB + GUARD,), 0xA5, dtype=torch.uint8, device=hip.device)
        stack = obs_out[GUARD:GUARD + E * OB]
        abuf, act3 = _banded(hip, E * K)
        action, qmax = z(E, torch.int32), z(E)
        stats = [z(E), z(E), z(E)]
        rep = [z(CAP, torch.int32), z(CAP), z(CAP)]
        env = (4321, 0, 17, obs_in, stack, *stats, 1, 0, 0.99, z(E, torch.int32), z(E), z(E), obs_in, big_ring, CAP, start, *rep)
        args = (feat, E, K, W1, b1, W2, b2, A, False, hip.empty(max(hip.actor_qhead_scratch(E, K), 4)), 7, 1, 2, 0, 0, 0.3, action, qmax, None, None)
        if kind == "merged":
            hip.actor_qhead_env_step_enc(*args, *env, task=0, wt=dn.wt, enc_w=dn.encoder_weights(), act3_next=act3)
        else:
            hip.actor_qhead_env_step(*args, *env, task=0)
            hip.encoder_fwd_fused(dn.net, dn.wt, dn.encoder_weights(), stack, None, OB, 0, E, None, None, act3)
        torch.cuda.synchronize()
        _bands_intact(abuf, E * K, f"{kind}: act3")
        assert bool((obs_out[:GUARD] == 0xA5).all()) and bool((obs_out[GUARD + E * OB:] == 0xA5).all()), f"{kind}: write outside the stacks"
        for s in near:
            if s not in slots:
                assert bool((rows[s] == 0xA5).all()), f"{kind}: row {s} next to the step's rows was written"
        got[kind] = dict(rows=torch.stack([rows[s].clone() for s in slots]), stack=stack.clone(), act3=act3.clone(), action=action, qmax=qmax,
                         **{f"stat{i}": t for i, t in enumerate(stats)}, **{f"rep{i}": t for i, t in enumerate(rep)})
    for e, s in enumerate(slots):
        r = got["merged"]["rows"][e]
        assert torch.equal(r[:OB], obs_in[e * OB:(e + 1) * OB]), f"row {s}: st is the env's observation before the step"
        assert torch.equal(r[OB:], got["merged"]["stack"][e * OB:(e + 1) * OB]), f"row {s}: st_next is the env's new stack"
    for k in got["merged"]:
        assert torch.equal(_bits(got["merged"][k]), _bits(got["pair"][k])), f"{k}: merged step against the two launches"


# ------------------------------------------------------------------------------------------------ 2. encoder outputs
@pytest.mark.parametrize("npass", [2, 3])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_encoder_passes_in_one_launch(hip, net, B, npass):
    """a0_net_encoder_fwd_fused_multi on gathered replay rows against one launch per pass: act1, act2, act3 of every pass, sentinels on both sides of each."""
    dn, _ = net
    cap = B + 4
    g = torch.Generator(device="cpu").manual_seed(40 * B + npass)
    ring = torch.randint(0, 256, (cap * 2 * OB,), dtype=torch.uint8, generator=g).to(hip.device)
    sizes = (B * 400 * 32, B * 81 * 64, B * 49 * 64)
    passes, multi, single = [], [], []
    for p in range(npass):
        slot = torch.randperm(cap, generator=g)[:B].to(torch.int32).to(hip.device)
        off = OB if p == 1 else 0
        m, s = [_banded(hip, n) for n in sizes], [_banded(hip, n) for n in sizes]
        passes.append((dn.wt, dn.encoder_weights(), ring, slot, 2 * OB, off, B, *[o for _, o in m]))
        hip.encoder_fwd_fused(dn.net, dn.wt, dn.encoder_weights(), ring, slot, 2 * OB, off, B, *[o for _, o in s])
        multi.append(m)
        single.append(s)
    hip.encoder_fwd_fused_multi(dn.net, passes)
    torch.cuda.synchronize()
    for p in range(npass):
        for (mb, mo), (sb, so), n, name in zip(multi[p], single[p], sizes, ("act1", "act2", "act3")):
            _bands_intact(mb, n, f"multi pass {p} {name}")
            _bands_intact(sb, n, f"single pass {p} {name}")
            assert torch.equal(_bits(mo), _bits(so)), f"pass {p} {name}: one launch against a launch per pass"
            assert bool((mo > 0).any()), f"pass {p} {name}: all zero"


# ------------------------------------------------------------------------------------------------ 3. data gradient
@pytest.mark.parametrize("B", [1, 3, 5])
def test_fused_data_gradient(hip, net, B):
    """a0_net_encoder_dgrad_fused against the implicit-GEMM backward on the fp32 fmaf chain: same taps and masks, another order of additions, so 2e-5 of the scale
    (the bound of test_gpu_engine.py's test_fused_dgrad_matches_unfused); d2 and d1 sit between sentinels."""
    dn, _ = net
    g = recipe.gen(70 + B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)
    frames = dev(g.integers(0, 256, B * OB, dtype=np.uint8))
    n1, n2, n3 = B * 400 * 32, B * 81 * 64, B * 49 * 64
    act1, act2, act3 = hip.empty(n1), hip.empty(n2), hip.empty(n3)
    hip.encoder_fwd_fused(dn.net, dn.wt, dn.encoder_weights(), frames, None, OB, 0, B, act1, act2, act3)
    d3 = (dev(g.standard_normal(n3).astype(np.float32)) * (act3 > 0)).contiguous()
    r2, r1 = hip.empty(n2), hip.empty(n1)
    grads = [hip.empty(32 * 256 + 32), hip.empty(64 * 512 + 64), hip.empty(64 * 576 + 64)]
    prev = hip.gemm_mode(0)
    try:
        hip.encoder_bwd(dn.net, dn.encoder_weights(), frames, None, OB, 0, B, act1, act2, d3, r2, r1, *grads, hip.empty(max(hip.encoder_bwd_scratch(dn.net, B), 4)))
    finally:
        hip.gemm_mode(prev)
    (b2, d2), (b1, d1) = _banded(hip, n2), _banded(hip, n1)
    hip.encoder_dgrad_fused(dn.net, dn.wt, d3, act1, act2, B, d2, d1)
    torch.cuda.synchronize()
    _bands_intact(b2, n2, "d2")
    _bands_intact(b1, n1, "d1")
    for name, got, ref, mask in (("d2", d2, r2, act2), ("d1", d1, r1, act1)):
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        print(f"B={B} {name}: {err:.3e} against the fp32 chain, scale {scale:.3e}")
        assert scale > 0 and err <= 2e-5 * scale, (name, B, err, scale)
        assert float(got[mask <= 0].abs().max()) == 0.0, f"{name}: the ReLU mask"


# ------------------------------------------------------------------------------------------------ 4. GEMM epilogues into outputs 4 and 16 bytes inside their allocation
FC1_SHAPES = [(512, 512, 2048), (512, 512, 2052), (516, 516, 2048)]
_fc1 = {}


def _fc1_case(hip, shape):
    if shape not in _fc1:
        R, N, K = shape
        g = recipe.gen(1700 + R + K)
        D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
        dY = D(g.standard_normal((R, N)).astype(np.float32))
        W = D((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
        X = D(np.maximum(g.standard_normal((R, K)), 0).astype(np.float32))
        dX0, g0 = hip.empty(R * K).fill_(float("nan")), hip.empty(N * K + N).fill_(float("nan"))
        hip.dense_dgrad_wgrad(dY, W, X, K, dX0, g0, R, N, K)
        torch.cuda.synchronize()
        assert torch.isfinite(dX0).all() and torch.isfinite(g0).all()
        _fc1[shape] = (dY, W, X, dX0, g0)
    return _fc1[shape]


def _run_or_refused(call, bands, what):
    """An output that is not 16-byte aligned either works or is refused with a status code; refused, nothing was written."""
    try:
        call()
    except A0Error:
        torch.cuda.synchronize()
        for buf, n, lead in bands:
            assert bool((buf[:GUARD + lead] == SENT).all()) and bool((buf[GUARD + lead + n:] == SENT).all()), f"{what}: refused, but wrote outside the output"
            assert bool(torch.isnan(buf[GUARD + lead:GUARD + lead + n]).all()), f"{what}: refused, but wrote"
        return False
    torch.cuda.synchronize()
    for buf, n, lead in bands:
        _bands_intact(buf, n, what, lead)
    return True


@pytest.mark.parametrize("lead", [1, 4], ids=["4-bytes", "16-bytes"])
@pytest.mark.parametrize("shape", FC1_SHAPES)
def test_fc1_backward_outputs_inside_their_allocation(hip, shape, lead):
    """The pair and the trio launch of fc1's backward (masked data gradient, [W | b] weight-gradient block) with dX and the block `lead` floats into their buffers,
    against the pair launch on aligned outputs."""
    R, N, K = shape
    dY, W, X, dX0, g0 = _fc1_case(hip, shape)
    (bx, dX1), (bg, g1) = _banded(hip, R * K, lead), _banded(hip, N * K + N, lead)
    if _run_or_refused(lambda: hip.dense_dgrad_wgrad(dY, W, X, K, dX1, g1, R, N, K), [(bx, R * K, lead), (bg, N * K + N, lead)], f"pair {shape} +{4 * lead} B"):
        assert torch.equal(_bits(dX0), _bits(dX1)) and torch.equal(_bits(g0), _bits(g1))
    N2, K2 = 4, 512
    gn = recipe.gen(N2)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
    dY2, X2 = D(gn.standard_normal((R, N2)).astype(np.float32)), D(np.maximum(gn.standard_normal((R, K2)), 0).astype(np.float32))
    h0 = hip.empty(N2 * K2 + N2).fill_(float("nan"))
    hip.dense_dgrad_wgrad2(dY, W, X, K, hip.empty(R * K), hip.empty(N * K + N), R, N, K, dY2, X2, K2, h0, N2, K2)
    (bx, dX2), (bg, g2), (bh, h1) = _banded(hip, R * K, lead), _banded(hip, N * K + N, lead), _banded(hip, N2 * K2 + N2, lead)
    bands = [(bx, R * K, lead), (bg, N * K + N, lead), (bh, N2 * K2 + N2, lead)]
    if _run_or_refused(lambda: hip.dense_dgrad_wgrad2(dY, W, X, K, dX2, g2, R, N, K, dY2, X2, K2, h1, N2, K2), bands, f"trio {shape} +{4 * lead} B"):
        assert torch.equal(_bits(dX0), _bits(dX2)) and torch.equal(_bits(g0), _bits(g2)) and torch.equal(_bits(h0), _bits(h1))


@pytest.mark.parametrize("lead", [1, 4], ids=["4-bytes", "16-bytes"])
@pytest.mark.parametrize("R", [1, 63, 64, 65])
def test_actor_fc1_slabs_inside_their_allocation(hip, R, lead):
    """a0_actor_fc1's slabs and the general split-K kernel's (EpiSlab), both `lead` floats into their buffers, against the general kernel on an aligned buffer."""
    N, K = 512, 3136
    g = torch.Generator(device="cpu").manual_seed(13 * R + lead)
    W = (torch.randn(N, K, generator=g) * 0.02).to(hip.device).contiguous()
    X = torch.relu(torch.randn(R, K, generator=g) - 0.5).to(hip.device).contiguous()
    planes = torch.empty(hip.actor_fc1_planes_words(N, K), dtype=torch.int32, device=hip.device)
    hip.actor_fc1_planes(W, planes, N, K)
    ns = hip.dense_fwd_partial_slabs(R, N, K)
    want = torch.full((ns * R * N,), float("nan"), device=hip.device)
    assert hip.dense_fwd_partial(X, K, W, R, N, K, want) == ns
    for name, run in (("a0_actor_fc1", lambda out: hip.actor_fc1(X, K, planes, R, N, K, out)), ("a0_dense_fwd_partial", lambda out: hip.dense_fwd_partial(X, K, W, R, N, K, out))):
        buf, out = _banded(hip, ns * R * N, lead)
        if _run_or_refused(lambda: run(out), [(buf, ns * R * N, lead)], f"{name} R={R} +{4 * lead} B"):
            assert torch.equal(_bits(out), _bits(want)), f"{name} R={R} +{4 * lead} B"


# ------------------------------------------------------------------------------------------------ 5. update tail
def _guard_behind(hip, t):
    buf = hip.empty(t.numel() + GUARD)
    buf[:t.numel()].copy_(t)
    buf[t.numel():].fill_(SENT)
    return buf, buf[:t.numel()]


@pytest.mark.parametrize("n_dense,extra", [(1701, 3), (1702, 0), (1700, 260)], ids=["n%4==1", "n%4==2", "n%4==0,n_total>n"])
def test_update_tail_against_the_folded_adam_step(hip, n_dense, extra):
    """One update through a0_net_encoder_wgrad_tail + a0_update_tail against a0_net_encoder_wgrad + a0_adam_step_sync_wt on the same bytes (the worlds and slab
    segments of test_gpu_update_tail.py), a step that also copies to the target (target_update_freq = 1): p, m, v, target and every byte of the weight copies,
    each of them with sentinels behind it."""
    from test_gpu_update_tail import _World, _pend
    shape, B, segs = (4, 84, 84), 3, [(1, "vec"), (7, "base"), (8, "vec"), (9, "count")]
    C_ = shape[0]
    net = hip.net(*shape)
    gen = recipe.gen(n_dense)
    f = lambda k: torch.from_numpy(gen.standard_normal(k).astype(np.float32)).to(hip.device)
    conv_end = 32 * 64 * C_ + 32 + 64 * 512 + 64 + 64 * 576 + 64
    n, n_total = conv_end + n_dense, conv_end + n_dense + extra
    frames = torch.from_numpy(recipe.make_frames(B, 5, shape)).to(hip.device).reshape(-1).contiguous()
    stride = frames.numel() // B
    act1, act2 = f(B * net.H1 * net.W1 * 32).abs(), f(B * net.H2 * net.W2 * 64).abs()
    d3, d2, d1 = f(B * net.feat), f(B * net.H2 * net.W2 * 64), f(B * net.H1 * net.W1 * 32)
    from test_gpu_update_tail import FORMS
    pend_slabs = f(sum((ns * FORMS[fm][2] + 3) // 4 * 4 for ns, fm in segs) + 4)
    need = hip.encoder_bwd_scratch(net, B)
    lr, b1, b2, eps, tf = 5e-4, 0.9, 0.999, 1e-2 / 32, 1
    worlds = {}
    for kind in ("folded", "tail"):
        w = _World(hip, C_, n, n_total, 77)
        bufs = {}
        for k in ("p", "t", "m", "v", "wt", "wt_t"):
            bufs[k], view = _guard_behind(hip, getattr(w, k))
            setattr(w, k, view)
        w.g.fill_(float("nan"))
        slabs = hip.empty(max(need, 4))
        o = w.off
        gs = (w.g[o[0]:o[1]], w.g[o[1]:o[2]], w.g[o[2]:w.conv_end])
        pend = _pend(w, segs, pend_slabs)
        if kind == "folded":
            hip.encoder_wgrad(net, w.weights(w.p), frames, None, stride, 0, B, act1, act2, d3, d2, d1, *gs, slabs, pend=pend)
            hip.adam_step_sync_wt(w.p, w.g, w.m, w.v, n, w.state, w.scal, lr, b1, b2, eps, tf, w.t, n_total, None, w.weights(w.p), C_, w.wt, w.wt_t)
        else:
            plan = hip.encoder_wgrad_tail(net, w.weights(w.p), frames, None, stride, 0, B, act1, act2, d3, d2, d1, *gs, slabs, pend, w.state, w.scal, lr, b1, b2, tf)
            hip.update_tail(w.p, w.g, w.m, w.v, n, w.state, w.scal, b1, b2, eps, w.t, n_total, plan, w.weights(w.p), C_, w.wt, w.wt_t)
        torch.cuda.synchronize()
        worlds[kind] = (w, bufs)
    (a, _), (b, bufs) = worlds["folded"], worlds["tail"]
    st = b.state.tolist()
    assert (st[1], st[3], st[4]) == (1, 0, 1), f"the step was taken and copied to the target: {st}"
    start = _World(hip, C_, n, n_total, 77)
    for k in ("p", "m", "v", "t", "wt", "wt_t"):
        x, y = getattr(a, k), getattr(b, k)
        assert bool((bufs[k][y.numel():] == SENT).all()), f"{k}: write past the end"
        assert torch.equal(_bits(x), _bits(y)), f"{k}: a0_update_tail against a0_adam_step_sync_wt"
    assert torch.equal(_bits(b.t), _bits(b.p)) and torch.equal(_bits(b.wt_t), _bits(b.wt))
    assert not torch.equal(_bits(b.p[:n]), _bits(start.p[:n])) and not torch.equal(_bits(b.wt), _bits(start.wt))
