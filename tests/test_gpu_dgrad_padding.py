"""GPU (MI355X): the fused data gradient (a0_net_encoder_dgrad_fused: a0_encoder_dgrad_fused_x9_kernel) where it leaves work out and where it runs ahead.

The kernel computes both gradients as gather convolutions over zero-padded LDS images and does not issue the (row block, tap) pairs that read nothing but
the padding; a workgroup with a second observation (B > 256: gridx = min(B, 256)) stages that observation's d3 while the first one's conv2 stages run.

1. One-hot d3 (a single 1.0): every product that is formed is an exact weight term, so d2 must be conv3's weights at the 3 x 3 footprint bit for bit and zero
   elsewhere — a (block, tap) pair left out by mistake removes a whole weight.  One case per class of d3 pixel; the corners' footprints reach d2 rows and
   columns 0 and 8, which is where conv2's stages leave pairs out, so d1 of the same launch is held to float64.
2. Dense d3 under random masks, B = 1, 2, 3, against float64; once with masks that pass everything.
3. B = 257 and 258: every observation bit for bit what a launch of its own gives, twice into the same buffers with other inputs the second time.

Reference and bound are those of test_gpu_conv_reference.py (imported): the float64 conv-transpose of the launch's own inputs (d1: of the launch's own d2), the
error of every element divided by its accumulated magnitude, 2e-6; where the magnitude is zero the element must be exactly zero.  d2 and d1 are prefilled
with NaN and sit between sentinels.  Cases 2 and 3 run under both product forms (a0_x9_products 6 and 9)."""
import numpy as np
import pytest
import torch

import recipe
from test_gpu_conv_reference import G84, TOL, _check, _check_guard, _guarded, _net, hip  # noqa: F401  (hip: the module-scoped fixture)
from util import conv_dgrad64, nchw_from_nhwc

pytestmark = pytest.mark.gpu

N3, N2, N1 = 49 * 64, 81 * 64, 400 * 32


@pytest.fixture(params=[6, 9], ids=["six", "nine"])
def products(request, hip):
    prev = hip.x9_products()
    hip.x9_products(request.param)
    yield request.param
    hip.x9_products(prev)


def _dev(hip, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)


def _launch(hip, d3, act1, act2, B):
    """-> (d2, d1) of one launch, as flat device tensors of B observations; guards checked."""
    net = _net(hip, G84)[0]
    d2, d1 = _guarded(hip, B * N2), _guarded(hip, B * N1)
    hip.encoder_dgrad_fused(net.net, net.wt, d3, act1, act2, B, d2, d1)
    torch.cuda.synchronize()
    _check_guard(d2, B * N2, f"d2 B={B}")
    _check_guard(d1, B * N1, f"d1 B={B}")
    return d2[:B * N2], d1[:B * N1]


def _against_float64(hip, d3, act1, act2, d2, d1, B, what):
    """d2 against the conv-transpose of d3, d1 against that of the launch's own d2, both masked, at TOL of the accumulated magnitude; prints the figures."""
    params = _net(hip, G84)[2]
    m2, m1 = nchw_from_nhwc(act2, B, 9, 9, 64) > 0, nchw_from_nhwc(act1, B, 20, 20, 32) > 0
    g2, g1 = nchw_from_nhwc(d2, B, 9, 9, 64), nchw_from_nhwc(d1, B, 20, 20, 32)
    assert bool((g2[~m2] == 0).all()) and bool((g1[~m1] == 0).all()), f"{what}: nonzero where the mask is closed"
    want2, scale2 = conv_dgrad64(nchw_from_nhwc(d3, B, 7, 7, 64), params[2][0], 1, (B, 64, 9, 9), m2)
    want1, scale1 = conv_dgrad64(g2, params[1][0], 2, (B, 32, 20, 20), m1)
    for name, got, want, scale in (("d2", g2, want2, scale2), ("d1", g1, want1, scale1)):
        err = (got - want).abs() / scale.clamp_min(1e-30)
        print(f"{what} {name}: {float(err.max()):.3e} of the accumulated magnitude (bound {TOL:g})")
    _check(g2, want2, scale2, f"{what} d2")
    _check(g1, want1, scale1, f"{what} d1")


# ------------------------------------------------------------------------------------------------ 1. every tap of every border position
# (h, w, channel) of the one-hot: four corners, four edge midpoints, the centre; the tenth is (6, 6) again — the only d3 pixel the lone position (8, 8) of
# conv3's last row block reads — in the other half of the channels, so that block's one live tap is exercised in both waves that share its k steps
ONE_HOT = [(0, 0, 5), (0, 6, 40), (6, 0, 63), (6, 6, 0), (0, 3, 31), (3, 0, 32), (6, 3, 17), (3, 6, 58), (3, 3, 9), (6, 6, 47)]


@pytest.mark.parametrize("h,w,c", ONE_HOT)
def test_one_hot_d3_gives_the_weights_exactly(hip, h, w, c):
    net, _, params = _net(hip, G84)
    d3 = torch.zeros(N3, device=hip.device)
    d3[(h * 7 + w) * 64 + c] = 1.0
    act2, act1 = torch.ones(N2, device=hip.device), torch.ones(N1, device=hip.device)
    d2, d1 = _launch(hip, d3, act1, act2, 1)
    w3 = params[2][0].to(torch.float32)                     # [co][ci][kh][kw], the state_dict's fp32 values
    want = torch.zeros(9, 9, 64)
    want[h:h + 3, w:w + 3, :] = w3[c].permute(1, 2, 0)       # d2[h + kh][w + kw][ci] = W3[c][ci][kh][kw]
    got = d2.cpu().view(9, 9, 64)
    if not torch.equal(got, want):
        bad = (got != want).any(-1).nonzero().tolist()
        raise AssertionError(f"one-hot d3 ({h}, {w}, channel {c}): d2 differs from conv3's weights at positions {bad}")
    _against_float64(hip, d3, act1, act2, d2, d1, 1, f"one-hot ({h}, {w}, {c})")


# ------------------------------------------------------------------------------------------------ 2. dense
def _dense_inputs(hip, B, seed, open_masks=False):
    g = recipe.gen(seed)
    d3 = g.standard_normal(B * N3).astype(np.float32)
    d3[d3 == 0] = 1.0                                       # nonzero everywhere
    if open_masks:
        act1, act2 = np.ones(B * N1, np.float32), np.ones(B * N2, np.float32)
    else:                                                   # + / - at random: about half of the masks closed
        act1, act2 = g.standard_normal(B * N1).astype(np.float32), g.standard_normal(B * N2).astype(np.float32)
    return _dev(hip, d3), _dev(hip, act1), _dev(hip, act2)


@pytest.mark.parametrize("B,open_masks", [(1, False), (2, False), (3, False), (2, True)])
def test_dense_d3_against_float64(hip, products, B, open_masks):
    d3, act1, act2 = _dense_inputs(hip, B, 900 + B + 10 * open_masks, open_masks)
    d2, d1 = _launch(hip, d3, act1, act2, B)
    _against_float64(hip, d3, act1, act2, d2, d1, B, f"dense B={B} masks {'open' if open_masks else 'random'} products={products}")


# ------------------------------------------------------------------------------------------------ 3. the loop and the early staging
_SINGLE = {}


def _singles(hip, products):
    """258 observations, all different, and each one's d2 / d1 from a launch of its own (B = 1): computed once per product form."""
    if products not in _SINGLE:
        net = _net(hip, G84)[0]
        d3, act1, act2 = _dense_inputs(hip, 258, 77)
        r2, r1 = hip.empty(258 * N2), hip.empty(258 * N1)
        r2.fill_(float("nan")); r1.fill_(float("nan"))
        for b in range(258):
            hip.encoder_dgrad_fused(net.net, net.wt, d3[b * N3:(b + 1) * N3], act1[b * N1:(b + 1) * N1], act2[b * N2:(b + 1) * N2], 1,
                                    r2[b * N2:(b + 1) * N2], r1[b * N1:(b + 1) * N1])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(r2).all()) and bool(torch.isfinite(r1).all())
        _SINGLE[products] = (d3, act1, act2, r2, r1)
    return _SINGLE[products]


@pytest.mark.parametrize("B", [257, 258])
def test_second_observation_of_a_workgroup(hip, products, B):
    """gridx = 256: at B = 257 one workgroup walks two observations, at 258 two do, the others one.  Second launch: the same buffers, every observation
    moved one slot up (slot b holds observation b + 1), so each workgroup's d3 planes must be rewritten in full."""
    net = _net(hip, G84)[0]
    d3, act1, act2, r2, r1 = _singles(hip, products)
    d2, d1 = _guarded(hip, B * N2), _guarded(hip, B * N1)
    for shift in (0, 1):
        sl = lambda t, n: (t[shift * n:(shift + B) * n] if shift + B <= 258 else torch.cat([t[shift * n:], t[:(shift + B - 258) * n]])).contiguous()
        hip.encoder_dgrad_fused(net.net, net.wt, sl(d3, N3), sl(act1, N1), sl(act2, N2), B, d2, d1)
        torch.cuda.synchronize()
        _check_guard(d2, B * N2, f"d2 B={B} launch {shift}")
        _check_guard(d1, B * N1, f"d1 B={B} launch {shift}")
        for name, got, ref, n in (("d2", d2[:B * N2], sl(r2, N2), N2), ("d1", d1[:B * N1], sl(r1, N1), N1)):
            if not torch.equal(got, ref):
                bad = (got.view(B, n) != ref.view(B, n)).any(1).nonzero().flatten().tolist()
                raise AssertionError(f"B={B} products={products} launch {shift}: {name} of observations {bad} differs from a launch of their own")
