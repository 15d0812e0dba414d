"""GPU (MI355X): the tile of the fc1 backward launches (a0_dense_dgrad_wgrad: the pair kernel, a0_dense_dgrad_wgrad2: the trio kernel) at the smallest shapes of their
class, R == N >= 512 with at least 256 tiles of 64 x 64: whole tiles, a ragged last column tile with a K that is no multiple of the tile, a ragged last row tile.

The single-problem paths a0_dense_dgrad and a0_dense_wgrad run other tiles (64 x 64 on four waves) and are the reference: every output element of the one launch
is the same k-ascending sequence of MFMAs, and the bias gradient the same 16 partial sums added in the same order, so dX and the [W | b] block are compared with
torch.equal.  The head's weight gradient is an unsplit sum where a0_dense_wgrad sums slabs: both are held against an fp64 product."""
import numpy as np
import pytest
import torch

import recipe
from agent0_amd._abi import A0Error

pytestmark = pytest.mark.gpu

SHAPES = [(512, 512, 2048), (512, 512, 2052), (516, 516, 2048)]
K2 = 512


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    return HipOps()


def D(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


_cases = {}


def case(hip, shape):
    """Inputs of one shape and the two single-problem results, computed once and left unchanged."""
    if shape not in _cases:
        R, N, K = shape
        g = recipe.gen(1700 + R + K)
        dY = D(hip, g.standard_normal((R, N)).astype(np.float32))
        W = D(hip, (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
        X = D(hip, np.maximum(g.standard_normal((R, K)), 0).astype(np.float32))
        X2n = np.maximum(g.standard_normal((R, K2)), 0).astype(np.float32)
        dX0, g0 = hip.empty(R * K).fill_(float("nan")), hip.empty(N * K + N).fill_(float("nan"))
        hip.dense_dgrad(dY, W, X, dX0, R, N, K)
        hip.dense_wgrad(dY, X, K, g0, R, N, K, hip.empty(max(hip.dense_wgrad_scratch(R, N, K), 4)))
        # the single-problem data gradient shares the GEMM body's masked epilogue with the launches under test, so the reference itself is held against
        # (dY W) * (X > 0) in fp64: an fp32 chain over N = 512 terms is off by about sqrt(N) 2^-24 = 1.4e-6 of the scale; 2e-5 leaves a factor of 14, and a value
        # masked, or passed, in the wrong place is off by the order of the scale
        want = (dY.double() @ W.double()) * (X > 0)
        err, scale = float((dX0.view(R, K).double() - want).abs().max()), float(want.abs().max())
        print(f"{shape}: dX of a0_dense_dgrad against fp64 (dY W) * (X > 0): {err:.3e}, scale {scale:.3e}")
        assert err < 2e-5 * scale, f"a0_dense_dgrad {err} against fp64, scale {scale}"
        _cases[shape] = (dY, W, X, X2n, dX0, g0)
    return _cases[shape]


def check_fc1(shape, X, dX0, g0, dX1, g1):
    R, N, K = shape
    assert torch.isfinite(dX1).all() and torch.isfinite(g1).all(), "an unwritten tile"
    assert torch.equal(dX0, dX1), "dX against a0_dense_dgrad"
    assert torch.equal(g0[: N * K], g1[: N * K]), "dW against a0_dense_wgrad"
    assert torch.equal(g0[N * K:], g1[N * K:]), "db (the row sums) against a0_dense_wgrad"
    assert float(dX1.view(R, K)[X.view(R, K) <= 0].abs().max()) == 0.0, "the ReLU mask"


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_launch_equals_the_single_problem_paths(hip, shape):
    R, N, K = shape
    assert hip.dense_dgrad_wgrad_ok(R, N, K)
    dY, W, X, _, dX0, g0 = case(hip, shape)
    dX1, g1 = hip.empty(R * K).fill_(float("nan")), hip.empty(N * K + N).fill_(float("nan"))
    hip.dense_dgrad_wgrad(dY, W, X, K, dX1, g1, R, N, K)
    check_fc1(shape, X, dX0, g0, dX1, g1)


@pytest.mark.parametrize("N2", [4, 24, 52])
@pytest.mark.parametrize("shape", SHAPES)
def test_trio_launch_equals_the_single_problem_paths(hip, shape, N2):
    R, N, K = shape
    assert hip.dense_dgrad_wgrad2_ok(R, N, K, N2, K2)
    dY, W, X, X2n, dX0, g0 = case(hip, shape)
    dY2n = recipe.gen(N2).standard_normal((R, N2)).astype(np.float32)
    dY2, X2 = D(hip, dY2n), D(hip, X2n)
    dX1, g1 = hip.empty(R * K).fill_(float("nan")), hip.empty(N * K + N).fill_(float("nan"))
    h0, h1 = hip.empty(N2 * K2 + N2).fill_(float("nan")), hip.empty(N2 * K2 + N2).fill_(float("nan"))
    hip.dense_wgrad(dY2, X2, K2, h0, R, N2, K2, hip.empty(max(hip.dense_wgrad_scratch(R, N2, K2), 4)))
    hip.dense_dgrad_wgrad2(dY, W, X, K, dX1, g1, R, N, K, dY2, X2, K2, h1, N2, K2)
    check_fc1(shape, X, dX0, g0, dX1, g1)
    assert torch.isfinite(h1).all(), "an unwritten tile of the head's gradient"
    ref = np.concatenate([(dY2n.astype(np.float64).T @ X2n.astype(np.float64)).reshape(-1), dY2n.astype(np.float64).sum(0)])
    scale = np.abs(ref).max()
    e_ref, e_new = np.abs(h0.cpu().numpy() - ref).max() / scale, np.abs(h1.cpu().numpy() - ref).max() / scale
    print(f"head weight gradient, {shape}, N2 = {N2}: {e_new:.3e} of the scale against fp64 (a0_dense_wgrad: {e_ref:.3e})")
    assert e_new < 4 * e_ref + 2e-7, f"head weight gradient {e_new} of the scale against fp64 (a0_dense_wgrad: {e_ref})"


def test_shapes_outside_the_class_are_refused(hip):
    K = 2048
    for R, N, Kx in [(256, 256, K), (256, 512, K), (512, 256, K), (512, 512, 1984), (512, 512, K + 2), (514, 514, K), (1028, 1028, K)]:
        assert not hip.dense_dgrad_wgrad_ok(R, N, Kx), (R, N, Kx)
        assert not hip.dense_dgrad_wgrad2_ok(R, N, Kx, 4, K2), (R, N, Kx)
    for N2, K2x in [(256, K2), (4, 1024), (6, K2), (4, 510)]:
        assert not hip.dense_dgrad_wgrad2_ok(512, 512, K, N2, K2x), (N2, K2x)
    R = N = 256
    bufs = [hip.zeros(n) for n in (R * N, N * K, R * K, R * K, N * K + N, R * 4, R * K2, 4 * K2 + 4)]
    dY, W, X, dX, grad, dY2, X2, grad2 = bufs
    with pytest.raises(A0Error):
        hip.dense_dgrad_wgrad2(dY, W, X, K, dX, grad, R, N, K, dY2, X2, K2, grad2, 4, K2)
