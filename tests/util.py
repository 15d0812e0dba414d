"""Helpers shared by the parity tests."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name: str):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def assert_close(got, want, rtol, atol, what=""):
    def _np(x):
        if hasattr(x, "detach"):
            x = x.detach().cpu().numpy()
        return np.asarray(x, dtype=np.float64)

    got, want = _np(got), _np(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {bad.sum()}/{bad.size} outside tol (rtol={rtol}, atol={atol}); worst at {i}: got {got[i]!r} want {want[i]!r}")


def assert_mostly_close(got, want, atol, max_bad_frac, max_rel_l2, what=""):
    """Robust comparison for chaotic paths (FQF: q(tau) runs through cos(pi*64*tau), so ulp-level differences in tau can
    flip an isolated ReLU and change a handful of elements by O(1)): bounds the FRACTION of elements outside ``atol``
    and the relative L2 error instead of the worst element."""
    def _np(x):
        if hasattr(x, "detach"):
            x = x.detach().cpu().numpy()
        return np.asarray(x, dtype=np.float64)

    got, want = _np(got), _np(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = np.abs(got - want) > atol
    frac = bad.mean() if bad.size else 0.0
    rel = np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30)
    assert frac <= max_bad_frac and rel <= max_rel_l2, f"{what}: {bad.sum()}/{bad.size} elements outside {atol} (allowed {max_bad_frac:.3%}), rel-L2 {rel:.3e} (allowed {max_rel_l2})"


def record_stats(name, payload):
    """Measured statistics of a GPU test, for profiles/ (gpurun merges gpurun_out/ back): one JSON file per statistic and case."""
    import json
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "test_stats")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as f:
            json.dump(payload, f, indent=1, sort_keys=True)
    except OSError:
        pass


def pinned_oracle(case: str):
    """The oracle's FQF steps of G6 case ``case`` computed in a child process in the CPU-independent mode (tests/golden/pinned.py, tests/pinned_oracle.py)."""
    import os, sys, tempfile
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import pinned
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        r = pinned.run([os.path.join(here, "pinned_oracle.py"), case, path], capture_output=True, text=True)
        assert r.returncode == 0, f"pinned oracle child failed:\n{r.stdout}\n{r.stderr}"
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ float64 convolution references (CPU torch, NCHW)
# The encoder's three layers (conv1 8x8 stride 4, conv2 4x4 stride 2, conv3 3x3 stride 1, each + bias + ReLU) evaluated in float64, every result with its
# accumulated magnitude: the same convolution on |a| and |b| (+ |bias|), the scale the device's fp32 accumulation error is measured on.  No import of the
# library: these are the yardstick the kernels are judged against (tests/test_conv_reference_helpers.py checks them against oracle/nets.py + autograd).
CONV_STRIDES = (4, 2, 1)


def conv_params64(sd):
    """The encoder's parameters of a reference state_dict as float64 torch tensors: [(w [N][C][kh][kw], b [N])] for conv1, conv2, conv3."""
    import torch
    return [(torch.as_tensor(np.asarray(sd[f"encoder.convs.{i}.weight"]), dtype=torch.float64),
             torch.as_tensor(np.asarray(sd[f"encoder.convs.{i}.bias"]), dtype=torch.float64)) for i in (0, 2, 4)]


def conv_fwd64(x, w, b, stride):
    """relu(conv(x, w) + b) and its scale conv(|x|, |w|) + |b|, float64 NCHW."""
    import torch.nn.functional as F
    x = x.double()
    y = F.conv2d(x, w, b, stride=stride)
    return y.clamp_min(0.0), F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride)


def encoder_chain64(x, params):
    """The three layers on x [B][C][H][W] (values, not bytes): [(act, scale)] per layer, each layer's scale propagated through |w| from the previous
    layer's, which bounds the error an fp32 evaluation of the whole chain can carry into every element (ReLU is 1-Lipschitz)."""
    import torch.nn.functional as F
    out, a, s = [], x.double(), x.double().abs()
    for (w, b), st in zip(params, CONV_STRIDES):
        a = F.conv2d(a, w, b, stride=st).clamp_min(0.0)
        s = F.conv2d(s, w.abs(), b.abs(), stride=st)
        out.append((a, s))
    return out


def conv_dgrad64(dy, w, stride, in_shape, mask):
    """The data gradient of a convolution, dx = conv_transpose(dy, w) masked by ``mask`` (the input layer's ReLU, 0/1 or bool), and its scale on |dy|, |w|."""
    from torch.nn.grad import conv2d_input
    m = mask.double()
    dy = dy.double()
    return conv2d_input(in_shape, w, dy, stride=stride) * m, conv2d_input(in_shape, w.abs(), dy.abs(), stride=stride) * m


def conv_wgrad64(x, dy, w_shape, stride):
    """Weight and bias gradients of a convolution (dW = sum_b,p dy x-patch, db = sum dy) and their scales on |x|, |dy|."""
    from torch.nn.grad import conv2d_weight
    x, dy = x.double(), dy.double()
    dw = conv2d_weight(x, w_shape, dy, stride=stride)
    sw = conv2d_weight(x.abs(), w_shape, dy.abs(), stride=stride)
    return dw, dy.sum((0, 2, 3)), sw, dy.abs().sum((0, 2, 3))


def nchw_from_nhwc(flat, B, H, W, C):
    """A device activation [B][H][W][C] (any flat tensor or array of B*H*W*C values) as a float64 NCHW torch tensor."""
    import torch
    t = flat.detach().cpu() if hasattr(flat, "detach") else torch.from_numpy(np.asarray(flat))
    return t.double().reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def conv_w_from_kernel(flat, layer, C=4):
    """A device weight block [N][K] (conv1: K in (c,kh,kw) order; conv2 / conv3: (kh,kw,c)) as float64 [N][C][kh][kw]."""
    import torch
    t = flat.detach().cpu() if hasattr(flat, "detach") else torch.from_numpy(np.asarray(flat))
    t = t.double()
    if layer == 0:
        return t.reshape(32, C, 8, 8)
    k, c = (4, 32) if layer == 1 else (3, 64)
    return t.reshape(64, k, k, c).permute(0, 3, 1, 2).contiguous()


def round_bf16(t):
    """Every element rounded to one bf16 term (the leading term of the kernels' three-term split), back in float64."""
    import torch
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def scale_err(got, want, scale):
    """Per-element |got - want| / scale (float64 numpy), the measure every convolution test bounds."""
    def _np(x):
        if hasattr(x, "detach"):
            x = x.detach().cpu()
            return x.double().numpy()
        return np.asarray(x, dtype=np.float64)
    got, want, scale = _np(got), _np(want), _np(scale)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    return (got - want) / np.maximum(scale, 1e-30)
