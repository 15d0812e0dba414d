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


# ------------------------------------------------------------------------------------------------ float64 action-selection references (numpy)
# What the actor's tail kernels compute between a head GEMM's split-K slabs and the action (slab sum + bias, dueling combine, action values, first maximum),
# in float64, every result with its accumulated magnitude: the same computation on absolute values, the scale an fp32 evaluation's rounding error is
# measured on.  No import of the library (tests/test_actor_tail_reference_helpers.py checks them against oracle/nets.py).
def _dueling64(x, A):
    """q(a) = v + (x(a) - mean_a x) over axis 1 of x [E][A + 1][T] (row A: the value stream)."""
    return x[:, A:A + 1] + (x[:, :A] - x[:, :A].mean(1, keepdims=True))


def head_from_slabs64(slabs, bias, A, T, dueling, kt):
    """(q, scale) [E][A][T] of a head GEMM's split-K slabs [nslab][rows][ld]: slab sum + bias, then the dueling combine per atom.  ``kt`` = 0: one row per
    env, columns (a, t) followed by the value stream's T columns, a bias per column; ``kt`` = 1: rows (env, quantile), columns a followed by the value
    column, a bias per column.  Pad columns beyond those are ignored."""
    s, b = np.asarray(slabs, np.float64), np.asarray(bias, np.float64)
    NQ = A + (1 if dueling else 0)

    def arrange(x, bb):
        raw = x.sum(0)
        if kt:
            return (raw.reshape(-1, T, raw.shape[-1])[:, :, :NQ] + bb[:NQ]).transpose(0, 2, 1)
        return (raw[:, :NQ * T] + bb[:NQ * T]).reshape(-1, NQ, T)

    q, m = arrange(s, b), arrange(np.abs(s), np.abs(b))
    if dueling:
        q, m = _dueling64(q, A), m[:, A:A + 1] + (m[:, :A] + m[:, :A].mean(1, keepdims=True))
    return np.ascontiguousarray(q), np.ascontiguousarray(m)


def action_values64(q, mode, aux=None, qscale=None):
    """(values, scale) [E][A] of q [E][A][T] (``qscale``: q's own accumulated magnitude, |q| if not given).  mode 0: q[..., 0]; 1: mean over t;
    2: sum_t softmax_t(q) atoms[t] (``aux`` = atoms [T]; scale sum_t p_t |atoms[t]|, the magnitude the expectation's errors are relative to);
    3: sum_t (tau[t + 1] - tau[t]) q (``aux`` = tau [E][T + 1])."""
    q = np.asarray(q, np.float64)
    m = np.abs(q) if qscale is None else np.asarray(qscale, np.float64)
    if mode == 0:
        return q[:, :, 0].copy(), m[:, :, 0].copy()
    if mode == 1:
        return q.mean(2), m.mean(2)
    if mode == 2:
        z = np.asarray(aux, np.float64)
        p = np.exp(q - q.max(2, keepdims=True))
        p /= p.sum(2, keepdims=True)
        return (p * z).sum(2), (p * np.abs(z)).sum(2)
    if mode == 3:
        tau = np.asarray(aux, np.float64)
        d = (tau[:, 1:] - tau[:, :-1])[:, None, :]
        return (d * q).sum(2), (np.abs(d) * m).sum(2)
    raise ValueError(mode)


def qhead64(feat, W1, b1, W2, b2, A, dueling):
    """(q, scale) [E][A] of the scalar head: h = relu(feat W1^T + b1), raw = h W2^T + b2, dueling combine.  The scale carries fc1's accumulated
    magnitude (|feat| |W1|^T + |b1|, which bounds |h|: ReLU is 1-Lipschitz) through |W2| and |b2| and the combine, as encoder_chain64 carries a layer's."""
    f, w1, bb1, w2, bb2 = (np.asarray(x, np.float64) for x in (feat, W1, b1, W2, b2))
    h = np.maximum(f @ w1.T + bb1, 0.0)
    s1 = np.abs(f) @ np.abs(w1).T + np.abs(bb1)
    # row by row, every row summed in the same order: bit-identical head rows give bit-identical values (a BLAS product does not promise that)
    q, m = (h[:, None, :] * w2[None]).sum(2) + bb2, (s1[:, None, :] * np.abs(w2)[None]).sum(2) + np.abs(bb2)
    if dueling:
        q, m = _dueling64(q[:, :, None], A)[:, :, 0], m[:, A:A + 1] + (m[:, :A] + m[:, :A].mean(1, keepdims=True))
    return np.ascontiguousarray(q[:, :A]), np.ascontiguousarray(m[:, :A])


def greedy_check(values64, tol, got_action, got_qmax, what="", exclude=None, tie=None, allow_empty=False):
    """Judges a device's greedy actions and their values against float64 action values [E][A] with a per-element error bound ``tol`` [E][A].  Env e is
    DECIDED when exactly one action lies within tol[e, a] + tol[e, a*] of the maximum: there the device's action must be the float64 argmax; on an
    undecided env it must be one of those candidates.  ``got_qmax`` must lie within tol of the float64 value of the action the device chose.  ``tie`` =
    (i, j), i < j: two actions whose inputs are bit-identical — wherever their float64 values are equal the device may never answer j (the first maximum
    wins).  Returns the share of undecided envs among those not flagged in ``exclude`` (bool [E]); if that leaves no env to judge the check fails, unless
    ``allow_empty`` (a single env, or two actions that are the tied pair: nothing but the tie can be asked for)."""
    v, tol = np.asarray(values64, np.float64), np.asarray(tol, np.float64)
    act, qm = np.asarray(got_action).astype(np.int64).reshape(-1), np.asarray(got_qmax, np.float64).reshape(-1)
    E, A = v.shape
    assert tol.shape == v.shape and act.shape == (E,) and qm.shape == (E,), (v.shape, tol.shape, act.shape, qm.shape)
    assert ((act >= 0) & (act < A)).all(), f"{what}: actions outside [0, {A}): {act}"
    best = v.argmax(1)
    rows = np.arange(E)
    cand = (v[rows, best][:, None] - v) <= (tol + tol[rows, best][:, None])
    undecided = cand.sum(1) > 1
    assert cand[rows, act].all(), f"{what}: envs {np.nonzero(~cand[rows, act])[0]}: action {act[~cand[rows, act]]}, float64 argmax {best[~cand[rows, act]]}"
    err = np.abs(qm - v[rows, act])
    bad = ~(err <= tol[rows, act])
    assert not bad.any(), f"{what}: max-Q of envs {np.nonzero(bad)[0]} off by {err[bad]} (bound {tol[rows, act][bad]})"
    if tie is not None:
        i, j = tie
        wrong = (act == j) & (v[:, i] == v[:, j])
        assert not wrong.any(), f"{what}: envs {np.nonzero(wrong)[0]}: of two equal actions {i} and {j} the later one was chosen"
    keep = np.ones(E, bool) if exclude is None else ~np.asarray(exclude, bool)
    assert keep.any() or allow_empty, f"{what}: every env is excluded, no free maximum is judged"
    return float(undecided[keep].mean()) if keep.any() else 0.0
