"""CPU: the float64 convolution references of tests/util.py (the yardstick of tests/test_gpu_conv_reference.py) against the oracle's encoder
(oracle/nets.py) run in float64 with torch autograd, at the tiny geometry; and the layout conversions those GPU tests use against the library's own
parameter packing."""
import numpy as np
import torch

import recipe
from oracle import nets
from util import (CONV_STRIDES, conv_dgrad64, conv_fwd64, conv_params64, conv_w_from_kernel, conv_wgrad64, encoder_chain64, nchw_from_nhwc,
                  scale_err)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def test_float64_conv_helpers_match_the_oracle_encoder_and_autograd():
    spec = recipe.NetSpec("dqn", 4, obs_shape=(4, 36, 36))
    sd = recipe.make_state_dict(spec, 3)
    params = conv_params64(sd)
    p = {f"encoder.convs.{i}.{k}": torch.from_numpy(np.asarray(sd[f"encoder.convs.{i}.{k}"])).double().requires_grad_(True)
         for i in (0, 2, 4) for k in ("weight", "bias")}
    B = 3
    x = torch.from_numpy(recipe.make_frames(B, 4, spec.obs_shape)[:, :4]).double() / 255.0
    feat, (a1, a2, a3) = nets.encoder(p, x, return_all=True)
    G = torch.from_numpy(recipe.gen(5).standard_normal(tuple(feat.shape)))
    loss = (feat * G).sum()
    ga1, ga2 = torch.autograd.grad(loss, [a1, a2], retain_graph=True)
    gw = torch.autograd.grad(loss, [p[f"encoder.convs.{i}.{k}"] for i in (0, 2, 4) for k in ("weight", "bias")])
    # forward, layer by layer on the oracle's own inputs, and as a chain
    ins = [x, a1.detach(), a2.detach()]
    outs = [a1, a2, a3]
    for layer, ((w, b), st) in enumerate(zip(params, CONV_STRIDES)):
        y, s = conv_fwd64(ins[layer], w, b, st)
        assert _rel(y, outs[layer].detach()) < 1e-12, layer
        assert bool((s >= y.abs()).all())
    for (y, s), ref in zip(encoder_chain64(x, params), outs):
        assert _rel(y, ref.detach()) < 1e-12
        assert bool((s >= y).all())
    # data gradients: the gradient at each pre-activation, masked by the layer's ReLU
    d3 = G.reshape(a3.shape) * (a3 > 0)
    d2, s2 = conv_dgrad64(d3, params[2][0], 1, a2.shape, a2.detach() > 0)
    assert _rel(d2, ga2 * (a2 > 0)) < 1e-12 and bool((s2 >= d2.abs()).all())
    d1, _ = conv_dgrad64(d2, params[1][0], 2, a1.shape, a1.detach() > 0)
    assert _rel(d1, ga1 * (a1 > 0)) < 1e-12
    # weight and bias gradients of every layer from its input and the gradient at its pre-activation
    for layer, (inp, dy) in enumerate(((x, d1), (a1.detach(), d2), (a2.detach(), d3))):
        dw, db, sw, sb = conv_wgrad64(inp, dy, params[layer][0].shape, CONV_STRIDES[layer])
        assert _rel(dw, gw[2 * layer]) < 1e-12 and _rel(db, gw[2 * layer + 1]) < 1e-12, layer
        assert bool((sw >= dw.abs()).all()) and bool((sb >= db.abs()).all())
    assert np.abs(scale_err(d2.float(), d2, s2)).max() < 1e-6


def test_layout_conversions_match_the_parameter_packing():
    """nchw_from_nhwc / conv_w_from_kernel invert the device layouts: activations [B][H][W][C], weights as NetLayout.pack stores them."""
    from agent0_amd.deepq.layout import NetLayout
    spec = recipe.NetSpec("dqn", 4, obs_shape=(4, 44, 52))
    L = NetLayout.from_spec(spec)
    sd = recipe.make_state_dict(spec, 8)
    flat = torch.zeros(L.n_params_padded, dtype=torch.float64)
    L.pack({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, flat)
    for layer, (w, b) in enumerate(conv_params64(sd)):
        blk = L.blocks[("conv1", "conv2", "conv3")[layer]]
        assert torch.equal(conv_w_from_kernel(flat[blk.w], layer), w)
        assert torch.equal(flat[blk.b], b)
    a = torch.arange(2 * 3 * 5 * 7, dtype=torch.float64).reshape(2, 7, 3, 5)
    assert torch.equal(nchw_from_nhwc(a.permute(0, 2, 3, 1).reshape(-1), 2, 3, 5, 7), a)
