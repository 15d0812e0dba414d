"""Float64 references of the quantile learners' small kernels (QR / IQN / FQF) and of the dueling combine: the yardstick of
tests/test_gpu_quantile_reference.py, itself held to the oracle, the G5 fixture and torch.autograd by tests/test_quantile_reference_helpers.py.

No import of the library.  Every function takes the fp32 inputs exactly as the kernel receives them (flat or shaped numpy arrays, the strides the entry
point takes) and evaluates the reference's formula in float64 in its most literal form: the B x N' x N pair tensor of agent.py:110-114 is materialised,
the fraction loss is written as agent.py:371-387 writes it and differentiated by torch.autograd.  Discontinuous decisions (T_j < q_i, q_i > prev,
q_i < next, the ReLU masks, done) are taken on the fp32 values themselves: fp32 -> float64 is exact and order preserving, so the reference and a correct
kernel take the same branch on every input and no case has to be left out.  Where a tolerance needs it the function also returns the result's
accumulated magnitude (the same computation on absolute values), the scale an fp32 evaluation's rounding error is measured on."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                                     # unit roundoff of fp32
PI32 = np.float32(3.14159274101257324)             # fl32(pi), the constant `np.pi * torch.arange(1, D + 1)` rounds to (model.py:235-251)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ dueling combine (model.py:163-177)
def dueling_fwd64(raw, ld, R, A, T, dueling):
    """(q, scale) [R][A][T] of raw [R][ld]: columns [0, A*T) the advantages (action-major), [A*T, A*T + T) the value stream when ``dueling``.
    q = v + (x - x.mean(actions)); scale = |v| + |x_a| + sum_a |x_a| / A.  Not dueling: q = x, scale = |x|."""
    x = _f64(raw).reshape(-1)[:R * ld].reshape(R, ld)
    adv = x[:, :A * T].reshape(R, A, T)
    if not dueling:
        return adv.copy(), np.abs(adv)
    v = x[:, A * T:A * T + T][:, None, :]
    return v + (adv - adv.mean(1, keepdims=True)), np.abs(v) + np.abs(adv) + np.abs(adv).sum(1, keepdims=True) / A


def dueling_bwd64(g, ld, R, A, T, dueling):
    """(draw, scale) [R][ld] of g = d loss / d q [R][A][T]: advantage column (a, t) gets g - sum_a g / A (scale |g| + sum_a |g| / A), value column t gets
    sum_a g (scale sum_a |g|), every further column 0 with scale 0.  Not dueling: the copy."""
    g = _f64(g).reshape(R, A, T)
    draw, scale = np.zeros((R, ld)), np.zeros((R, ld))
    if not dueling:
        draw[:, :A * T], scale[:, :A * T] = g.reshape(R, A * T), np.abs(g).reshape(R, A * T)
        return draw, scale
    s, sa = g.sum(1, keepdims=True), np.abs(g).sum(1, keepdims=True)
    draw[:, :A * T], scale[:, :A * T] = (g - s / A).reshape(R, A * T), (np.abs(g) + sa / A).reshape(R, A * T)
    draw[:, A * T:A * T + T], scale[:, A * T:A * T + T] = s[:, 0], sa[:, 0]
    return draw, scale


# ------------------------------------------------------------------------------------------------ target quantiles (agent.py:281-286, 359-364)
def _gather(flat, B, n, sb, sn, sa, a):
    """x[b][i] = flat[b*sb + i*sn + a[b]*sa], float64."""
    flat = _f64(flat).reshape(-1)
    idx = np.arange(B)[:, None] * sb + np.arange(n)[None, :] * sn + np.asarray(a, np.int64)[:, None] * sa
    return flat[idx]


def quantile_target64(q_next, sb, sj, sa, a_star, rew, done, gamma_n, B, Nd):
    """(y, scale) [B][Nd]: y = r + gamma_n (1 - done) q'(b, j, a*_b), gamma_n rounded to fp32 as the entry point receives it; scale = |r| + gamma_n |q'|."""
    qn = _gather(q_next, B, Nd, sb, sj, sa, a_star)
    gam = float(np.float32(gamma_n))
    r, d = _f64(rew).reshape(B, 1), _f64(done).reshape(B, 1)
    return r + gam * (1.0 - d) * qn, np.abs(r) + gam * np.abs(qn)


# ------------------------------------------------------------------------------------------------ quantile Huber (agent.py:110-114)
def quantile_huber64(q, sb, si, sa, y, taus, tb, act, wgt, B, N, Nd):
    """agent.py:110-114 on the materialised B x N' x N pair tensor, and d (sum_b w_b loss_b) / d q at the taken action by torch.autograd, in float64.
    q(b, i, a) = q[b*sb + i*si + a*sa]; y [B][N']; taus[b*tb + i] (tb = 0: one shared row).  Returns (loss [B], dq [B][N], dq_scale [B][N]) with
    dq_scale = |w_b| / N' * sum_j |clamp(q_i - T_j, -1, 1)| |tau_i - 1{T_j < q_i}|.  Every term of the loss is non-negative: it is its own scale."""
    import torch
    import torch.nn.functional as F
    qa = torch.from_numpy(_gather(q, B, N, sb, si, sa, act)).requires_grad_(True)            # [B][N]
    t = torch.from_numpy(_f64(y).reshape(B, Nd))
    tau = torch.from_numpy(_f64(taus).reshape(-1)[(np.arange(B)[:, None] * tb + np.arange(N)[None, :])])
    w = torch.from_numpy(_f64(wgt).reshape(B))
    qe, te = qa.view(B, 1, N).expand(B, Nd, N), t.view(B, Nd, 1).expand(B, Nd, N)            # q "b 1 n", q_target "b n 1"
    huber = F.smooth_l1_loss(qe, te, reduction="none")
    ind = te.lt(qe).detach().double()
    pair = huber * (tau.view(B, 1, N) - ind).abs()
    loss = pair.sum(-1).mean(-1).view(-1)
    loss.mul(w).sum().backward()
    with torch.no_grad():
        d = (qe - te).clamp(-1.0, 1.0).abs()
        scale = w.abs().view(B, 1) / Nd * (d * (tau.view(B, 1, N) - ind).abs()).sum(1)
    return loss.detach().numpy(), qa.grad.numpy(), scale.numpy()


# ------------------------------------------------------------------------------------------------ cosine features (model.py:235-251)
def cos_args32(taus, D):
    """The fp32 argument the kernels hand to cosf: fl32(fl32(fl32(pi) * (d + 1)) * tau), [R][D] float32."""
    ipi = (PI32 * np.arange(1, D + 1, dtype=np.float32)).astype(np.float32)
    return (ipi[None, :] * np.asarray(taus, np.float32).reshape(-1, 1)).astype(np.float32)


def cos_features64(taus, D):
    """cos of the fp32 argument, in float64, [R][D]: a comparison against it measures cosf alone and not the argument's rounding."""
    return np.cos(cos_args32(taus, D).astype(np.float64))


# ------------------------------------------------------------------------------------------------ Hadamard product (model.py:253-257)
def hadamard_fwd32(emb, feat, B, n, D):
    """x[(b, n)][d] = fl32(emb * feat[b]): one fp32 product per element, so the kernel is held to it bit for bit."""
    return (np.asarray(emb, np.float32).reshape(B, n, D) * np.asarray(feat, np.float32).reshape(B, 1, D)).astype(np.float32)


def hadamard_bwd64(dx, emb, feat, B, n, D):
    """(demb32 [B][n][D], d3 [B][D], d3_scale [B][D]) of x = emb * feat with emb = relu(.) and feat = relu(.) as the kernels' inputs:
    demb = emb > 0 ? fl32(dx * feat) : 0 (one fp32 product: exact); d3 = feat > 0 ? sum_n dx emb : 0 in float64, scale sum_n |dx| |emb| under the same
    mask.  The masks are taken on the fp32 values (0 and -0.0 are not > 0); emb enters d3's sum as given, so an input that is not a ReLU's output
    (negative emb) is judged by the same formula."""
    dx32, e32, f32 = (np.asarray(a, np.float32) for a in (dx, emb, feat))
    dx32, e32, f32 = dx32.reshape(B, n, D), e32.reshape(B, n, D), f32.reshape(B, 1, D)
    demb = np.where(e32 > 0, (dx32 * f32).astype(np.float32), np.float32(0)).astype(np.float32)
    keep = f32[:, 0] > 0
    d3 = np.where(keep, (_f64(dx32) * _f64(e32)).sum(1), 0.0)
    scale = np.where(keep, (np.abs(_f64(dx32)) * np.abs(_f64(e32))).sum(1), 0.0)
    return demb, d3, scale


# ------------------------------------------------------------------------------------------------ FQF fraction proposal (model.py:268-278)
def fqf_taus64(logits, ld, B, F):
    """(taus [B][F + 1], tau_hat [B][F], p [B][F]) of logits [B][ld] (columns [F, ld) are padding and never read): p = softmax, taus = (0, cumsum p),
    tau_hat the midpoints."""
    x = _f64(np.asarray(logits).reshape(-1)[:B * ld].reshape(B, ld)[:, :F])
    z = x - x.max(1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(1, keepdims=True)
    taus = np.concatenate((np.zeros((B, 1)), np.cumsum(p, 1)), 1)
    return taus, (taus[:, :-1] + taus[:, 1:]) / 2.0, p


# ------------------------------------------------------------------------------------------------ FQF fraction loss (agent.py:371-387)
def fqf_fraction64(q, qh, taus, act, wgt, logits, ldl, B, F, A):
    """The fraction loss as agent.py:371-387 writes it and the gradient of sum_b w_b loss_b w.r.t. the fraction logits.
    q [B][F-1][A] at the interior fractions, qh [B][F][A] at the tau-hats, taus [B][F+1] (fp32, what the loss value multiplies), logits [B][ldl].
    loss_b = sum_i g_i taus[b][i + 1].  The gradient comes from torch.autograd on w_b sum_i g_i cumsum(softmax(logits[b][:F]))_{i+1} with g detached.
    Returns a dict: loss [B], dlogits [B][F], and the scales loss_scale [B] = sum_i (|v1_i| + |v2_i|) tau_{i+1}, S [B] = sum_i (|v1_i| + |v2_i|),
    p [B][F] = softmax(logits), g [B][F-1] = the detached gradients_of_taus."""
    import torch
    ar = torch.arange(B)
    a = torch.from_numpy(np.asarray(act, np.int64).reshape(B))
    q_all = torch.from_numpy(_f64(q).reshape(B, F - 1, A))
    qh_all = torch.from_numpy(_f64(qh).reshape(B, F, A))
    t_in = torch.from_numpy(_f64(taus).reshape(B, F + 1))
    w = torch.from_numpy(_f64(wgt).reshape(B))
    lg = torch.from_numpy(_f64(np.asarray(logits).reshape(-1)[:B * ldl].reshape(B, ldl)[:, :F]).copy()).requires_grad_(True)
    q_hat = qh_all[ar, :, a]
    with torch.no_grad():
        qq = q_all[ar, :, a]
        values_1 = qq - q_hat[:, :-1]
        signs_1 = qq.gt(torch.cat((q_hat[:, :1], qq[:, :-1]), dim=1))
        values_2 = qq - q_hat[:, 1:]
        signs_2 = qq.lt(torch.cat((qq[:, 1:], q_hat[:, -1:]), dim=1))
    gradients_of_taus = torch.where(signs_1, values_1, -values_1) + torch.where(signs_2, values_2, -values_2)
    loss = (gradients_of_taus * t_in[:, 1:-1]).sum(dim=1).view(-1)
    # the differentiable taus of FQFHead.prop_taus: (0, cumsum softmax); taus[:, 1:-1] are cumsum's first F - 1 entries
    p = lg.softmax(dim=-1)
    cum = torch.cumsum(p, dim=-1)
    (w * (gradients_of_taus.detach() * cum[:, :-1]).sum(dim=1)).sum().backward()
    mag = values_1.abs() + values_2.abs()
    return {"loss": loss.numpy(), "dlogits": lg.grad.numpy(), "loss_scale": (mag * t_in[:, 1:-1]).sum(1).numpy(), "S": mag.sum(1).numpy(),
            "p": p.detach().numpy(), "g": gradients_of_taus.numpy()}
