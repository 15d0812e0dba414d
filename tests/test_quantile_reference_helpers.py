"""CPU: the float64 references of tests/quantile_ref.py (the yardstick of tests/test_gpu_quantile_reference.py) against what the project already trusts:
the G5 fixture (the reference's huber_qr_loss and its gradient), the oracle's losses and nets run in float64, torch.autograd on the plain formulas and a
central finite difference.  Each returned scale must bound the result it belongs to."""
import numpy as np
import pytest
import torch

import quantile_ref as Q
import recipe
from util import golden


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


# ------------------------------------------------------------------------------------------------ quantile Huber
G5_TAGS = ["4x200x200", "8x64x64", "8x32x32", "3x8x5"]


def _g5(tag):
    g = golden("g5_huber_qr")
    q, t, tau, w = g[f"q_{tag}"], g[f"t_{tag}"], g[f"tau_{tag}"], g[f"w_{tag}"]
    B, N = q.shape
    tb = N if (tau.shape[0] == B and B > 1) else 0
    return g, q, t, tau, w, B, N, t.shape[1], tb


@pytest.mark.parametrize("tag", G5_TAGS)
def test_quantile_huber_against_the_reference_fixture(tag):
    """loss_* and dq_* of G5 were computed by the reference in fp32 from these very inputs: 1e-6 relative.  dq is a signed sum, so its fp32 error is
    relative to its accumulated magnitude: an element is held to 1e-6 of max(|dq|, scale) (the two agree unless the element cancels)."""
    g, q, t, tau, w, B, N, Nd, tb = _g5(tag)
    loss, dq, scale = Q.quantile_huber64(q, N, 1, N, t, tau, tb, np.zeros(B, np.int32), w, B, N, Nd)
    assert _rel(loss, g[f"loss_{tag}"]) < 1e-6
    want = g[f"dq_{tag}"].astype(np.float64)
    assert float(np.max(np.abs(dq - want) / np.maximum(np.abs(want), scale))) < 1e-6
    assert (np.abs(dq) <= scale * (1 + 1e-12) + 1e-300).all()


@pytest.mark.parametrize("tag", G5_TAGS)
@pytest.mark.parametrize("layout", ["qr", "iqn"])
def test_quantile_huber_against_the_oracle_in_float64(tag, layout):
    """oracle.losses.huber_quantile on float64 tensors, loss and autograd gradient, 1e-12; the G5 rows are scattered into an A = 3 tensor in the QR layout
    (sb, si, sa) = (A N, 1, N) and in the IQN / FQF layout (N A, A, 1), so the strides are exercised too."""
    from oracle.losses import huber_quantile
    g, q, t, tau, w, B, N, Nd, tb = _g5(tag)
    A = 3
    act = (np.arange(B) % A).astype(np.int32)
    full = recipe.gen(7).standard_normal((B, A, N)).astype(np.float32)
    full[np.arange(B), act] = q
    if layout == "qr":
        flat, (sb, si, sa) = full.reshape(-1), (A * N, 1, N)
    else:
        flat, (sb, si, sa) = np.ascontiguousarray(full.transpose(0, 2, 1)).reshape(-1), (N * A, A, 1)
    loss, dq, _ = Q.quantile_huber64(flat, sb, si, sa, t, tau, tb, act, w, B, N, Nd)
    qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    want = huber_quantile(qt, torch.from_numpy(t.astype(np.float64)), torch.from_numpy(tau.astype(np.float64)))
    want.mul(torch.from_numpy(w.astype(np.float64))).sum().backward()
    assert _rel(loss, want.detach().numpy()) < 1e-12
    assert float(np.max(np.abs(dq - qt.grad.numpy()))) < 1e-12 * float(np.max(np.abs(dq)))


def test_quantile_target_is_the_reference_expression():
    """agent.py:281-286 on float64 tensors, both layouts; done = 1 rows are the reward; the scale bounds the value."""
    g = recipe.gen(3)
    B, Nd, A, gam = 6, 5, 4, 0.99 ** 3
    qn = g.standard_normal((B, Nd, A)).astype(np.float32)
    a = np.array([0, 3, 1, 2, 3, 0], np.int32)
    r, d = g.standard_normal(B).astype(np.float32), np.array([0, 1, 0, 1, 0, 0], np.float32)
    want = r.astype(np.float64)[:, None] + float(np.float32(gam)) * (1 - d.astype(np.float64)[:, None]) * qn.astype(np.float64)[np.arange(B), :, a]
    for flat, (sb, sj, sa) in ((qn.reshape(-1), (Nd * A, A, 1)), (np.ascontiguousarray(qn.transpose(0, 2, 1)).reshape(-1), (A * Nd, 1, Nd))):
        y, s = Q.quantile_target64(flat, sb, sj, sa, a, r, d, gam, B, Nd)
        assert np.array_equal(y, want)
        assert np.array_equal(y[d == 1], np.broadcast_to(r.astype(np.float64)[d == 1, None], (2, Nd)))
        assert (np.abs(y) <= s).all()


# ------------------------------------------------------------------------------------------------ FQF
def _fraction_case(B, F, A, seed, ldl=None):
    g = recipe.gen(seed)
    ldl = F if ldl is None else ldl
    q = np.sort(g.standard_normal((B, F - 1, A)).astype(np.float32), 1)
    qh = np.sort(g.standard_normal((B, F, A)).astype(np.float32), 1)
    if seed % 2:
        q, qh = g.permuted(q, axis=1), g.permuted(qh, axis=1)
    logits = np.full((B, ldl), np.nan, np.float32)
    logits[:, :F] = g.standard_normal((B, F)).astype(np.float32)
    taus = Q.fqf_taus64(logits, ldl, B, F)[0].astype(np.float32)
    act = g.integers(0, A, B).astype(np.int32)
    w = g.uniform(0.2, 1.0, B).astype(np.float32)
    return q, qh, taus, act, w, logits, ldl


@pytest.mark.parametrize("B,F,A,seed,ldl", [(3, 5, 4, 1, None), (2, 32, 9, 2, None), (4, 33, 2, 3, 64), (1, 2, 1, 4, 32)])
def test_fraction_loss_against_the_oracle_expression(B, F, A, seed, ldl):
    """The fraction_loss of oracle.losses.fqf_loss (lines `v1 = ...` to `fraction_loss = ...`), its own expression on float64 tensors: 1e-12."""
    q, qh, taus, act, w, logits, ldl = _fraction_case(B, F, A, seed, ldl)
    out = Q.fqf_fraction64(q, qh, taus, act, w, logits, ldl, B, F, A)
    ar = torch.arange(B)
    at = torch.from_numpy(act.astype(np.int64))
    qq = torch.from_numpy(q.astype(np.float64))[ar, :, at]
    q_hat = torch.from_numpy(qh.astype(np.float64))[ar, :, at]
    t = torch.from_numpy(taus.astype(np.float64))[:, :, None]
    v1 = qq - q_hat[:, :-1]
    s1 = qq > torch.cat((q_hat[:, :1], qq[:, :-1]), dim=1)
    v2 = qq - q_hat[:, 1:]
    s2 = qq < torch.cat((qq[:, 1:], q_hat[:, -1:]), dim=1)
    gg = torch.where(s1, v1, -v1) + torch.where(s2, v2, -v2)
    want = (gg * t[:, 1:-1, 0]).sum(dim=1).numpy()
    assert float(np.max(np.abs(out["loss"] - want))) <= 1e-12 * float(np.max(out["loss_scale"]))
    assert (np.abs(out["loss"]) <= out["loss_scale"] * (1 + 1e-12)).all()
    assert (np.abs(out["g"]).sum(1) <= out["S"] * (1 + 1e-12)).all()
    # |d (w loss) / d logit_k| = |w| p_k |dp_k - sum_j p_j dp_j| <= 2 |w| S p_k
    assert (np.abs(out["dlogits"]) <= 2 * np.abs(w.astype(np.float64))[:, None] * out["S"][:, None] * out["p"] * (1 + 1e-9) + 1e-300).all()
    assert np.abs(out["dlogits"].sum(1)).max() < 1e-12 * max(1.0, float(out["S"].max()))          # softmax: the gradient sums to 0 over the logits


def test_fraction_gradient_against_a_central_difference():
    """F = 5: d (sum_b w_b sum_i g_i tau_{i+1}(logits)) / d logits by central differences in float64 on an independent numpy evaluation of the taus."""
    B, F, A = 3, 5, 4
    q, qh, taus, act, w, logits, ldl = _fraction_case(B, F, A, 1)
    out = Q.fqf_fraction64(q, qh, taus, act, w, logits, ldl, B, F, A)
    g = out["g"]

    def surrogate(lg):
        t = Q.fqf_taus64(lg, F, B, F)[0]
        return float((w.astype(np.float64) * (g * t[:, 1:-1]).sum(1)).sum())

    x = logits.astype(np.float64)
    h, fd = 1e-6, np.zeros((B, F))
    for b in range(B):
        for k in range(F):
            xp, xm = x.copy(), x.copy()
            xp[b, k] += h
            xm[b, k] -= h
            fd[b, k] = (surrogate(xp) - surrogate(xm)) / (2 * h)
    assert float(np.max(np.abs(out["dlogits"] - fd))) < 1e-8 * max(1.0, float(np.abs(fd).max()))
    assert float(np.abs(out["dlogits"]).max()) > 1e-3                                                # a gradient that is really there


@pytest.mark.parametrize("B,F,ld", [(1, 2, 2), (3, 32, 32), (3, 33, 64), (2, 64, 64), (3, 7, 32)])
def test_fractions_against_the_oracle_in_float64(B, F, ld):
    """oracle.nets.fqf_prop_taus with the fraction net set to the identity (weight I, bias 0), so that its input is the logits, on float64 tensors."""
    from oracle import nets
    logits = np.full((B, ld), np.nan, np.float32)
    logits[:, :F] = (recipe.gen(F).standard_normal((B, F)) * 3).astype(np.float32)
    taus, tau_hat, p = Q.fqf_taus64(logits, ld, B, F)
    params = {"head.fraction_net.weight": torch.eye(F, dtype=torch.float64), "head.fraction_net.bias": torch.zeros(F, dtype=torch.float64)}
    t, th, _ = nets.fqf_prop_taus(params, None, torch.from_numpy(logits[:, :F].astype(np.float64)))
    assert float(np.max(np.abs(taus - t[:, :, 0].numpy()))) < 1e-12
    assert float(np.max(np.abs(tau_hat - th[:, :, 0].numpy()))) < 1e-12
    assert (taus[:, 0] == 0).all() and (np.diff(taus, axis=1) >= 0).all() and np.abs(taus[:, -1] - 1).max() < 1e-12
    assert np.abs(p.sum(1) - 1).max() < 1e-12


# ------------------------------------------------------------------------------------------------ dueling combine
@pytest.mark.parametrize("R,A,T,dueling", [(1, 1, 1, 0), (1, 1, 1, 1), (5, 4, 1, 1), (3, 18, 51, 1), (7, 2, 37, 1), (4, 6, 3, 0)])
@pytest.mark.parametrize("extra", [0, 32])
def test_dueling_against_autograd(R, A, T, dueling, extra):
    """v + (x - x.mean(actions)) on float64 tensors and its autograd gradient; pad columns get gradient 0 and scale 0; the scales bound the values."""
    g = recipe.gen(R * 100 + A)
    ld = -(-(A * T + (T if dueling else 0)) // 32) * 32 + extra
    raw = g.standard_normal((R, ld)).astype(np.float32)
    go = g.standard_normal((R, A, T)).astype(np.float32)
    q, qs = Q.dueling_fwd64(raw.reshape(-1), ld, R, A, T, dueling)
    dr, ds = Q.dueling_bwd64(go, ld, R, A, T, dueling)
    x = torch.from_numpy(raw.astype(np.float64)).requires_grad_(True)
    adv = x[:, :A * T].reshape(R, A, T)
    want = (x[:, A * T:A * T + T].reshape(R, 1, T) + (adv - adv.mean(1, keepdim=True))) if dueling else adv
    (want * torch.from_numpy(go.astype(np.float64))).sum().backward()
    assert float(np.max(np.abs(q - want.detach().numpy()))) < 1e-14 * max(1.0, float(qs.max()))
    assert float(np.max(np.abs(dr - x.grad.numpy()))) < 1e-14 * max(1.0, float(ds.max()))
    assert (np.abs(q) <= qs * (1 + 1e-12)).all() and (np.abs(dr) <= ds * (1 + 1e-12)).all()
    used = A * T + (T if dueling else 0)
    assert (dr[:, used:] == 0).all() and (ds[:, used:] == 0).all()


# ------------------------------------------------------------------------------------------------ Hadamard product and cosine features
@pytest.mark.parametrize("B,n,D", [(1, 1, 4), (3, 5, 85), (4, 3, 64), (2, 7, 1)])
def test_hadamard_backward_against_autograd(B, n, D):
    """relu(e) * relu(f) on float64 tensors: the kernels receive emb = relu(e) and feat = relu(f) (with exact zeros where e, f <= 0) and return the gradients
    w.r.t. the pre-activations e and f.  demb is one fp32 product (compared after rounding the float64 one), d3 float64 to 1e-14 of its scale."""
    g = recipe.gen(B * 10 + n)
    e, f = g.standard_normal((B, n, D)).astype(np.float32), g.standard_normal((B, 1, D)).astype(np.float32)
    e[0, 0, 0], f[0, 0, -1] = 0.0, -0.0
    dx = g.standard_normal((B, n, D)).astype(np.float32)
    emb, feat = np.maximum(e, 0), np.maximum(f, 0)
    demb, d3, s3 = Q.hadamard_bwd64(dx, emb, feat, B, n, D)
    et, ft = torch.from_numpy(e.astype(np.float64)).requires_grad_(True), torch.from_numpy(f.astype(np.float64)).requires_grad_(True)
    (et.relu() * ft.relu() * torch.from_numpy(dx.astype(np.float64))).sum().backward()
    assert np.array_equal(Q.hadamard_fwd32(emb, feat, B, n, D), (et.relu() * ft.relu()).detach().numpy().astype(np.float32))
    assert np.array_equal(demb, et.grad.numpy().astype(np.float32))
    assert float(np.max(np.abs(d3 - ft.grad.numpy()[:, 0]))) <= 1e-14 * max(1.0, float(s3.max()))
    assert (np.abs(d3) <= s3 * (1 + 1e-12)).all()
    assert (d3[feat[:, 0] <= 0] == 0).all() and (demb[emb <= 0] == 0).all()


def test_cosine_features_are_the_cosine_of_the_fp32_argument():
    """The argument is two fp32 products: fl32(pi) (d + 1), then times tau, each rounded once.  Against cos(pi (d + 1) tau) in float64 the difference is the
    argument's rounding alone, at most 2^-23 |x| + ... with |x| <= 64 pi; at tau = 0 every feature is exactly 1."""
    taus = np.concatenate(([0.0, 0.5, 1 - 2.0 ** -24, 2.0 ** -24], recipe.gen(5).random(60))).astype(np.float32)
    for D in (64, 7):
        a = Q.cos_args32(taus, D)
        assert a.dtype == np.float32 and a.shape == (64, D)
        ipi = (np.float32(np.pi) * np.arange(1, D + 1, dtype=np.float32)).astype(np.float32)
        assert np.array_equal(ipi, torch.mul(torch.arange(1, D + 1, dtype=torch.float32), np.pi).numpy())          # np.pi * torch.arange(1, D + 1), model.py
        assert np.array_equal(a, (torch.from_numpy(ipi)[None, :] * torch.from_numpy(taus)[:, None]).numpy())
        c = Q.cos_features64(taus, D)
        exact = np.cos(np.pi * np.arange(1, D + 1)[None, :] * taus.astype(np.float64)[:, None])
        assert float(np.max(np.abs(c - exact))) <= 2.0 ** -22 * np.pi * D
        assert (c[0] == 1.0).all() and (np.abs(c) <= 1.0).all()
