"""GPU (MI355X): the quantile learners' small kernels and the dueling combine against float64, each on its own, at the edges of its work split.

Kernels (agent0_amd/csrc/quantile.hip, loss.hip and loss_quantile.hip): a0_dueling_fwd / _bwd, a0_quantile_target, a0_loss_quantile_huber (a0_qh_sweep, which the
fused QR kernel shares), a0_cos_features, a0_tau_cos_features, a0_fqf_taus, a0_fqf_taus_cos, a0_fqf_inner_taus, a0_hadamard_fwd / _bwd and
a0_fqf_fraction_loss.  References: tests/quantile_ref.py, held on the CPU to the G5 fixture, the oracle in float64, torch.autograd and a finite difference by
tests/test_quantile_reference_helpers.py.  The whole-update tests reach these kernels at one geometry only (F = 32, N = N' = 64, A = 4 / 9 / 18) and the
bit-identity tests of the fused kernels use them as their yardstick; here every shape is the smallest that straddles a work split: one element, one past a
block of 256, one past a wave of 64, the four-wide target sweep with and without its scalar tail, strided ownership (N > 256), both (sb, si, sa) layouts,
F on both sides of 32 and at 64, a padded leading dimension whose padding holds NaN.

Every output is prefilled with NaN (or, where the contract says "left alone", with a sentinel that must survive bit for bit) and followed by 64 sentinel
elements, so an element never written, written out of place or written past the end fails.  Discontinuous decisions are taken on the fp32 inputs by both
sides (quantile_ref.py), so ties and seams are planted, not avoided, and nothing is excluded.

Tolerances.  u = 2^-24; an fp32 operation moves its result by at most u of the magnitude it works at, and an element is held to c u SCALE, SCALE the same
computation on absolute values and c the roundings on its longest path:
  dueling forward   (A + 4) u (|v| + |x_a| + sum_a |x_a| / A); not dueling: the copy, bit for bit
  dueling backward  (A + 4) u (|g| + sum_a |g| / A), value column (A + 4) u sum_a |g|; pad columns exactly 0; <fwd(x), g> = <x, bwd(g)> to the two bounds summed
  target quantiles  3 u (|r| + gamma_n |q'|); done = 1: the reward, bit for bit
  quantile Huber    loss (N' + 12) u loss_b (all terms non-negative); dq (N' + 4) u |w_b| / N' sum_j |clamp(d)| |tau - 1{T_j < q_i}|
  Hadamard          forward and demb: one fp32 product, bit for bit; d3 (n + 1) u sum_n |dx| |emb|, a masked d3 exactly 0
  fractions         taus, tau_hat rtol 1e-5 + atol 1e-6 (what tests/test_gpu_reference_vectors.py holds a0_fqf_taus to); tau_hat the fp32 midpoint of the
                    kernel's own taus and a0_fqf_inner_taus its interior, bit for bit
  fraction loss     loss 16 u sum_i (|v1_i| + |v2_i|) tau_{i+1}; dlogits (F + 24) u 2 |w_b| S_b p_k + 1e-30, S_b = sum_i (|v1_i| + |v2_i|)
  cosine features   cosf against the float64 cosine of the same fp32 argument (|x| <= 64 pi < 202), absolute.  cosf's accuracy on this device is not
                    documented, so it is measured: test_cosine_features_against_float64 takes the largest deviation over all its cases and kernels.
                    COS_MEASURED = 6.5e-8 below is that figure on an MI355X (just over half an ulp of 1), COS_BOUND = 2^-22 twice it rounded up to a power of two;
                    the test asserts COS_BOUND.
Each test prints its largest error as a fraction of its tolerance (and records it with util.record_stats)."""
import numpy as np
import pytest
import torch

import quantile_ref as Q
import recipe
from util import assert_close, record_stats

pytestmark = pytest.mark.gpu

U = Q.U
GUARD = 64
SENT = -1.25e38                          # exact in fp32
NAN = float("nan")
COS_MEASURED = 6.5e-8                    # largest |cosf(x) - cos(x)| over the cases of test_cosine_features_against_float64 (MI355X)
COS_BOUND = 2.0 ** -22                   # twice that (1.3e-7), rounded up to a power of two (2.4e-7)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


# ------------------------------------------------------------------------------------------------ helpers
def _dev(hip, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(hip.device)


def _out(hip, n, fill=NAN, dtype=torch.float32):
    """n elements of ``fill`` followed by GUARD sentinels."""
    buf = hip.empty(n + GUARD, dtype=dtype)
    buf[:n].fill_(fill)
    buf[n:].fill_(SENT if dtype == torch.float32 else 0x5A5A5A5A)
    return buf


def _take(buf, n, what):
    torch.cuda.synchronize()
    guard = SENT if buf.dtype == torch.float32 else 0x5A5A5A5A
    assert bool((buf[n:] == guard).all()), f"{what}: write past the end"
    return buf[:n].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, want, what):
    got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ in their bits, first at {bad[:5]}"


def _judge(name, got, want, tol, what):
    """Every element within its tolerance (an element whose tolerance is 0 must be exact; an unwritten NaN fails); prints and records the worst ratio."""
    got, want, tol = (np.asarray(x, np.float64) for x in (got, want, tol))
    assert got.shape == want.shape == tol.shape, (what, got.shape, want.shape, tol.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements unwritten or not finite"
    err = np.abs(got - want)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    print(f"{name} {what}: largest error {worst:.3f} of its tolerance")
    record_stats(f"quantile_ref_{name}", {"what": what, "worst_error_over_tolerance": worst})
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert worst <= 1.0, f"{what}: element {i} off by {err[i]:.3e}, tolerance {tol[i]:.3e} (got {got[i]!r}, float64 {want[i]!r})"
    return worst


def _pad32(n):
    return -(-n // 32) * 32


# ------------------------------------------------------------------------------------------------ dueling combine
@pytest.mark.parametrize("extra", [0, 32])
@pytest.mark.parametrize("R,A,T,dueling", [(1, 1, 1, 0), (1, 1, 1, 1), (5, 4, 1, 1), (300, 6, 1, 0), (3, 18, 51, 1), (2, 3, 200, 1), (7, 2, 37, 1)])
def test_dueling_combine_against_float64(hip, R, A, T, dueling, extra):
    used = A * T + (T if dueling else 0)
    ld = _pad32(used) + extra
    g = recipe.gen(1000 + R + 7 * A + 13 * T + extra)
    raw = np.full((R, ld), np.nan, np.float32)                      # the padding is not to be read
    raw[:, :used] = g.standard_normal((R, used)).astype(np.float32) * 2 + 0.5
    go = g.standard_normal((R, A, T)).astype(np.float32)
    name = f"dueling_r{R}_a{A}_t{T}_d{dueling}_ld{ld}"
    # forward
    q = _out(hip, R * A * T)
    hip.dueling_fwd(_dev(hip, raw), ld, q, R, A, T, dueling)
    got_q = _take(q, R * A * T, "dueling_fwd").reshape(R, A, T)
    want_q, sq = Q.dueling_fwd64(raw, ld, R, A, T, dueling)
    tol_q = (A + 4) * U * sq
    if dueling:
        _judge(name + "_fwd", got_q, want_q, tol_q, "dueling forward")
    else:
        _same_bits(got_q, raw[:, :A * T], "dueling forward (copy)")
    # backward
    draw = _out(hip, R * ld)
    hip.dueling_bwd(_dev(hip, go), draw, ld, R, A, T, dueling)
    got_d = _take(draw, R * ld, "dueling_bwd").reshape(R, ld)
    want_d, sd = Q.dueling_bwd64(go, ld, R, A, T, dueling)
    tol_d = (A + 4) * U * sd
    _judge(name + "_bwd", got_d, want_d, tol_d, "dueling backward")
    assert (got_d[:, used:] == 0).all(), "dueling backward: pad columns must be exactly 0"
    if not dueling:
        _same_bits(got_d[:, :used], go.reshape(R, used), "dueling backward (copy)")
    # the backward is the forward's transpose
    x64, g64 = raw[:, :used].astype(np.float64), go.astype(np.float64)
    lhs, rhs = float((got_q.astype(np.float64) * g64).sum()), float((x64 * got_d[:, :used].astype(np.float64)).sum())
    bound = float((tol_q * np.abs(g64)).sum() + (tol_d[:, :used] * np.abs(x64)).sum())
    print(f"{name} transpose: |<fwd(x), g> - <x, bwd(g)>| = {abs(lhs - rhs) / max(bound, 1e-300):.3f} of its bound")
    assert abs(lhs - rhs) <= bound, f"dueling: <fwd(x), g> = {lhs!r}, <x, bwd(g)> = {rhs!r}, bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------ target quantiles
def _strides(layout, n, A):
    """(sb, s_quantile, sa) of [B][A][n] (QR) or [B][n][A] (IQN / FQF)."""
    return (A * n, 1, n) if layout == "qr" else (n * A, A, 1)


def _laid_out(full, layout):
    """full [B][A][n] as the flat tensor of the layout."""
    return np.ascontiguousarray(full if layout == "qr" else full.transpose(0, 2, 1)).reshape(-1)


def _actions(g, B, A):
    """B actions in [0, A) that hit 0 and A - 1."""
    a = g.integers(0, A, B).astype(np.int32)
    a[0] = 0
    a[-1] = A - 1
    if B > 2:
        a[1] = A - 1
    return a


@pytest.mark.parametrize("layout", ["qr", "iqn"])
@pytest.mark.parametrize("B,Nd,A", [(1, 1, 1), (3, 85, 4), (4, 64, 9), (257, 1, 2), (5, 200, 18)])
def test_quantile_target_against_float64(hip, B, Nd, A, layout):
    g = recipe.gen(2000 + B + Nd + A)
    gam = 0.99 ** 3
    sb, sj, sa = _strides(layout, Nd, A)
    qn = (g.standard_normal((B, A, Nd)) * 3).astype(np.float32)
    rew = g.standard_normal(B).astype(np.float32)
    a_star = _actions(g, B, A)
    dones = g.integers(0, 2, B).astype(np.float32)
    dones[0], dones[-1] = 1.0, 0.0
    if B > 2:
        dones[1], dones[2] = 0.0, 1.0                                # a* = A - 1 not done, and a done row in the middle
    worst = 0.0
    for done in ([dones] if B > 1 else [np.zeros(1, np.float32), np.ones(1, np.float32)]):      # B = 1: both values, one launch each
        assert (a_star == 0).any() and (a_star == A - 1).any() and (B == 1 or ((done == 0).any() and (done == 1).any()))
        y = _out(hip, B * Nd)
        hip.quantile_target(_dev(hip, _laid_out(qn, layout)), sb, sj, sa, _dev(hip, a_star), _dev(hip, rew), _dev(hip, done), gam, B, Nd, y)
        got = _take(y, B * Nd, "quantile_target").reshape(B, Nd)
        want, scale = Q.quantile_target64(_laid_out(qn, layout), sb, sj, sa, a_star, rew, done, gam, B, Nd)
        worst = max(worst, _judge(f"target_{layout}_b{B}_n{Nd}_a{A}", got, want, 3 * U * scale, "target quantiles"))
        on = done == 1
        _same_bits(got[on], np.broadcast_to(rew[on, None], (int(on.sum()), Nd)), "target quantiles of done rows (the reward)")


# ------------------------------------------------------------------------------------------------ quantile Huber
HUBER_PAIRS = [(1, 203), (63, 1), (64, 3), (65, 4), (255, 5), (256, 200), (257, 203), (300, 5), (8, 13), (64, 4)]        # (N, N')


def _huber_case(N, Nd, layout, per_sample, seed, B=4, A=3):
    g = recipe.gen(seed)
    full = (g.standard_normal((B, A, N)) * 1.5).astype(np.float32)
    y = (g.standard_normal((B, Nd)) * 1.5).astype(np.float32)
    act = _actions(g, B, A)
    # planted pairs (all exact in fp32): sample 0 an exact tie, sample 1 |d| == 1 with both signs, sample 2 |d| one ulp above 1, sample 3 one ulp below
    i0, j0, i1, j1 = 0, 0, N - 1, Nd - 1
    q075 = np.float32(0.75)
    full[0, act[0], i0] = y[0, j0]
    full[1, act[1], i0], y[1, j0] = q075, np.float32(1.75)                                   # d = -1
    if N > 1 and Nd > 1:
        full[1, act[1], i1], y[1, j1] = q075, np.float32(-0.25)                              # d = +1 (and (i0, j1): d = 1 too, (i1, j0): -1)
    full[2, act[2], i0], y[2, j0] = 0.0, np.nextafter(np.float32(1), np.float32(2))          # d = -(1 + 2^-23), one ulp beyond the seam
    full[3, act[3], i0], y[3, j0] = 0.0, np.nextafter(np.float32(1), np.float32(0))          # d = -(1 - 2^-24), one ulp inside it
    assert np.float32(full[2, act[2], i0] - y[2, j0]) == -np.float32(1 + 2.0 ** -23) and np.float32(full[3, act[3], i0] - y[3, j0]) == -np.float32(1 - 2.0 ** -24)
    if per_sample:
        taus, tb = g.random((B, N)).astype(np.float32), N
    else:
        taus, tb = ((2 * np.arange(N) + 1) / (2.0 * N)).astype(np.float32), 0
    w = g.uniform(0.2, 1.0, B).astype(np.float32)
    return full, y, act, taus, tb, w


def _run_huber(hip, full, y, act, taus, tb, w, layout):
    B, A, N = full.shape
    Nd = y.shape[1]
    sb, si, sa = _strides(layout, N, A)
    flat = _laid_out(full, layout)
    loss, dq, state = _out(hip, B), _out(hip, B * N * A, fill=SENT), hip.zeros(8, dtype=torch.int32)
    hip.loss_quantile_huber(_dev(hip, flat), sb, si, sa, _dev(hip, y), _dev(hip, taus), tb, _dev(hip, act), _dev(hip, w), B, N, Nd, loss, dq, state)
    got_loss, got_dq = _take(loss, B, "quantile huber loss"), _take(dq, B * N * A, "quantile huber dq")
    got_dq = got_dq.reshape(B, A, N) if layout == "qr" else got_dq.reshape(B, N, A).transpose(0, 2, 1)
    return got_loss, got_dq, state.cpu().numpy(), (flat, sb, si, sa)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared_taus", "per_sample_taus"])
@pytest.mark.parametrize("layout", ["qr", "iqn"])
@pytest.mark.parametrize("N,Nd", HUBER_PAIRS)
def test_quantile_huber_against_float64(hip, N, Nd, layout, per_sample):
    full, y, act, taus, tb, w = _huber_case(N, Nd, layout, per_sample, 3000 + 7 * N + Nd)
    B, A, _ = full.shape
    got_loss, got_dq, state, (flat, sb, si, sa) = _run_huber(hip, full, y, act, taus, tb, w, layout)
    loss, dq, dq_scale = Q.quantile_huber64(flat, sb, si, sa, y, taus, tb, act, w, B, N, Nd)
    name = f"huber_{layout}_n{N}_nd{Nd}_{'ps' if per_sample else 'sh'}"
    _judge(name + "_loss", got_loss, loss, (Nd + 12) * U * loss, "quantile Huber loss")
    taken = np.zeros((B, A, N), bool)
    taken[np.arange(B), act] = True
    _judge(name + "_dq", got_dq[np.arange(B), act], dq, (Nd + 4) * U * dq_scale, "quantile Huber dq at the taken action")
    assert (_bits(got_dq)[~taken] == _bits(np.float32(SENT))).all(), "dq at the other actions must be left alone"
    assert int(state[0]) == 0 and not state[1:].any(), f"status words {state}"


@pytest.mark.parametrize("layout", ["qr", "iqn"])
def test_quantile_huber_flags_a_nan_target(hip, layout):
    """One NaN among sample 2's targets: the status word becomes 1 and the NaN stays in that sample's loss."""
    N, Nd = 65, 5
    full, y, act, taus, tb, w = _huber_case(N, Nd, layout, True, 3999)
    y[2, 3] = np.nan
    B, A, _ = full.shape
    got_loss, got_dq, state, (flat, sb, si, sa) = _run_huber(hip, full, y, act, taus, tb, w, layout)
    assert int(state[0]) == 1, f"status words {state}"
    assert np.isnan(got_loss[2])
    keep = np.array([0, 1, 3])
    loss, dq, dq_scale = Q.quantile_huber64(flat, sb, si, sa, y, taus, tb, act, w, B, N, Nd)
    _judge(f"huber_nan_{layout}_loss", got_loss[keep], loss[keep], (Nd + 12) * U * loss[keep], "quantile Huber loss of the samples without a NaN")
    _judge(f"huber_nan_{layout}_dq", got_dq[keep, act[keep]], dq[keep], (Nd + 4) * U * dq_scale[keep], "quantile Huber dq of the samples without a NaN")


# ------------------------------------------------------------------------------------------------ cosine features
SPECIAL_TAUS = np.array([0.0, 0.5, 1 - 2.0 ** -24, 2.0 ** -24], np.float32)


def _tau_sets(R, seed):
    """Tau vectors of length R that between them hold 0, 0.5, 1 - 2^-24, 2^-24 and random values."""
    g = recipe.gen(seed)
    if R >= 4:
        t = g.random(R).astype(np.float32)
        t[:4] = SPECIAL_TAUS
        return [t] if R > 4 else [t, g.random(R).astype(np.float32)]
    sets = [np.roll(SPECIAL_TAUS, -k)[:R].copy() for k in range(0, 4, R)]
    return sets + [g.random(R).astype(np.float32)]


def test_cosine_features_against_float64(hip):
    """a0_cos_features, a0_tau_cos_features and the cos_out of a0_fqf_taus_cos against the float64 cosine of the fp32 argument each kernel forms
    (quantile_ref.cos_features64 on the kernel's own taus), as an absolute error over (R, D) = (1, 64), (4, 64), (5, 64), (3, 7), (1000, 64).
    Measured on an MI355X: largest deviation 6.45e-8 (cos_features 6.39e-8, tau_cos_features 6.45e-8, fqf_taus_cos 6.26e-8), recorded as COS_MEASURED =
    6.5e-8; asserted: COS_BOUND = 2^-22 (2.4e-7), twice the measured value (1.3e-7) rounded up to a power of two.  At tau = 0 the feature is cos(0) = 1 exactly."""
    worst = {}
    for R, D in [(1, 64), (4, 64), (5, 64), (3, 7), (1000, 64)]:
        for k, taus in enumerate(_tau_sets(R, 4000 + R + D)):
            out = _out(hip, R * D)
            hip.cos_features(_dev(hip, taus), out, R, D)
            got = _take(out, R * D, "cos_features").reshape(R, D)
            assert np.isfinite(got).all(), "cos_features: unwritten or not finite"
            worst["cos_features"] = max(worst.get("cos_features", 0.0), float(np.abs(got - Q.cos_features64(taus, D)).max()))
            assert (got[taus == 0] == 1.0).all()
        # drawn taus
        t_out, out = _out(hip, R), _out(hip, R * D)
        hip.tau_cos_features(97, 5, 13, t_out, out, R, D)
        t, got = _take(t_out, R, "tau_cos_features taus"), _take(out, R * D, "tau_cos_features").reshape(R, D)
        assert np.isfinite(got).all() and ((t >= 0) & (t < 1)).all(), "tau_cos_features: unwritten, not finite or outside [0, 1)"
        worst["tau_cos_features"] = max(worst.get("tau_cos_features", 0.0), float(np.abs(got - Q.cos_features64(t, D)).max()))
    for B, F, D in [(3, 33, 64), (2, 5, 7), (1, 64, 64)]:
        logits = recipe.gen(4100 + F).standard_normal((B, F)).astype(np.float32)
        taus, th, co = _out(hip, B * (F + 1)), _out(hip, B * F), _out(hip, B * F * D)
        hip.fqf_taus_cos(_dev(hip, logits), F, taus, th, co, D, B, F)
        t, got = _take(th, B * F, "fqf_taus_cos tau_hat"), _take(co, B * F * D, "fqf_taus_cos cos_out").reshape(B * F, D)
        assert np.isfinite(got).all() and np.isfinite(t).all()
        worst["fqf_taus_cos"] = max(worst.get("fqf_taus_cos", 0.0), float(np.abs(got - Q.cos_features64(t, D)).max()))
    top = max(worst.values())
    print(f"cosine features: largest |cosf - cos| {top:.4e} ({worst}); recorded {COS_MEASURED:.2e}, bound {COS_BOUND:.4e}: {top / COS_BOUND:.3f} of its tolerance")
    record_stats("quantile_ref_cosf", {"largest_abs_error": worst, "recorded": COS_MEASURED, "bound": COS_BOUND})
    assert top <= COS_BOUND, f"cosf deviates by {top:.3e} from the float64 cosine of its fp32 argument (bound {COS_BOUND:.3e}): {worst}"


@pytest.mark.parametrize("with_ctrl", [False, True])
@pytest.mark.parametrize("R,D", [(1, 64), (5, 64), (257, 64), (5, 7)])
def test_tau_cos_features_equals_rng_uniform_then_cos_features(hip, R, D, with_ctrl):
    """Bit for bit, taus and features, at an offset that is no multiple of four, by value and with the offset's second part read from a control word."""
    seed, stream, offset = 0x1234567, 3, 13
    ctrl = None
    if with_ctrl:
        ctrl = hip.zeros(8, dtype=torch.int64)
        ctrl[3] = 6                                                  # total offset 19
    t1, o1, t2, o2 = _out(hip, R), _out(hip, R * D), _out(hip, R), _out(hip, R * D)
    if with_ctrl:
        hip.tau_cos_features(seed, stream, offset, t1, o1, R, D, ctrl=ctrl, ctrl_idx=3)
        hip.rng_uniform_ctrl(seed, stream, offset, t2, R, ctrl, 3)
    else:
        hip.tau_cos_features(seed, stream, offset, t1, o1, R, D)
        hip.rng_uniform(seed, stream, offset, t2, R)
    hip.cos_features(t2, o2, R, D)
    a, b = _take(t1, R, "tau_cos_features taus"), _take(t2, R, "rng_uniform")
    assert np.isfinite(a).all() and ((a >= 0) & (a < 1)).all()
    _same_bits(a, b, "taus against rng_uniform")
    _same_bits(_take(o1, R * D, "tau_cos_features"), _take(o2, R * D, "cos_features"), "features against cos_features")
    if with_ctrl:                                                    # the control word really moved the stream
        t3 = _out(hip, R)
        hip.rng_uniform(seed, stream, offset + 6, t3, R)
        _same_bits(a, _take(t3, R, "rng_uniform"), "taus against rng_uniform at offset + ctrl")


@pytest.mark.parametrize("B,F,D,ld", [(3, 2, 64, 2), (3, 32, 64, 32), (2, 33, 7, 64), (1, 64, 64, 64), (3, 5, 7, 32)])
def test_fqf_taus_cos_equals_fqf_taus_then_cos_features(hip, B, F, D, ld):
    logits = np.full((B, ld), np.nan, np.float32)
    logits[:, :F] = recipe.gen(4200 + F).standard_normal((B, F)).astype(np.float32)
    lg = _dev(hip, logits)
    t1, h1, c1 = _out(hip, B * (F + 1)), _out(hip, B * F), _out(hip, B * F * D)
    t2, h2, c2 = _out(hip, B * (F + 1)), _out(hip, B * F), _out(hip, B * F * D)
    hip.fqf_taus_cos(lg, ld, t1, h1, c1, D, B, F)
    hip.fqf_taus(lg, ld, t2, h2, B, F)
    hip.cos_features(h2, c2, B * F, D)
    a = _take(t1, B * (F + 1), "fqf_taus_cos taus")
    assert np.isfinite(a).all()
    _same_bits(a, _take(t2, B * (F + 1), "fqf_taus taus"), "taus")
    _same_bits(_take(h1, B * F, "fqf_taus_cos tau_hat"), _take(h2, B * F, "fqf_taus tau_hat"), "tau_hat")
    c = _take(c1, B * F * D, "fqf_taus_cos cos_out")
    assert np.isfinite(c).all()
    _same_bits(c, _take(c2, B * F * D, "cos_features"), "cos_out against cos_features(tau_hat)")


# ------------------------------------------------------------------------------------------------ Hadamard product
@pytest.mark.parametrize("B,n,D", [(1, 1, 4), (3, 5, 12), (2, 32, 3136), (43, 64, 3136)])
def test_hadamard_forward_is_the_fp32_product(hip, B, n, D):
    """(43, 64, 3136): 2 157 568 16-byte elements, more than the grid's 8192 x 256 threads: the grid-stride loop takes a second trip."""
    g = recipe.gen(5000 + B)
    emb = g.standard_normal((B, n, D), dtype=np.float32)
    feat = g.standard_normal((B, D), dtype=np.float32)
    emb[0, 0, 0], feat[0, 1] = 0.0, -0.0
    x = _out(hip, B * n * D)
    hip.hadamard_fwd(_dev(hip, emb), _dev(hip, feat), x, B, n, D)
    _same_bits(_take(x, B * n * D, "hadamard_fwd"), Q.hadamard_fwd32(emb, feat, B, n, D), "hadamard forward")


@pytest.mark.parametrize("B,n,D", [(1, 1, 4), (3, 5, 85), (4, 3, 64), (257, 2, 1), (2, 64, 3136)])
def test_hadamard_backward_against_float64(hip, B, n, D):
    g = recipe.gen(5100 + B + n)
    emb = np.maximum(g.standard_normal((B, n, D)), 0).astype(np.float32)          # ReLU outputs: about half exact zeros
    feat = np.maximum(g.standard_normal((B, D)), 0).astype(np.float32)
    dx = g.standard_normal((B, n, D)).astype(np.float32)
    # planted 0, -0.0 and negative values in both masks (cyclic positions, so that the smallest case holds some too)
    fe, ff = emb.reshape(-1), feat.reshape(-1)
    for k, v in enumerate((0.0, -0.0, -0.75, 1.5)):
        fe[(3 * k + 1) % fe.size] = v
    for k, v in enumerate((1.25, 0.0, -0.0, -0.5)):
        ff[(5 * k) % ff.size] = v
    demb, d3 = _out(hip, B * n * D), _out(hip, B * D)
    hip.hadamard_bwd(_dev(hip, dx), _dev(hip, emb), _dev(hip, feat), demb, d3, B, n, D)
    got_e, got_3 = _take(demb, B * n * D, "hadamard_bwd demb").reshape(B, n, D), _take(d3, B * D, "hadamard_bwd d3").reshape(B, D)
    want_e, want_3, s3 = Q.hadamard_bwd64(dx, emb, feat, B, n, D)
    _same_bits(got_e, want_e, "demb")
    _judge(f"hadamard_bwd_b{B}_n{n}_d{D}", got_3, want_3, (n + 1) * U * s3, "d3")
    masked = ~(feat > 0)
    assert masked.any() and (got_3[masked] == 0).all(), "a masked d3 must be exactly 0"


# ------------------------------------------------------------------------------------------------ fraction proposal
def _logit_sets(g, B, F):
    rnd = g.standard_normal((B, F)).astype(np.float32)
    peak = g.standard_normal((B, F)).astype(np.float32)
    peak[np.arange(B), g.integers(0, F, B)] += np.float32(80.0)      # its probability rounds to 1, the others underflow towards 0
    return {"scale1": rnd, "equal": np.full((B, F), 0.37, np.float32), "peak80": peak, "scale10": (rnd * 10).astype(np.float32)}


def _fqf_lds(F):
    """ld = F and the padded width, 32 below F = 32 and 64 from there on (F = 64 leaves no padding)."""
    return sorted({F, 32 if F < 32 else 64})


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [2, 3, 31, 32, 33, 63, 64])
def test_fqf_taus_against_float64(hip, F, B):
    """ld = F and ld = the padded width (32 or 64) with NaN in the padding, four logit sets each."""
    g = recipe.gen(6000 + 10 * F + B)
    worst = 0.0
    for name, lg in _logit_sets(g, B, F).items():
        for ld in _fqf_lds(F):
            logits = np.full((B, ld), np.nan, np.float32)
            logits[:, :F] = lg
            taus, th = _out(hip, B * (F + 1)), _out(hip, B * F)
            hip.fqf_taus(_dev(hip, logits), ld, taus, th, B, F)
            t, h = _take(taus, B * (F + 1), "fqf_taus taus").reshape(B, F + 1), _take(th, B * F, "fqf_taus tau_hat").reshape(B, F)
            what = f"F={F} B={B} ld={ld} {name}"
            assert np.isfinite(t).all() and np.isfinite(h).all(), f"{what}: unwritten or not finite (was the padding read?)"
            want_t, want_h, _ = Q.fqf_taus64(logits, ld, B, F)
            assert_close(t, want_t, 1e-5, 1e-6, f"taus {what}")
            assert_close(h, want_h, 1e-5, 1e-6, f"tau_hat {what}")
            worst = max(worst, float((np.abs(t - want_t) / (1e-6 + 1e-5 * np.abs(want_t))).max()), float((np.abs(h - want_h) / (1e-6 + 1e-5 * np.abs(want_h))).max()))
            assert (_bits(t[:, 0]) == 0).all(), f"{what}: taus[b][0] must be +0"
            assert (np.diff(t, axis=1) >= 0).all(), f"{what}: taus must not decrease"
            assert (t[:, F] <= 1 + 1e-5).all(), f"{what}: taus[b][F] = {t[:, F]}"
            _same_bits(h, (t[:, :-1] + t[:, 1:]) / np.float32(2), f"{what}: tau_hat against the fp32 midpoints of the kernel's taus")
    print(f"fqf_taus F={F} B={B}: largest error {worst:.3f} of its tolerance")
    record_stats(f"quantile_ref_fqf_taus_f{F}_b{B}", {"worst_error_over_tolerance": worst})


@pytest.mark.parametrize("B,F", [(1, 2), (8, 33), (5, 52), (257, 2), (3, 64)])
def test_fqf_inner_taus_is_the_interior(hip, B, F):
    taus = recipe.gen(6500 + B).random((B, F + 1)).astype(np.float32)
    out = _out(hip, B * (F - 1))
    hip.fqf_inner_taus(_dev(hip, taus), out, B, F)
    got = _take(out, B * (F - 1), "fqf_inner_taus")
    assert np.isfinite(got).all()
    _same_bits(got, taus[:, 1:-1], "taus[:, 1:-1]")


# ------------------------------------------------------------------------------------------------ fraction loss
def _fraction_q_sets(g, B, F, A):
    """(q [B][F-1][A], qh [B][F][A]) monotone along the fractions and interleaved as quantile values are, unsorted, and with exact ties."""
    both = np.sort((g.standard_normal((B, 2 * F - 1, A)) * 2).astype(np.float32), 1)
    mono = (np.ascontiguousarray(both[:, 1::2]), np.ascontiguousarray(both[:, 0::2]))            # qh_0 <= q_0 <= qh_1 <= ... <= qh_{F-1}
    uns = ((g.standard_normal((B, F - 1, A)) * 2).astype(np.float32), (g.standard_normal((B, F, A)) * 2).astype(np.float32))
    tq, th = mono[0].copy(), mono[1].copy()
    tq[:, 0] = th[:, 0]                                                                          # q_0 == qh_0 (prev of i = 0)
    tq[:, -1] = th[:, -1] if F > 2 else tq[:, -1]                                                # q_{F-2} == qh_{F-1} (next of i = F - 2)
    if F > 3:
        tq[:, 2] = tq[:, 1]                                                                      # q_i == q_{i-1}
    return {"monotone": mono, "unsorted": uns, "ties": (tq, th)}


@pytest.mark.parametrize("padded", [False, True], ids=["ldl_F", "ldl_padded"])
@pytest.mark.parametrize("A", [1, 4, 18])
@pytest.mark.parametrize("F", [2, 3, 32, 33, 63, 64])
def test_fqf_fraction_loss_against_float64(hip, F, A, padded):
    """ldl = F and ldl = 32 / 64 with NaN logits in the padding; sample 2 has w = 0: its gradient is all zero."""
    B = 4
    ldl = F if not padded else (32 if F < 32 else 64)
    g = recipe.gen(7000 + 20 * F + A)
    logits = np.full((B, ldl), np.nan, np.float32)
    logits[:, :F] = g.standard_normal((B, F)).astype(np.float32)
    taus = Q.fqf_taus64(logits, ldl, B, F)[0].astype(np.float32)                                 # the float64 cumsum rounded to fp32
    act = _actions(g, B, A)
    w = g.uniform(0.2, 1.0, B).astype(np.float32)
    w[2] = 0.0
    for name, (q, qh) in _fraction_q_sets(g, B, F, A).items():
        loss, dl = _out(hip, B), _out(hip, B * ldl)
        hip.fqf_fraction_loss(_dev(hip, q), _dev(hip, qh), _dev(hip, taus), _dev(hip, act), _dev(hip, w), B, F, A, ldl, loss, dl, _dev(hip, logits))
        got_l, got_d = _take(loss, B, "fqf_fraction_loss loss"), _take(dl, B * ldl, "fqf_fraction_loss dlogits").reshape(B, ldl)
        ref = Q.fqf_fraction64(q, qh, taus, act, w, logits, ldl, B, F, A)
        tag = f"fraction_f{F}_a{A}_ldl{ldl}_{name}"
        _judge(tag + "_loss", got_l, ref["loss"], 16 * U * ref["loss_scale"], f"fraction loss ({name})")
        tol = (F + 24) * U * 2 * np.abs(w.astype(np.float64))[:, None] * ref["S"][:, None] * ref["p"] + 1e-30
        _judge(tag + "_dlogits", got_d[:, :F], ref["dlogits"], tol, f"fraction-loss dlogits ({name})")
        assert (got_d[:, F:] == 0).all(), "dlogits[:, F:ldl] must be exactly 0"
        assert (got_d[2] == 0).all(), "w_b = 0: the gradient must be all zero"
        assert np.abs(ref["dlogits"][[0, 1, 3]]).max() > 0, "the case has no gradient to judge"
