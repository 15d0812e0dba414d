"""CPU: tests/miqn_ref.py, the yardstick of tests/test_gpu_miqn.py, held to (1) a literal torch float64 restatement of the paper's Munchausen-IQN target, (2) closed
forms, (3) six wrong computations, each of which must lie more than a hundred bounds away from the reference on the very cases the GPU test runs, and (4) an fp32
restatement in numpy, which must lie inside the bound (a bound an honest fp32 evaluation misses would be no bound)."""
import numpy as np
import pytest
import torch

import miqn_ref as M

ALL = [(B, Nd, A, tau) for (B, Nd, A) in M.SHAPES for tau in M.TAUS]


def _ref(c, B, Nd, A, tau, layout="bja", alpha=M.ALPHA, lo=M.LO, q_cur=None, done=None):
    sb, sj, sa = M.strides(layout, Nd, A)
    return M.miqn_target64(M.laid_out(c["q_next"], layout), M.laid_out(c["q_cur"] if q_cur is None else q_cur, layout), sb, sj, sa, c["act"], c["rew"],
                           c["done"] if done is None else done, M.GAMMA, tau, alpha, lo, B, Nd, A)


def _paper(zn, zc, act, rew, done, gamma_n, tau, alpha, lo):
    """Vieillard et al. 2020, appendix B, in torch float64: pi = softmax(mean_j z_j / tau), the bonus alpha [tau log pi(a|s)] clipped to [lo, 0], and the soft
    target sum_a' pi(a'|s') (z'_j(a') - tau log pi(a'|s'))."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    zn, zc = t(zn), t(zc)
    gam, tau, alpha, lo = (float(np.float32(v)) for v in (gamma_n, tau, alpha, lo))
    logpi_n = torch.log_softmax(zn.mean(1) / tau, dim=-1)                      # [B][A]
    logpi_c = torch.log_softmax(zc.mean(1) / tau, dim=-1)
    bonus = (tau * logpi_c.gather(1, torch.from_numpy(np.asarray(act, np.int64))[:, None])).clamp(lo, 0.0)          # [B][1]
    soft = (logpi_n.exp()[:, None, :] * (zn - tau * logpi_n[:, None, :])).sum(-1)                                      # [B][N']
    return (t(rew)[:, None] + alpha * bonus + gam * (1.0 - t(done))[:, None] * soft).numpy()


@pytest.mark.parametrize("B,Nd,A,tau", ALL, ids=str)
@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_reference_is_the_papers_target(B, Nd, A, tau, layout):
    c = M.case(B, Nd, A, tau)
    ref = _ref(c, B, Nd, A, tau, layout)
    want = _paper(c["q_next"], c["q_cur"], c["act"], c["rew"], c["done"], M.GAMMA, tau, M.ALPHA, M.LO)
    assert ref["y"].shape == (B, Nd) and not ref["nan_rows"].any()
    err = np.abs(ref["y"] - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), err
    assert (ref["e_y"] > 0).all() and np.isfinite(ref["e_y"]).all()


def test_the_cases_meet_every_planted_kind_and_the_seams():
    seen = set()
    for (B, Nd, A, tau) in ALL:
        c = M.case(B, Nd, A, tau)
        ref = _ref(c, B, Nd, A, tau)
        for b, kind in c["planted"].items():
            if A == 1 and kind != "done":
                continue
            seen.add(kind)
            a = int(c["act"][b])
            if kind == "tie":
                o = (a + 1) % A
                assert np.array_equal(c["q_next"][b, :, a], c["q_next"][b, :, o]) and np.array_equal(c["q_cur"][b, :, a], c["q_cur"][b, :, o])
                assert ref["q_next_mean"][b, a] == ref["q_next_mean"][b].max() and ref["q_cur_mean"][b, a] == ref["q_cur_mean"][b].max()
            elif kind == "gap10":
                srt = np.sort(ref["q_next_mean"][b])
                assert srt[-1] - srt[-2] >= 10.0
                if tau == 0.03:
                    assert np.sort(ref["pi"][b])[-2] < 2.0 ** -149, "every other exponential is below the smallest fp32 number: pi' is one-hot in fp32"
            elif kind == "argmax":
                assert -1e-6 < ref["lp_cur"][b, a] <= 0.0 and abs(ref["m"][b]) < 1e-6, "the bonus sits at the upper seam"
            elif kind == "below_lo":
                assert ref["lp_cur"][b, a] < M.LO - 0.5 and ref["m"][b] == float(np.float32(M.ALPHA)) * M.LO, "the bonus sits at the lower seam"
            elif kind == "done":
                assert c["done"][b] == 1.0
    assert seen == set(M.KINDS), seen


def test_closed_forms():
    g = np.random.default_rng(5)
    gam = float(np.float32(M.GAMMA))
    for (B, Nd, A, tau) in ALL:
        c = M.case(B, Nd, A, tau)
        r, d = c["rew"].astype(np.float64)[:, None], c["done"].astype(np.float64)[:, None]
        t32, a32 = float(np.float32(tau)), float(np.float32(M.ALPHA))
        # all actions equal: pi uniform, lp = -tau log A
        col = (g.standard_normal((B, Nd, 1)) * 2).astype(np.float32)
        eq = dict(c, q_next=np.repeat(col, A, 2), q_cur=np.repeat((col * 0.5).astype(np.float32), A, 2))
        want = r + a32 * np.clip(-t32 * np.log(A), M.LO, 0.0) + gam * (1 - d) * (col[:, :, 0].astype(np.float64) + t32 * np.log(A))
        assert np.abs(_ref(eq, B, Nd, A, tau)["y"] - want).max() < 1e-12 * 20
        # lo = 0 or alpha = 0: no bonus; done = 1: y = r + m
        base = _ref(c, B, Nd, A, tau)
        for kw in (dict(lo=0.0), dict(alpha=0.0)):
            nb = _ref(c, B, Nd, A, tau, **kw)
            assert (nb["m"] == 0).all()
            assert np.abs((base["y"] - base["m"][:, None]) - nb["y"]).max() < 1e-12 * 20
        dn = _ref(c, B, Nd, A, tau, done=np.ones(B, np.float32))
        assert np.array_equal(dn["y"], np.broadcast_to(r + dn["m"][:, None], (B, Nd)))
        if A == 1:
            assert np.abs(base["y"] - (r + gam * (1 - d) * c["q_next"][:, :, 0].astype(np.float64))).max() < 1e-12 * 20


def test_nan_rows_are_marked_and_stay_alone():
    B, Nd, A, tau = 4, 64, 18, 0.03
    c = M.case(B, Nd, A, tau)
    zc = c["q_cur"].copy()
    zc[2, 5, 3] = np.nan
    ref = _ref(c, B, Nd, A, tau, q_cur=zc)
    clean = _ref(c, B, Nd, A, tau)
    assert ref["nan_rows"].tolist() == [False, False, True, False] and np.isnan(ref["y"][2]).all()
    keep = [0, 1, 3]
    assert np.array_equal(ref["y"][keep], clean["y"][keep])


@pytest.mark.parametrize("tau", M.TAUS)
def test_wrong_computations_lie_a_hundred_bounds_away(tau):
    """On the GPU test's own cases.  temp1 at tau = 1 is the reference itself; a head of one action has no policy to get wrong; N' = 1 has no fractions to differ."""
    worst = {v: 0.0 for v in M.VARIANTS}
    for (B, Nd, A) in M.SHAPES:
        if A == 1:
            continue
        c = M.case(B, Nd, A, tau)
        ref = _ref(c, B, Nd, A, tau)
        for v in M.VARIANTS:
            y = M.variant64(v, c["q_next"], c["q_cur"], c["q_online"], c["act"], c["rew"], c["done"], M.GAMMA, tau, M.ALPHA, M.LO)
            ratio = float((np.abs(y - ref["y"]) / ref["e_y"]).max())
            print(f"tau={tau} (B, N', A)={(B, Nd, A)} {v}: {ratio:.3g} bounds")
            worst[v] = max(worst[v], ratio)
    for v, ratio in worst.items():
        if v == "temp1" and tau == 1.0:
            assert ratio < 1e-6, "at temperature 1 the two softmaxes are the same"
            continue
        assert ratio > 100.0, f"{v} at tau={tau}: only {ratio:.3g} bounds away"


def _fp32_restatement(zn, zc, act, rew, done, gamma_n, tau, alpha, lo):
    """The formulas in numpy fp32, one operation at a time (means summed in j order)."""
    f = np.float32
    B, Nd, A = zn.shape
    tau, alpha, lo, gam = f(tau), f(alpha), f(lo), f(gamma_n)
    y = np.zeros((B, Nd), f)

    def parts(z):
        s = np.zeros(A, f)
        for j in range(Nd):
            s = (s + z[j]).astype(f)
        x = (s / f(Nd)).astype(f)
        zz = (x - x.max()).astype(f)
        e = np.exp((zz / tau).astype(f)).astype(f)
        se = f(0)
        for k in range(A):
            se = f(se + e[k])
        lp = (zz - tau * np.log(se).astype(f)).astype(f)
        return lp, (e / se).astype(f)

    with np.errstate(under="ignore"):
        for b in range(B):
            lpn, pi = parts(zn[b])
            lpc, _ = parts(zc[b])
            m = f(alpha * min(max(lpc[act[b]], lo), f(0)))
            g = f(gam * f(f(1) - done[b]))
            for j in range(Nd):
                acc = f(0)
                for k in range(A):
                    acc = f(acc + f(pi[k] * f(zn[b, j, k] - lpn[k])))
                y[b, j] = f(f(rew[b] + m) + f(g * acc))
    return y


@pytest.mark.parametrize("B,Nd,A,tau", ALL, ids=str)
def test_an_fp32_evaluation_lies_inside_the_bound(B, Nd, A, tau):
    c = M.case(B, Nd, A, tau)
    ref = _ref(c, B, Nd, A, tau)
    got = _fp32_restatement(c["q_next"], c["q_cur"], c["act"], c["rew"], c["done"], M.GAMMA, tau, M.ALPHA, M.LO)
    share = float((np.abs(got.astype(np.float64) - ref["y"]) / ref["e_y"]).max())
    print(f"(B, N', A)={(B, Nd, A)} tau={tau}: the fp32 restatement uses {share:.3f} of the bound")
    assert share <= 1.0
