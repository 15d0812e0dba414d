"""CPU: tests/hl_gauss_ref.py, the float64 yardstick of tests/test_gpu_hl_gauss.py, held to closed forms of the HL-Gauss target (Farebrother et al. 2024) and
told apart from six wrong computations — before any device run, so that the bound the kernel is judged by is not fitted to the kernel."""
import math

import numpy as np
import pytest

import hl_gauss_ref as H

T, A = 51, 4
ATOMS = H.c51_atoms(H.VMIN, H.VMAX, T)
DELTA = (H.VMAX - H.VMIN) / (T - 1)


def _terminal(y, T=T, vmin=H.VMIN, vmax=H.VMAX, rho=0.75):
    """The reference on terminals whose rewards are y: y itself is the target."""
    y = np.atleast_1d(np.asarray(y, np.float32))
    B = len(y)
    z = np.zeros((B, 1, T), np.float32)
    return H.hl_gauss64(z, 1, T, np.zeros(B, np.int32), y, np.ones(B, np.float32), H.c51_atoms(vmin, vmax, T), H.GAMMA, vmin, vmax, rho, B)


def _all_cases():
    for Tn in H.TS:
        for An in H.AS:
            for B, shift in H.launches(Tn, An):
                yield Tn, An, B, H.case(Tn, An, B, shift)


def _ref(c, Tn, An, B, rho, **kw):
    return H.hl_gauss64(c["tgt_logits"], An, Tn, c["a_star"], c["rew"], c["done"], c["atoms"], H.GAMMA, c["vmin"], c["vmax"], rho, B, **kw)


def test_the_mass_sums_to_one_and_is_positive():
    for Tn, An, B, c in _all_cases():
        for rho in H.rhos(Tn):
            ref = _ref(c, Tn, An, B, rho)
            assert not ref["nan_rows"].any()
            assert np.abs(ref["m"].sum(-1) - 1.0).max() < 1e-14 and (ref["m"] >= 0).all()
            assert (ref["e_m"] > 0).all() and np.isfinite(ref["e_m"]).all()
            assert ref["e_m"].max() < 1e-3, "the bound stays a bound on an fp32 evaluation, not a tolerance"


def test_symmetric_about_an_interior_centre():
    Ts, lo, hi = 33, -8.0, 8.0                                  # Delta = 0.5: atoms and edges are exact in fp32
    for k in (1, 10, 16, 31):
        m = _terminal(lo + 0.5 * k, T=Ts, vmin=lo, vmax=hi)["m"][0]
        n = min(k, Ts - 1 - k)
        for j in range(1, n + 1):
            assert m[k + j] == pytest.approx(m[k - j], rel=1e-9, abs=1e-15)      # a mass is a difference of two Phi values of up to 1: a few 2^-53 absolute
        assert m.argmax() == k


def test_one_hot_as_the_ratio_goes_to_zero_and_a_two_bin_split_on_an_edge():
    m = _terminal(ATOMS[20], rho=1e-3)["m"][0]
    assert m[20] == 1.0 and m.sum() == 1.0
    edge = np.float32(H.VMIN - 0.5 * DELTA + 21 * DELTA)           # between bins 20 and 21, as an fp32 number
    m = _terminal(edge, rho=1e-3)["m"][0]
    assert m[20] + m[21] == pytest.approx(1.0, abs=1e-12) and m[20] == pytest.approx(0.5, abs=1e-3) and m[21] == pytest.approx(0.5, abs=1e-3)
    m = _terminal(edge, rho=0.75)["m"][0]
    assert m[20] == pytest.approx(m[21], rel=1e-4) and m[19] == pytest.approx(m[22], rel=1e-4)


def test_the_target_is_clamped_at_both_ends():
    lo, at_lo, hi, at_hi = (_terminal(v) for v in (-37.5, H.VMIN, 1e6, H.VMAX))
    assert lo["y"][0] == H.VMIN and hi["y"][0] == H.VMAX and lo["y_raw"][0] == -37.5
    assert np.array_equal(lo["m"], at_lo["m"]) and np.array_equal(hi["m"], at_hi["m"])
    assert np.allclose(at_lo["m"][0], at_hi["m"][0, ::-1], rtol=1e-9, atol=1e-15), "the support is symmetric, so are the two ends"
    assert at_lo["m"][0].argmax() == 0 and 0.5 < at_lo["Z"][0] < 0.76, "half a bin inside the outer edge: the normaliser is Phi(big) - Phi(-0.5 / 0.75)"
    assert at_lo["Z"][0] == pytest.approx(0.5 * (1 + math.erf(0.5 / 0.75 / math.sqrt(2))), rel=1e-12)


def test_a_terminal_ignores_the_next_state():
    c = H.case(T, A, 5, 0)
    done = np.ones(5, np.float32)
    a = H.hl_gauss64(c["tgt_logits"], A, T, c["a_star"], c["rew"], done, c["atoms"], H.GAMMA, H.VMIN, H.VMAX, 0.75, 5)
    b = H.hl_gauss64(c["online_next"] * 3, A, T, (c["a_star"] + 1) % A, c["rew"], done, c["atoms"], H.GAMMA, H.VMIN, H.VMAX, 0.75, 5)
    assert np.array_equal(a["m"], b["m"])
    live = H.hl_gauss64(c["tgt_logits"], A, T, c["a_star"], c["rew"], np.zeros(5, np.float32), c["atoms"], H.GAMMA, H.VMIN, H.VMAX, 0.75, 5)
    assert not np.array_equal(live["m"], a["m"])
    # the expectation, against a literal restatement
    x = c["tgt_logits"][np.arange(5), c["a_star"]].astype(np.float64)
    p = np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    assert np.allclose(live["v"], (p * c["atoms"].astype(np.float64)).sum(-1), rtol=1e-12)
    assert np.allclose(live["y_raw"], c["rew"].astype(np.float64) + float(np.float32(H.GAMMA)) * live["v"], rtol=1e-12)


def test_two_bins_by_hand():
    """T = 2 on [-1, 1]: Delta = 2, edges -2, 0, 2; rho = 0.5: sigma = 1.  A terminal with r = 0.5."""
    ref = _terminal(0.5, T=2, vmin=-1.0, vmax=1.0, rho=0.5)
    P = lambda u: 0.5 * (1 + math.erf(u / math.sqrt(2)))
    Z = P(1.5) - P(-2.5)
    assert ref["sigma"] == 1.0 and ref["Z"][0] == pytest.approx(Z, rel=1e-14)
    assert ref["m"][0, 0] == pytest.approx((P(-0.5) - P(-2.5)) / Z, rel=1e-13) and ref["m"][0, 1] == pytest.approx((P(1.5) - P(-0.5)) / Z, rel=1e-13)
    assert ref["m"][0, 0] == pytest.approx(0.32614, abs=1e-5) and ref["m"][0, 1] == pytest.approx(0.67386, abs=1e-5), "from a table of Phi: 0.30854, 0.00621, 0.93319"


def test_the_derivative_in_the_bound_is_the_derivative():
    y = np.float32(1.2345)
    h = 2.0 ** -12
    a, b, mid = _terminal(np.float32(y - h)), _terminal(np.float32(y + h)), _terminal(y)
    num = (b["m"][0] - a["m"][0]) / (2 * h)
    assert np.allclose(num, mid["dm"][0], rtol=1e-4, atol=1e-9)


def test_the_loss_and_its_gradient():
    c = H.case(T, A, 5, 5)
    ref = H.hl_gauss_loss64(c["logits"], c["tgt_logits"], A, T, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], c["atoms"], H.GAMMA, H.VMIN, H.VMAX, 0.75, 5)
    x = c["logits"][np.arange(5), c["act"]].astype(np.float64)
    logp = x - np.log(np.exp(x).sum(-1, keepdims=True))
    assert np.allclose(ref["loss"], -(ref["m"] * logp).sum(-1), rtol=1e-12)
    assert np.allclose(ref["g"], c["wgt"].astype(np.float64)[:, None] * (np.exp(logp) - ref["m"]), atol=1e-12), "sum(m) = 1: softmax - m"
    assert np.array_equal(ref["dlogits"][np.arange(5), c["act"]], ref["g"]) and np.count_nonzero(ref["dlogits"]) == np.count_nonzero(ref["g"]) and (ref["tol_loss"] > 0).all() and (ref["tol_g"] > 0).all()
    assert ref["tol_loss"].max() < 1e-2 and ref["tol_g"].max() < 1e-3


def test_a_nan_reward_stays_in_its_sample():
    c = H.case(T, A, 5, 0)
    rew = c["rew"].copy()
    rew[3] = np.nan
    ref = H.hl_gauss_loss64(c["logits"], c["tgt_logits"], A, T, c["act"], c["a_star"], rew, c["done"], c["wgt"], c["atoms"], H.GAMMA, H.VMIN, H.VMAX, 0.75, 5)
    assert ref["nan_rows"].tolist() == [False, False, False, True, False]
    assert np.isnan(ref["m"][3]).all() and np.isnan(ref["loss"][3]) and np.isfinite(np.delete(ref["m"], 3, 0)).all() and np.isfinite(np.delete(ref["loss"], 3)).all()


@pytest.mark.parametrize("variant", H.VARIANTS)
def test_a_wrong_computation_lies_far_outside_the_bound(variant):
    """Each of the six, somewhere on the GPU test's own inputs, by more than 100 bounds; and the cases hit every kind of sample."""
    worst, kinds = 0.0, set()
    for Tn, An, B, c in _all_cases():
        kinds |= set(c["kinds"])
        for rho in H.rhos(Tn):
            ref = _ref(c, Tn, An, B, rho)
            bad = _ref(c, Tn, An, B, rho, variant=variant, online_next=c["online_next"])
            worst = max(worst, float((np.abs(bad["m"] - ref["m"]) / ref["e_m"]).max()))
    assert kinds == set(H.KINDS)
    assert worst > 100.0, f"{variant}: at most {worst:.3g} bounds away"
