"""CPU: the float64 restatement of ``learner.iqn.risk``'s distortions (tests/iqn_risk_ref.py) held to what the formulas must satisfy, before any device run."""
import math

import numpy as np
import pytest

import iqn_risk_ref as ref

TAUS = ref.fractions(4 + 4096).astype(np.float64)
# every (kind, eta) of the paper and of the range ends at which the distortion is monotone: cpw (Tversky-Kahneman's weighting function) is not below eta ~ 0.279
CASES = [(k, e) for k in ("cvar", "pow", "cpw", "wang") for e in ref.PAPER_ETA[k] + ref.RANGE_ENDS[k] if not (k == "cpw" and e < 0.28)] + [("cpw", 0.3)]


def test_the_inputs_are_the_edges_and_grid_fractions():
    assert tuple(TAUS[:4]) == ref.EDGES and TAUS.size == 4100
    k = TAUS * 2.0 ** 24
    assert np.all(k == np.floor(k)) and TAUS.min() == 0.0 and TAUS.max() < 1.0 and np.unique(TAUS).size > 4000


@pytest.mark.parametrize("kind,eta", CASES)
def test_zero_stays_zero_and_beta_is_monotone_within_the_unit_interval(kind, eta):
    assert ref.beta(kind, eta, 0.0) == 0.0
    t = np.sort(TAUS)
    b = ref.beta_array(kind, eta, t)
    assert np.all(np.isfinite(b)) and b.min() >= 0.0 and b.max() <= 1.0
    assert np.all(np.diff(b) >= 0.0), "monotone"
    distinct = np.diff(t) > 0
    if not (kind == "wang" and abs(eta) == 8.0):      # (at |eta| = 8 one tail saturates in double)
        assert np.all(np.diff(b)[distinct] > 0.0), "strictly, where the fractions differ"


def test_the_identities_are_exact():
    assert np.array_equal(ref.beta_array("cvar", 1.0, TAUS), TAUS)
    assert np.array_equal(ref.beta_array("pow", 0.0, TAUS), TAUS)
    assert np.array_equal(ref.beta_array("pow", -0.0, TAUS), TAUS)
    assert np.array_equal(ref.beta_array("cpw", 1.0, TAUS), TAUS), "tau + (1 - tau) is exact on the 2^-24 grid"
    assert np.array_equal(ref.beta_array("neutral", 3.0, TAUS), TAUS)
    assert np.array_equal(ref.cvar_f32(1.0, TAUS), TAUS.astype(np.float32))


def test_known_values():
    assert ref.ncdf(0.0) == 0.5 and ref.ncdfinv(0.5) == 0.0
    assert ref.ncdfinv(0.975) == pytest.approx(1.959963984540054, rel=1e-14)
    assert ref.ncdfinv(2.0 ** -24) == pytest.approx(-5.2947, abs=1e-4) and ref.ncdf(ref.ncdfinv(2.0 ** -24)) == pytest.approx(2.0 ** -24, rel=1e-13)
    assert ref.ncdf(-8.0) == pytest.approx(6.220960574271785e-16, rel=1e-13)
    assert ref.beta("pow", -2.0, 0.5) == pytest.approx(1.0 - 0.5 ** (1.0 / 3.0), rel=1e-15)
    assert ref.beta("pow", 2.0, 0.125) == pytest.approx(0.5, rel=1e-15)
    assert ref.beta("cpw", 0.71, 0.5) == pytest.approx(0.5 ** 0.71 / (2 * 0.5 ** 0.71) ** (1 / 0.71), rel=1e-15)
    assert ref.beta("wang", 0.75, 0.5) == pytest.approx(ref.ncdf(0.75), rel=1e-15) and ref.beta("wang", -0.75, 0.5) == pytest.approx(1.0 - ref.ncdf(0.75), rel=1e-14)
    assert ref.beta("cvar", 0.25, 0.5) == 0.125


def test_risk_averse_settings_move_the_fractions_down():
    t = TAUS[TAUS > 0]
    for kind, eta in (("cvar", 0.25), ("pow", -2.0), ("wang", -0.75)):
        assert np.all(ref.beta_array(kind, eta, t) < t), (kind, eta)
    assert np.all(ref.beta_array("wang", 0.75, t) > t) and np.all(ref.beta_array("pow", 2.0, t) > t)


def test_the_inverse_normal_cdf_inverts_the_cdf_to_a_tenth_of_the_device_tolerance():
    t = TAUS[TAUS > 0]
    back = np.array([ref.ncdf(ref.ncdfinv(float(x))) for x in t])
    err = np.abs(back - t) / ref.spacing32(t)
    assert err.max() <= 0.1, err.max()
    assert err.max() <= 1e-6, "in fact to the last places of double"


@pytest.mark.parametrize("eta", [0.75, -0.75])
def test_wang_composed_with_its_opposite_is_the_identity(eta):
    t = TAUS[TAUS > 0]
    back = np.array([ref.beta("wang", eta, ref.beta("wang", -eta, float(x))) for x in t])
    err = np.abs(back - t) / ref.spacing32(t)
    assert err.max() <= 0.1, err.max()


def test_spacing32_is_the_fp32_spacing_at_the_value():
    for x in (1.0, 0.75, 0.5, 2.0 ** -24, 3e-39, 1e-45, 0.9999999):
        want = float(np.spacing(np.float32(x))) if float(np.float32(x)) <= x else float(np.float32(x) - np.nextafter(np.float32(x), np.float32(0)))
        assert float(ref.spacing32(x)) == want, x
    assert float(ref.spacing32(0.0)) == 2.0 ** -149


def test_rounding_the_reference_to_fp32_stays_within_the_margin_it_derives():
    """The bound the device test uses — one spacing at the float64 value — leaves room for the one rounding: half a spacing."""
    for kind, eta in CASES:
        if kind == "cvar":
            continue
        b = ref.beta_array(kind, eta, TAUS)
        assert np.all(np.abs(b.astype(np.float32).astype(np.float64) - b) <= 0.5 * ref.spacing32(b)), (kind, eta)
