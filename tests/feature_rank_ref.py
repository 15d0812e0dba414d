"""numpy restatement of the feature rank (``learner.rank_freq`` / ``learner.rank_delta``; a0_feature_rank, include/agent0_hip.h): srank_delta of Kumar et al. 2021
through the Gram matrix, its error rule, and the input set both test files share (tests/test_feature_rank_config.py, tests/test_gpu_feature_rank.py)."""
import numpy as np

N = 512
FLOOR = N * 2.0 ** -52          # sigma_i = 0 where lambda_i <= FLOOR * lambda_1
EIG_TOL = N * 2.0 ** -53        # what an eigenvalue may differ by, in units of lambda_1: half the floor
DELTAS = (0.01, 0.1)


def gram(X):
    """G = X^T X accumulated in np.longdouble, returned as float64 (the products of fp32 values are exact in either)."""
    Xl = np.asarray(X, np.float32).astype(np.longdouble)
    return (Xl.T @ Xl).astype(np.float64)


def abs_gram(X):
    """sum_r |x_ri x_rj|: what the any-order summation bound of a Gram element is stated in."""
    Xa = np.abs(np.asarray(X, np.float32).astype(np.float64))
    return Xa.T @ Xa


def eigenvalues(G):
    """The eigenvalues of G, descending."""
    return np.linalg.eigvalsh(np.asarray(G, np.float64))[::-1].copy()


def floor_of(lam):
    """sigma from descending eigenvalues: sqrt above the floor, 0 at or under it (tiny negative eigenvalues included)."""
    lam = np.asarray(lam, np.float64)
    keep = (lam > FLOOR * lam[0]) & (lam > 0.0)
    return np.sqrt(np.where(keep, lam, 0.0))


def spectrum(G):
    return floor_of(eigenvalues(G))


def ratios(sigma):
    """The cumulative shares (sigma_1 + ... + sigma_k) / (sigma_1 + ... + sigma_512), sums in index order; None if every sigma is 0."""
    cum = np.cumsum(np.asarray(sigma, np.float64))
    return None if cum[-1] == 0.0 else cum / cum[-1]


def srank(sigma, delta):
    r = ratios(sigma)
    return 0 if r is None else int(np.argmax(r >= 1.0 - delta)) + 1


def margin(sigma, delta):
    """The distance of the nearest cumulative share from 1 - delta (inf for the zero spectrum)."""
    r = ratios(sigma)
    return np.inf if r is None else float(np.abs(r - (1.0 - delta)).min())


def ratio_error_bound(lam, tol):
    """The largest change of any cumulative share when every eigenvalue above the floor moves by tol * lambda_1, to first order: |d sigma_i| = |d lambda_i| /
    (2 sigma_i); share k = S_k / S moves most when the leading k sigmas go one way and the others the opposite way: (dS_k (S - S_k) + S_k (dS - dS_k)) / S^2."""
    lam = np.asarray(lam, np.float64)
    sigma = floor_of(lam)
    if not sigma.any():
        return 0.0
    ds = np.where(sigma > 0.0, tol * lam[0] / (2.0 * np.where(sigma > 0.0, sigma, 1.0)), 0.0)
    S, dS = np.cumsum(sigma), np.cumsum(ds)
    return float(((dS * (S[-1] - S) + S * (dS[-1] - dS)) / S[-1] ** 2).max())


# ------------------------------------------------------------------------------------------------ the input set
ROWS = (1, 3, 4, 5, 63, 511, 512, 513, 2051)
MIXES = ((1, 0.0), (7, 0.01), (64, 0.05), (512, 0.0))
FIXED = ("zeros", "one-element", "identity", "graded", "inf-row")
CASES = [("mix", r, k, z) for r in ROWS for k, z in MIXES] + [(name, 0, 0, 0.0) for name in FIXED]
SEED = 2029


def case_id(case):
    return f"rows{case[1]}-k{case[2]}-noise{case[3]}" if case[0] == "mix" else case[0]


_X, _REF = {}, {}


def make(case):
    """The case's activations, fp32 [rows][512]; cached, never modified.  ``mix``: relu(A B / sqrt(k) + noise Z) from a Philox generator keyed by the case."""
    if case not in _X:
        kind, rows, k, noise = case
        if kind == "mix":
            g = np.random.Generator(np.random.Philox(key=SEED + 1000 * rows + k))
            A, B, Z = g.standard_normal((rows, k)), g.standard_normal((k, N)), g.standard_normal((rows, N))
            X = np.maximum(A @ B / np.sqrt(k) + noise * Z, 0.0)
        elif kind == "zeros":
            X = np.zeros((6, N))
        elif kind == "one-element":
            X = np.zeros((9, N))
            X[7, 300] = 3.0
        elif kind == "identity":
            X = np.eye(N)
        elif kind == "graded":
            X = np.diag(2.0 ** (-np.arange(N) / 8.0))
        else:
            assert kind == "inf-row"
            X = np.ones((5, N))
            X[3, :] = np.inf
        _X[case] = np.ascontiguousarray(X.astype(np.float32))
        _X[case].setflags(write=False)
    return _X[case]


def reference(case):
    """(G, its descending eigenvalues, sigma) of the case through ``gram`` and ``eigvalsh``; cached."""
    if case not in _REF:
        G = gram(make(case))
        lam = eigenvalues(G)
        _REF[case] = (G, lam, floor_of(lam))
    return _REF[case]
