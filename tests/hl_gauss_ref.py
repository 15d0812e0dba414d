"""Float64 reference, error bound and cases of the HL-Gauss classification target (a0_loss_c51_hl_gauss, ``learner.c51.hl_gauss``): the yardstick of
tests/test_gpu_hl_gauss.py, itself held to closed forms and to six wrong computations by tests/test_hl_gauss_reference_helpers.py.  No import of the library.

The target (Farebrother et al. 2024, "Stop Regressing: Training Value Functions via Classification for Scalable Deep RL", section 3.1 and 4), per sample, from
the TARGET network's logits x_t at the greedy next action a*, on the support z_t = vmin + t Delta, t < T, Delta = (vmax - vmin) / (T - 1), read as bin centres
with the T + 1 edges e_k = vmin - Delta / 2 + k Delta:

    p'   = softmax(x),  v' = sum_t p'_t z_t,  y = clamp(r + gamma_n (1 - d) v', vmin, vmax),  sigma = rho Delta
    m_t  = [Phi((e_{t+1} - y) / sigma) - Phi((e_t - y) / sigma)] / [Phi((e_T - y) / sigma) - Phi((e_0 - y) / sigma)],  Phi(u) = (1 + erf(u / sqrt 2)) / 2

``hl_gauss64`` evaluates it in float64 (``torch.erf`` on float64) from the fp32 inputs, gamma_n, vmin and vmax rounded to fp32 as the entry point receives them, and
returns with m the bound e_m [B][T] on the kernel, which forms y in fp32 and the Gaussian mass in double, rounded to fp32 once.  The derivation, u = 2^-24:

  exp       e_t = expf(x_t - max x): the subtraction rounds once (u |x_t - max|, which moves the exponential by as much relatively) and expf has the relative error
            EXPF_REL (the project's recorded figure, doubled): r_t = 2 EXPF_REL + u |x_t - max|, as in value_loss_ref._softmax_rel.  A result below 2^-126 may be
            flushed: TINY per term, against a denominator that is at least 1.
  v'        sum e_t z_t / sum e_t.  A relative perturbation eps_t of e_t reaches both sums and moves the quotient by sum_t p'_t eps_t (z_t - v'): the common part
            cancels.  The products round once and each butterfly has six stages (7 u sum p'|z| and 6 u |v'|), the division once (u |v'|):
            e_v = 1.01 [sum_t p'_t r_t |z_t - v'| + 7 u sum_t p'_t |z_t| + 7 u |v'| + T TINY (max|z| + |v'|)], the 1.01 for the second-order terms.
  y         g = gamma_n (1 - d) rounds twice, g v' once, r + g v' once (a fused multiply-add rounds less): e_y = |g| e_v + 3 u |g v'| + u |r + g v'|.  The clamp
            is 1-Lipschitz and continuous: an fp32 y on the other side of a seam is no further from the float64 one than before it.
  m(y)      dm_t/dy = [phi(u_t) - phi(u_{t+1})] / (sigma Z) - m_t [phi(u_0) - phi(u_T)] / (sigma Z), phi the normal density, u_k = (e_k - y) / sigma, Z the
            normaliser; the second derivative is bounded by M2 = (1 / Zl + 0.64 / Zl^2) / sigma^2 (from |phi| <= 0.3990, |phi'| <= 0.2420 and N_t <= Z), Zl = Z -
            0.4 e_y / sigma a lower bound of Z over the interval.  So the fp32 y moves m_t by at most |dm_t/dy| e_y + M2 e_y^2 / 2.
  double    both sides evaluate T + 1 error functions in double: the argument (e_k - y) / sigma / sqrt 2 carries 2^-53 (2 (|e_k| + |y|) + 3 |e_k - y|) / sigma,
            which erf (slope <= 1.13) passes on, and erf itself a few 2^-53: E1 = 2^-53 (4 + 5.65 (max|e| + |y|) / sigma) per value and side; a difference of two,
            on both sides, over the normaliser 2 Z (in erf units): e_dbl = 4 E1 (1 + m_t) / (2 Zl) + 2^-52 m_t.
  rounding  the one rounding to fp32: u m_t + 2^-149.

  e_m = |dm_t/dy| e_y + M2 e_y^2 / 2 + e_dbl + u m_t + 2^-149.

``hl_gauss_loss64`` adds the cross entropy of a0_c51_xent against m and its gradient, with value_loss_ref.c51_bounds' terms carried over (tol_m = e_m) and one
rounding more in the gradient: w ((e / s) sum(m) - m) rounds at the subtraction AND at the product with w, each by u times at most po sum(m) + m — 2 u (po sum(m) + m),
where c51_bounds counts one.  There the projection's tol_m has the room; here, where the online softmax puts no weight on a bin, the gradient is -w m and the bound
is e_m + 2 u m with e_m as small as u m.
A NaN reward: m, the loss and the gradient of that sample are NaN (``nan_rows``)."""
from __future__ import annotations

import numpy as np
import torch

import recipe
from actor_tail_cases import EXPF_REL, U
from value_loss_ref import LOGF_BOUND, TINY, _softmax_rel, c51_atoms, c51_loss64

SQRT2 = float(np.sqrt(2.0))
VARIANTS = ("edges_on_atoms", "no_normaliser", "sigma_is_rho", "no_sqrt2", "no_clamp", "online_expectation")
GAMMA = 0.99 ** 3
VMIN, VMAX = -10.0, 10.0
TS, AS, BS = (2, 51, 64), (1, 4, 18), (1, 5)
KINDS = ("vmin", "vmax", "below", "above", "edge", "centre", "done", "spread30", "random")


def _f64(x):
    return np.asarray(x, np.float64)


def _rows(x, idx):
    return x[np.arange(x.shape[0]), np.asarray(idx, np.int64)]


def rhos(T):
    """The ratios of the GPU test: a near one-hot histogram, the paper's value, and the limit of the setting (sigma = the whole support's width + one bin)."""
    return (0.05, 0.75, float(T))


def erf64(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(_f64(x)))).numpy()


def Phi(u, sqrt2=True):
    return 0.5 * (1.0 + erf64(_f64(u) / (SQRT2 if sqrt2 else 1.0)))


def phi(u):
    return np.exp(-0.5 * _f64(u) ** 2) / np.sqrt(2.0 * np.pi)


def support(vmin, vmax, T):
    """(vmin, vmax, Delta, edges [T + 1]) in float64 from the fp32 vmin and vmax."""
    vmin, vmax = float(np.float32(vmin)), float(np.float32(vmax))
    delta = (vmax - vmin) / (T - 1)
    return vmin, vmax, delta, vmin - 0.5 * delta + np.arange(T + 1) * delta


def mass64(y, vmin, vmax, T, rho, variant=None):
    """The Gaussian histogram of y [B] (float64, already clamped) -> (m [B][T], Z [B], u [B][T + 1], sigma)."""
    vmin, vmax, delta, edges = support(vmin, vmax, T)
    if variant == "edges_on_atoms":
        edges = vmin + np.arange(T + 1) * delta
    sigma = float(rho) if variant == "sigma_is_rho" else float(rho) * delta
    u = (edges[None, :] - _f64(y).reshape(-1, 1)) / sigma
    P = Phi(u, sqrt2=variant != "no_sqrt2")
    Z = P[:, -1] - P[:, 0]
    N = P[:, 1:] - P[:, :-1]
    return (N if variant == "no_normaliser" else N / Z[:, None]), Z, u, sigma


def target64(tgt_logits, A, T, a_star, rew, done, atoms, gamma_n, vmin, vmax, B, variant=None, online_next=None):
    """Steps 1 - 5 in float64: (y [B] clamped, y_raw, v', p' [B][T], x [B][T] the logits the expectation is taken of)."""
    src = online_next if variant == "online_expectation" else tgt_logits
    x = _f64(_rows(np.asarray(src, np.float32).reshape(B, A, T), a_star))
    ex = np.exp(x - x.max(-1, keepdims=True))
    p = ex / ex.sum(-1, keepdims=True)
    z = _f64(np.asarray(atoms, np.float32)).reshape(1, T)
    v = (p * z).sum(-1)
    g = float(np.float32(gamma_n)) * (1.0 - _f64(np.asarray(done, np.float32)).reshape(B))
    y_raw = _f64(np.asarray(rew, np.float32)).reshape(B) + g * v
    lo, hi = float(np.float32(vmin)), float(np.float32(vmax))
    y = y_raw if variant == "no_clamp" else np.where(y_raw < lo, lo, np.where(y_raw > hi, hi, y_raw))      # comparisons: a NaN stays
    return y, y_raw, v, p, x, g


def hl_gauss64(tgt_logits, A, T, a_star, rew, done, atoms, gamma_n, vmin, vmax, rho, B, variant=None, online_next=None):
    """-> dict(m [B][T], e_m [B][T], y, y_raw, v, p, Z, e_y, e_v, nan_rows).  The module's docstring has the formulas and the derivation of e_m; a variant (one of
    VARIANTS, for the helper test's negative controls) carries no bound."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y, y_raw, v, p, x, g = target64(tgt_logits, A, T, a_star, rew, done, atoms, gamma_n, vmin, vmax, B, variant, online_next)
        nan_rows = ~np.isfinite(y)
        ys = np.where(nan_rows, 0.0, y)
        m, Z, u, sigma = mass64(ys, vmin, vmax, T, rho, variant)
        out = dict(y=y, y_raw=y_raw, v=v, p=p, Z=Z, nan_rows=nan_rows, sigma=sigma)
        if variant is None:
            z = _f64(np.asarray(atoms, np.float32)).reshape(1, T)
            dz = np.abs(x - x.max(-1, keepdims=True))
            r = 2 * EXPF_REL + U * dz
            e_v = 1.01 * ((p * r * np.abs(z - v[:, None])).sum(-1) + 7 * U * (p * np.abs(z)).sum(-1) + 7 * U * np.abs(v) + T * TINY * (np.abs(z).max() + np.abs(v)))
            yr = np.where(nan_rows, 0.0, y_raw)
            e_y = np.abs(g) * e_v + 3 * U * np.abs(g * v) + U * np.abs(yr)
            _, _, _, edges = support(vmin, vmax, T)
            Zl = Z - 0.4 * e_y / sigma
            assert (Zl > 0.25).all(), "the normaliser stays away from 0 (it is at least about 0.34 for rho <= num_atoms)"
            ph = phi(u)
            dm = (ph[:, :-1] - ph[:, 1:]) / (sigma * Z[:, None]) - m * ((ph[:, 0] - ph[:, -1]) / (sigma * Z))[:, None]
            M2 = (1.0 / Zl + 0.64 / Zl ** 2) / sigma ** 2
            E1 = 2.0 ** -53 * (4 + 5.65 * (np.abs(edges).max() + np.abs(ys)) / sigma)
            e_dbl = 4 * E1[:, None] * (1 + m) / (2 * Zl[:, None]) + 2.0 ** -52 * m
            out.update(e_v=e_v, e_y=e_y, dm=dm, e_m=np.abs(dm) * e_y[:, None] + 0.5 * (M2 * e_y ** 2)[:, None] + e_dbl + U * m + 2.0 ** -149)
        m = m.copy()
        m[nan_rows] = np.nan
        out["m"] = m
    return out


def hl_gauss_loss64(logits, tgt_logits, A, T, act, a_star, rew, done, wgt, atoms, gamma_n, vmin, vmax, rho, B):
    """The whole of a0_loss_c51_hl_gauss: hl_gauss64's m, loss = -sum_t m_t log softmax(online logits at the taken action)_t, dlogits = w (softmax sum(m) - m) at the
    taken action ([B][A][T], 0 elsewhere), with tol_loss [B] and tol_g [B][T]: value_loss_ref.c51_bounds with e_m in tol_m's place."""
    ref = hl_gauss64(tgt_logits, A, T, a_star, rew, done, atoms, gamma_n, vmin, vmax, rho, B)
    m, tol_m = np.where(ref["nan_rows"][:, None], 0.0, ref["m"]), ref["e_m"]
    xa = _f64(_rows(np.asarray(logits, np.float32).reshape(B, A, T), act))
    loss, logp, po = c51_loss64(xa, m)
    w = _f64(np.asarray(wgt, np.float32)).reshape(B, 1)
    msum = m.sum(-1, keepdims=True)
    g = w * (po * msum - m)
    dz = np.abs(xa - xa.max(-1, keepdims=True))
    lse = np.abs(np.log(np.exp(-dz).sum(-1, keepdims=True)))
    e_sum = EXPF_REL + U * (po * dz).sum(-1, keepdims=True) + 6 * U
    tol_logp = U * dz + e_sum + LOGF_BOUND + U * (dz + lse)
    tol_loss = (tol_m * np.abs(logp) + m * tol_logp).sum(-1) + 7 * U * (m * np.abs(logp)).sum(-1)
    tol_msum = tol_m.sum(-1, keepdims=True) + 6 * U * msum
    tol_g = np.abs(w) * (po * msum * (_softmax_rel(xa, po) + 2 * U) + po * tol_msum + tol_m + 2 * U * (po * msum + m) + TINY)
    nan = ref["nan_rows"]
    loss, g = loss.copy(), g.copy()
    loss[nan], g[nan] = np.nan, np.nan
    dl = np.zeros((B, A, T))
    dl[np.arange(B), np.asarray(act, np.int64)] = g
    ref.update(loss=loss, g=g, dlogits=dl, tol_loss=tol_loss, tol_g=tol_g, logp=logp, po=po)
    return ref


# ------------------------------------------------------------------------------------------------ cases
_CASES = {}


def case(T, A, B, shift=0, vmin=VMIN, vmax=VMAX):
    """Inputs of one launch (computed once; never modified): logits, tgt_logits, online_next [B][A][T] fp32, act, a_star, rew, done, wgt, atoms, and ``kinds`` — sample b
    is of kind KINDS[(b + shift) % 9]:
      vmin / vmax    a terminal whose reward is vmin / vmax: y on the first / last centre, half a bin inside the outer edge
      below / above  y beyond the support before the clamp (not terminal: the reward alone is 3 / 5 outside)
      edge / centre  a terminal whose reward is fl32 of an interior bin edge / exactly an interior atom (T = 2: the only interior edge, 0; the centre vmin)
      done           done = 1 with a random reward inside the support
      spread30       target and online logits spread over +-30
      random         none of these"""
    key = (T, A, B, shift, vmin, vmax)
    if key in _CASES:
        return _CASES[key]
    g = recipe.gen(35000 + 977 * T + 31 * A + 7 * B + shift)
    atoms = c51_atoms(vmin, vmax, T)
    delta = (vmax - vmin) / (T - 1)
    x, xt, xn = (g.standard_normal((B, A, T)).astype(np.float32) * np.float32(1.5) for _ in range(3))
    act, a_star = g.integers(0, A, B).astype(np.int32), g.integers(0, A, B).astype(np.int32)
    rew = g.uniform(-1.0, 1.0, B).astype(np.float32)
    done = np.zeros(B, np.float32)
    wgt = g.uniform(0.25, 1.0, B).astype(np.float32)
    kinds = []
    for b in range(B):
        kind = KINDS[(b + shift) % len(KINDS)]
        kinds.append(kind)
        k = int(g.integers(1, T - 1)) if T > 2 else 0
        if kind in ("vmin", "vmax", "edge", "centre", "done"):
            done[b] = 1.0
            rew[b] = {"vmin": vmin, "vmax": vmax, "edge": vmin - 0.5 * delta + (k if T > 2 else 1) * delta, "centre": float(atoms[k]),
                      "done": float(g.uniform(vmin, vmax))}[kind]
        elif kind == "below":
            rew[b] = vmin - 3.0 - float(np.abs(atoms).max())
        elif kind == "above":
            rew[b] = vmax + 5.0 + float(np.abs(atoms).max())
        elif kind == "spread30":
            xt[b] = g.uniform(-30.0, 30.0, (A, T)).astype(np.float32)
            x[b] = g.uniform(-30.0, 30.0, (A, T)).astype(np.float32)
            xn[b] = g.uniform(-30.0, 30.0, (A, T)).astype(np.float32)
    c = dict(logits=x, tgt_logits=xt, online_next=xn, act=act, a_star=a_star, rew=rew, done=done, wgt=wgt, atoms=atoms, kinds=tuple(kinds), vmin=vmin, vmax=vmax)
    _CASES[key] = c
    return c


def launches(T, A):
    """(B, shift) of the launches of one (T, A): B = 5 twice (kinds 0 - 4 and 5 - 8, 0) and B = 1 nine times, so that either batch size meets every kind."""
    return [(5, 0), (5, 5)] + [(1, s) for s in range(len(KINDS))]
