"""The reference of ``learner.net_reset_freq`` (a0_net_reset): the rule table restated from the constructor (agent0_amd/deepq/model.py), and what a reset leaves in
every buffer, in numpy.

Rule table: (offset, count, kind, scale, keep) entries that tile [0, n_adam).  kind 0 = constant ``scale``, 1 = normal with std ``scale``, 2 = uniform in
+-``scale``; keep = 1 marks the encoder, which keeps the share alpha of its values.  An orthogonal matrix of gain g has element RMS exactly g / sqrt(max(rows, cols)).

A reset's arithmetic per element, with phi the fresh value and a32 = alpha rounded to fp32 once (keep = 0: a32 = 0):
  a32 == 1: untouched;  a32 == 0: phi;  otherwise fmaf(a32, fl32(p - phi), phi) — tests/target_tau_ref.py's blend with phi in the target's place.
"""
import math

import numpy as np

import target_tau_ref as TT

CONST, NORMAL, UNIFORM = 0, 1, 2
STREAM_RESET = 8
RELU_GAIN = math.sqrt(2.0)


def segments(L):
    """The table for a ``NetLayout``, written from the constructor's rules block by block (not from ``NetLayout.reset_segments``)."""
    out = []

    def put(off, cnt, kind, scale, keep=0):
        if cnt:
            out.append((off, cnt, kind, float(scale), keep))

    def orth(gain, rows, cols):
        return gain / math.sqrt(max(rows, cols))

    for name, blk in L.blocks.items():
        w, b, N, K = blk.offset, blk.offset + blk.N * blk.K, blk.N, blk.K
        if name.startswith("conv"):
            put(w, N * K, NORMAL, orth(RELU_GAIN, N, K), 1)
            put(b, N, CONST, 0.0, 1)
        elif name in ("fc1", "cos"):
            put(w, N * K, NORMAL, orth(RELU_GAIN, N, K))
            put(b, N, CONST, 0.0)
        elif name == "head":
            put(w, L.Nq * K, NORMAL, orth(0.01, L.Nq, K))
            put(w + L.Nq * K, L.V * K, NORMAL, orth(1.0, L.V, K) if L.V else 0.0)
            put(w + (L.Nq + L.V) * K, (N - L.Nq - L.V) * K, CONST, 0.0)
            put(b, N, CONST, 0.0)
        elif name.endswith(".mu"):
            real = blk.n_real
            put(w, real * K, UNIFORM, 1.0 / math.sqrt(K))
            put(w + real * K, (N - real) * K, CONST, 0.0)
            put(b, real, UNIFORM, 1.0 / math.sqrt(K))
            put(b + real, N - real, CONST, 0.0)
        elif name.endswith(".sigma"):
            real = blk.n_real
            put(w, real * K, CONST, 0.4 / math.sqrt(K))
            put(w + real * K, (N - real) * K, CONST, 0.0)
            if name == "fc1.sigma":
                put(b, N, CONST, 0.4 / math.sqrt(N))
            else:
                put(b, L.Nq, CONST, 0.4 / math.sqrt(L.Nq))
                put(b + L.Nq, L.V, CONST, 0.4 / math.sqrt(L.V) if L.V else 0.0)
                put(b + real, N - real, CONST, 0.0)
        else:
            assert name == "frac", name      # behind n_adam: no entry
    return out


def uniform_fresh(bound, u: np.ndarray) -> np.ndarray:
    """bound * (2 u - 1) in fp32: 2 u - 1 is exact (u is a multiple of 2^-24 below 1), the product is rounded once."""
    u = np.asarray(u, np.float32)
    return (np.float32(bound) * (np.float32(2.0) * u - np.float32(1.0))).astype(np.float32)


def alpha32(alpha) -> np.float32:
    return np.float32(float(alpha))


def expect(p: np.ndarray, phi: np.ndarray, segs, alpha):
    """(want, exact, suspects) over the whole buffer: ``want`` the parameters after a reset from ``p`` with the fresh values ``phi`` (read at normal and uniform
    elements only); ``exact``: True where the result must be these bytes (untouched, replaced, constant); ``suspects``: blended elements where the float64 reference
    rounds twice (at most one ulp there)."""
    p = np.asarray(p, np.float32)
    want = p.copy()
    exact = np.ones(p.size, bool)
    suspects = np.zeros(p.size, bool)
    for off, cnt, kind, scale, keep in segs:
        sl = slice(off, off + cnt)
        a = alpha32(alpha) if keep else np.float32(0.0)
        if a == 1.0:
            continue
        f = np.full(cnt, np.float32(scale), np.float32) if kind == CONST else np.asarray(phi[sl], np.float32)
        if a == 0.0:
            want[sl] = f
        else:
            want[sl] = TT.blend_nearest(f, p[sl], float(a))
            exact[sl] = False
            suspects[sl] = TT.double_rounding_suspects(f, p[sl], float(a))
    return want, exact, suspects
