"""numpy restatement of the replay-snapshot packing format (agent0_amd/csrc/snapshot.hip): the CPU reference the kernels are compared against.

A chunk is ``rows`` [R][F][frame_bytes] u8.  For every frame in row order the FIRST byte-identical frame among the candidates — frames (r, 0 .. j - 1), then frames
(r - stride, 0 .. F - 1) when that row is in the chunk — is its reference; a frame without one is a literal.  Literals are numbered in row order, references are
followed to their literal.  Packed bytes: u32 lit_id[R * F] | u32 n_lit | pad to 16 B | literals[n_lit][frame_bytes].
"""
from __future__ import annotations

import numpy as np


def pack(rows: np.ndarray, stride: int):
    """-> (lit_id [R][F] uint32, n_lit, literals [n_lit][frame_bytes] uint8)"""
    R, F, fb = rows.shape
    stride = min(int(stride), R)
    lit_id = np.zeros((R, F), dtype=np.uint32)
    lits = []
    for r in range(R):
        for j in range(F):
            me = rows[r, j]
            cands = [(r, c) for c in range(j)]
            if stride > 0 and r >= stride:
                cands += [(r - stride, c) for c in range(F)]
            hit = next((c for c in cands if np.array_equal(rows[c], me)), None)
            if hit is None:
                lit_id[r, j] = len(lits)
                lits.append(me)
            else:
                lit_id[r, j] = lit_id[hit]          # the candidate is earlier in row order: already resolved to its literal
    literals = np.stack(lits) if lits else np.zeros((0, fb), dtype=np.uint8)
    return lit_id, len(lits), literals


def unpack(lit_id: np.ndarray, literals: np.ndarray) -> np.ndarray:
    return literals[lit_id.astype(np.int64)]


def literal_offset(n_frames: int) -> int:
    return (n_frames * 4 + 4 + 15) // 16 * 16


def to_bytes(lit_id: np.ndarray, n_lit: int, literals: np.ndarray) -> bytes:
    n = lit_id.size
    head = np.zeros(literal_offset(n), dtype=np.uint8)
    head[: n * 4] = lit_id.reshape(-1).astype("<u4").view(np.uint8)
    head[n * 4: n * 4 + 4] = np.array([n_lit], dtype="<u4").view(np.uint8)
    return head.tobytes() + literals[:n_lit].tobytes()


# ----------------------------------------------------------------------------- rows as an actor writes them
def window_rows(E: int, S: int, fb: int, n: int = 1, resets=(), seed: int = 0):
    """Ring rows of ``E`` envs over ``S`` steps in the order the actor writes them (step-major, env-major): row = st || st_next, each a sliding window of four
    frames, st_next ``n`` steps after st (the n-step transition emitted at step t starts at step t - n + 1, clipped to the run's start).  Every frame an env emits is
    unique (a counter stamped into random bytes).  ``resets``: (env, step) pairs — the env's step at ``step`` ends an episode, so the observation after it is a fresh
    stack of four new frames.  -> (rows [E * S][8][fb], frames emitted in all)"""
    rng = np.random.default_rng(seed)
    count = [0]

    def new_frame():
        f = rng.integers(0, 256, fb, dtype=np.uint8)
        f[:8] = np.array([count[0]], dtype="<u8").view(np.uint8)
        count[0] += 1
        return f

    resets = set(resets)
    obs = [[[new_frame() for _ in range(4)] for _ in range(E)]]          # obs[t][e] = the stack before step t
    for t in range(S):
        nxt = []
        for e in range(E):
            if (e, t) in resets:
                nxt.append([new_frame() for _ in range(4)])
            else:
                nxt.append(obs[t][e][1:] + [new_frame()])
        obs.append(nxt)
    rows = np.zeros((E * S, 8, fb), dtype=np.uint8)
    for t in range(S):
        t0 = max(t - n + 1, 0)
        for e in range(E):
            rows[t * E + e, :4] = np.stack(obs[t0][e])
            rows[t * E + e, 4:] = np.stack(obs[t + 1][e])
    return rows, count[0]
