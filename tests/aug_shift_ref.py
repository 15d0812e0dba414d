"""numpy restatement of ``learner.aug_shift`` (agent0_amd/csrc/augment.hip): the CPU reference the kernel and the learners are compared against, byte for byte.

The draw: sample b of update u owns words 4 (u B + b) .. + 3 of Philox stream 7 of the learner's seed — dy(st), dx(st), dy(st_next), dx(st_next), each
``word % (2 pad + 1) - pad``.  The shift: out[c][y][x] = in[c][clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)], one (dy, dx) for all planes of an observation.
"""
from __future__ import annotations

import numpy as np

STREAM_AUG = 7


def draws(seed: int, u: int, B: int, pad: int) -> np.ndarray:
    """-> int64 [B, 4]: (dy, dx) of st, (dy, dx) of st_next for every sample of update ``u``."""
    from oracle.core import rng_u32
    words = rng_u32(int(seed), STREAM_AUG, 4 * (int(u) * int(B)), 4 * int(B)).reshape(B, 4)
    return words.astype(np.int64) % (2 * pad + 1) - pad


def shift_rows(rows: np.ndarray, d: np.ndarray) -> np.ndarray:
    """rows u8 [B, 2, C, H, W] (st, st_next), d [B, 4] -> the shifted rows, by clamped index arrays."""
    B, two, C, H, W = rows.shape
    assert two == 2 and d.shape == (B, 4) and rows.dtype == np.uint8
    out = np.empty_like(rows)
    for b in range(B):
        for o in range(2):
            ys = np.clip(np.arange(H) + int(d[b, 2 * o]), 0, H - 1)
            xs = np.clip(np.arange(W) + int(d[b, 2 * o + 1]), 0, W - 1)
            out[b, o] = rows[b, o][:, ys][:, :, xs]
    return out
