"""Resumable snapshots: the file formats and the state blobs behind ``Trainer.save_snapshot`` / ``Trainer.load_snapshot``.

A snapshot directory holds
  checkpoint.pth   ``Trainer.save_checkpoint``, unchanged (weights, optimizer moments, the learner's state block, the frame counter)
  state.pth        everything else a run needs to CONTINUE: ``meta`` (format version, config dict, ring geometry, chunk list), the replay's and the actor's state blobs
                   (the layouts of a0_rbuf_state_save / a0_actor_state_save, include/agent0_hip.h — written and read here too, so that a snapshot saved under the
                   library's handles loads under the Python classes and the other way round), the learner's Philox state, the raw network / NoisyNet buffers, the
                   ring's act / rew / done, priorities or sum-tree, the statistics windows
  frames.bin       the ring's frames, deduplicated chunk by chunk by a0_snapshot_pack (csrc/snapshot.hip): per chunk
                   u32 lit_id[rows * 8] | u32 n_lit | pad to 16 B | u8 literals[n_lit][frame_bytes]
Everything in this module that does not touch the device is plain numpy / file work and is tested without a GPU (tests/test_snapshot_format.py).
"""
from __future__ import annotations

import os
import shutil
from typing import Dict, List, Optional

import numpy as np

FORMAT_VERSION = 1
CHUNK_ROWS = 4096                      # rows per chunk: at most 231 MB unpacked, whatever replay.size is
FRAMES_PER_ROW = 8                     # st || st_next, 4 frames each
RBUF_MAGIC = int.from_bytes(b"A0A0RBS1", "little")
ACTOR_MAGIC = int.from_bytes(b"A0A0ACT1", "little")
WORDS = 32

# what has to agree between the Trainer that saved and the Trainer that loads (seed excepted: it is part of the state)
GEOMETRY_KEYS = ("replay.size", "obs_shape", "action_dim", "learner.algo", "actor.num_envs", "actor.sample_steps", "learner.n_step_q", "learner.batch_size",
                 "learner.dueling_head", "learner.noisy_net", "replay.policy", "replay.sumtree", "schedule", "env")


def _dbits(x: float) -> int:
    return int(np.array([x], dtype="<f8").view("<i8")[0])


def _bitsd(w: int) -> float:
    return float(np.array([w], dtype="<i8").view("<f8")[0])


# ----------------------------------------------------------------------------- meta
def geometry(cfg_dict: dict, schedule: str, env: str) -> dict:
    def get(path):
        d = cfg_dict
        for k in path.split("."):
            d = d[k]
        return list(d) if isinstance(d, (tuple, list)) else d
    g = {k: get(k) for k in GEOMETRY_KEYS if k not in ("schedule", "env")}
    g["schedule"], g["env"] = schedule, env
    return g


def check_geometry(saved: dict, mine: dict, where: str = "snapshot"):
    diff = [k for k in GEOMETRY_KEYS if saved.get(k) != mine.get(k)]
    if diff:
        raise ValueError(f"{where} was written by a run with another configuration; differing keys: " + ", ".join(f"{k} (saved {saved.get(k)!r}, here {mine.get(k)!r})" for k in diff))


def make_meta(cfg_dict: dict, geo: dict, chunks: List[dict], frame_bytes: int, extra: Optional[dict] = None) -> dict:
    m = {"format": FORMAT_VERSION, "config": cfg_dict, "geometry": geo, "chunks": chunks, "frame_bytes": int(frame_bytes), "frames_per_row": FRAMES_PER_ROW}
    m.update(extra or {})
    return m


def check_meta(meta: dict):
    if not isinstance(meta, dict) or meta.get("format") != FORMAT_VERSION:
        raise ValueError(f"snapshot format {None if not isinstance(meta, dict) else meta.get('format')!r}: this build reads format {FORMAT_VERSION}")


# ----------------------------------------------------------------------------- directories: write to <dir>.tmp, then rename
def begin_write(path: str) -> str:
    tmp = path.rstrip("/") + ".tmp"
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)               # left behind by a job killed mid-write
    os.makedirs(tmp)
    return tmp


def commit_write(path: str):
    """<dir>.tmp becomes <dir>; a previous <dir> is kept as <dir>.old until the new one is in place."""
    path = path.rstrip("/")
    tmp, old = path + ".tmp", path + ".old"
    if os.path.isdir(old):
        shutil.rmtree(old)
    if os.path.isdir(path):
        os.rename(path, old)
    os.rename(tmp, path)
    if os.path.isdir(old):
        shutil.rmtree(old)


def resolve_dir(path: str) -> str:
    """The directory ``load_snapshot(path)`` reads: ``path`` itself — never ``path.tmp`` — or ``path.old`` when a writer was killed between its two renames."""
    path = path.rstrip("/")
    for p in (path, path + ".old"):
        if os.path.isfile(os.path.join(p, "state.pth")) and os.path.isfile(os.path.join(p, "checkpoint.pth")) and os.path.isfile(os.path.join(p, "frames.bin")):
            return p
    raise FileNotFoundError(f"{path}: no complete snapshot (state.pth, checkpoint.pth, frames.bin)")


def is_snapshot_dir(path: str) -> bool:
    return bool(path) and (os.path.isdir(path.rstrip("/")) or os.path.isdir(path.rstrip("/") + ".old"))


# ----------------------------------------------------------------------------- chunks
def chunk_plan(size: int, top: int, written: int, chunk_rows: int = CHUNK_ROWS) -> List[dict]:
    """The ring's filled rows in AGE order (oldest first), split at the wrap and into chunks of at most ``chunk_rows`` rows: [{slot, rows}]."""
    head = written % size if written > size else 0
    spans = [(head, top - head), (0, head)] if head else [(0, top)]
    out = []
    for s0, n in spans:
        o = 0
        while o < n:
            k = min(chunk_rows, n - o)
            out.append({"slot": int(s0 + o), "rows": int(k)})
            o += k
    return out


def literal_offset(n_frames: int) -> int:
    return (n_frames * 4 + 4 + 15) // 16 * 16


def check_chunk_header(head: np.ndarray, n_frames: int, n_lit_meta: int):
    """``head``: the first literal_offset(n_frames) bytes of a chunk record.  Raises unless the table is consistent with the literal count."""
    ids = head[: n_frames * 4].view("<u4")
    n_lit = int(head[n_frames * 4: n_frames * 4 + 4].view("<u4")[0])
    if n_lit != n_lit_meta or n_lit < 1 or n_lit > n_frames or int(ids.max()) >= n_lit:
        raise ValueError(f"frames.bin: damaged chunk (literal count {n_lit}, listed {n_lit_meta}, largest id {int(ids.max())}, frames {n_frames})")


# ----------------------------------------------------------------------------- state blobs (include/agent0_hip.h)
def replay_blob(size, obs_bytes, B, prioritize, top, written, epoch, rng_seed, rng_off, beta_use, sched_cur, max_p, alpha, eps, beta0, total_steps) -> np.ndarray:
    w = np.zeros(WORDS, dtype="<i8")
    w[0:8] = [RBUF_MAGIC, 1, size, obs_bytes, B, prioritize, top, written]
    if epoch is not None:
        w[8:13] = [1, epoch["top"], epoch["nb"], epoch["pos"], epoch["seed"]]
    w[13:21] = [int(o) for o in rng_off]
    w[21], w[22], w[23] = _dbits(beta_use), _dbits(sched_cur), _dbits(float(np.float32(max_p)))
    w[24] = np.array([rng_seed], dtype="<u8").view("<i8")[0]
    w[25], w[26], w[27], w[28] = _dbits(alpha), _dbits(eps), _dbits(beta0), int(total_steps)
    return w.view(np.uint8).copy()


def parse_replay_blob(blob: np.ndarray) -> dict:
    w = np.asarray(blob, dtype=np.uint8)[: WORDS * 8].view("<i8")
    if int(w[0]) != RBUF_MAGIC or int(w[1]) != 1:
        raise ValueError("not a replay state blob of version 1")
    return {"size": int(w[2]), "obs_bytes": int(w[3]), "B": int(w[4]), "prioritize": int(w[5]), "top": int(w[6]), "written": int(w[7]),
            "epoch": {"top": int(w[9]), "nb": int(w[10]), "pos": int(w[11]), "seed": int(w[12])} if int(w[8]) else None,
            "rng_off": [int(x) for x in w[13:21]], "beta_use": _bitsd(w[21]), "sched_cur": _bitsd(w[22]), "max_p": _bitsd(w[23]),
            "rng_seed": int(w[24:25].view("<u8")[0]), "alpha": _bitsd(w[25]), "eps": _bitsd(w[26]), "beta0": _bitsd(w[27]), "total_steps": int(w[28])}


_ACTOR_ARRAYS = (("obs", np.uint8), ("ep_ret", "<f4"), ("ring_act", "<i4"), ("ring_rew", "<f4"), ("ring_done", "<f4"), ("qs", "<f4"), ("stat_mask", "<f4"), ("stat_ret", "<f4"))


def _actor_counts(E, T, n, K, obs_bytes) -> Dict[str, int]:
    return {"obs": K * E * obs_bytes, "ep_ret": E, "ring_act": n * E, "ring_rew": n * E, "ring_done": n * E, "qs": T, "stat_mask": T * E, "stat_ret": T * E}


def actor_blob(d: dict) -> np.ndarray:
    """``d``: E, T, A, dueling, n_step, env_task, reset_noise_freq, discount, K, cur, g, steps, rng_seed, rng_off[8], env_seed, rank + the arrays of ``_ACTOR_ARRAYS``."""
    w = np.zeros(WORDS, dtype="<i8")
    w[0:9] = [ACTOR_MAGIC, 1, d["E"], d["T"], d["A"], int(bool(d["dueling"])), d["n_step"], d["env_task"], d["reset_noise_freq"]]
    w[9] = _dbits(d["discount"])
    w[10:14] = [d["K"], d["cur"], d["g"], d["steps"]]
    w[14] = np.array([d["rng_seed"]], dtype="<u8").view("<i8")[0]
    w[15:23] = [int(o) for o in d["rng_off"]]
    w[23], w[24] = int(d["env_seed"]), int(d["rank"])
    obs_bytes = np.asarray(d["obs"]).size // (d["K"] * d["E"])
    counts = _actor_counts(d["E"], d["T"], d["n_step"], d["K"], obs_bytes)
    parts = [w.view(np.uint8)]
    for name, dt in _ACTOR_ARRAYS:
        a = np.ascontiguousarray(np.asarray(d[name]).reshape(-1)[: counts[name]], dtype=dt)
        assert a.size == counts[name], f"actor state: {name} has {a.size} elements, expected {counts[name]}"
        parts.append(a.view(np.uint8))
    return np.concatenate(parts)


def parse_actor_blob(blob: np.ndarray, obs_bytes: int = 4 * 84 * 84) -> dict:
    blob = np.asarray(blob, dtype=np.uint8)
    w = blob[: WORDS * 8].view("<i8")
    if int(w[0]) != ACTOR_MAGIC or int(w[1]) != 1:
        raise ValueError("not an actor state blob of version 1")
    d = {"E": int(w[2]), "T": int(w[3]), "A": int(w[4]), "dueling": int(w[5]), "n_step": int(w[6]), "env_task": int(w[7]), "reset_noise_freq": int(w[8]),
         "discount": _bitsd(w[9]), "K": int(w[10]), "cur": int(w[11]), "g": int(w[12]), "steps": int(w[13]), "rng_seed": int(w[14:15].view("<u8")[0]),
         "rng_off": [int(x) for x in w[15:23]], "env_seed": int(w[23]), "rank": int(w[24])}
    counts = _actor_counts(d["E"], d["T"], d["n_step"], d["K"], obs_bytes)
    o = WORDS * 8
    for name, dt in _ACTOR_ARRAYS:
        nbytes = counts[name] * np.dtype(dt).itemsize
        if o + nbytes > blob.size:
            raise ValueError("actor state blob: truncated")
        d[name] = blob[o:o + nbytes].view(dt).copy()
        o += nbytes
    return d


ACTOR_DESC_KEYS = ("E", "T", "A", "dueling", "n_step", "env_task", "reset_noise_freq", "discount", "K")


def check_actor_desc(saved: dict, mine: dict):
    diff = [k for k in ACTOR_DESC_KEYS if saved[k] != mine[k]]
    if diff:
        raise ValueError("actor state was saved by an actor of another description; differing keys: " + ", ".join(f"{k} (saved {saved[k]!r}, here {mine[k]!r})" for k in diff))


# ----------------------------------------------------------------------------- frames.bin through ONE page-locked staging buffer
class FrameFile:
    """Packs / unpacks ring rows chunk by chunk: one device buffer and one page-locked host buffer of a chunk's worst case, whatever the ring's size."""

    def __init__(self, ops, frame_bytes: int, max_rows: int):
        import torch
        self.ops, self.fb, self.F = ops, int(frame_bytes), FRAMES_PER_ROW
        self.max_rows = max(1, min(int(max_rows), CHUNK_ROWS))
        bound = ops.snapshot_pack_bound(self.max_rows, self.F, self.fb)
        self.dev = torch.empty(bound, dtype=torch.uint8, device=ops.device)
        self.work = torch.empty(self.max_rows * self.F, dtype=torch.int32, device=ops.device)
        self.host = torch.empty(bound, dtype=torch.uint8).pin_memory()
        self.bad = torch.zeros(1, dtype=torch.int32, device=ops.device)

    def write(self, f, frames, chunks: List[dict], stride: int, buf: str) -> List[dict]:
        """``frames``: a ring's flat uint8 tensor; appends one record per chunk to the open file ``f`` and returns the chunks with their literal counts."""
        import torch
        out = []
        row_bytes = self.F * self.fb
        for c in chunks:
            n, s0 = c["rows"], c["slot"]
            nf = n * self.F
            off = literal_offset(nf)
            self.ops.snapshot_pack(frames[s0 * row_bytes:(s0 + n) * row_bytes], n, self.F, self.fb, stride, self.dev, self.work)
            self.host[:off].copy_(self.dev[:off], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            n_lit = int(self.host[nf * 4: nf * 4 + 4].numpy().view("<u4")[0])
            total = off + n_lit * self.fb
            self.host[off:total].copy_(self.dev[off:total], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            f.write(memoryview(self.host[:total].numpy()))
            out.append({"buf": buf, "slot": s0, "rows": n, "n_lit": n_lit, "bytes": total})
        return out

    def read(self, f, frames, chunks: List[dict]):
        import torch
        row_bytes = self.F * self.fb
        for c in chunks:
            n, s0, n_lit = c["rows"], c["slot"], c["n_lit"]
            nf = n * self.F
            off = literal_offset(nf)
            total = off + n_lit * self.fb
            if n > self.max_rows or total != c["bytes"] or (s0 + n) * row_bytes > frames.numel():
                raise ValueError(f"frames.bin: chunk {c} does not fit this ring")
            view = self.host[:total].numpy()
            if f.readinto(memoryview(view)) != total:
                raise ValueError("frames.bin: truncated")
            check_chunk_header(view[:off], nf, n_lit)
            self.dev[:total].copy_(self.host[:total], non_blocking=True)
            self.ops.snapshot_unpack(self.dev, n, self.F, self.fb, frames[s0 * row_bytes:(s0 + n) * row_bytes], self.bad)
            torch.cuda.current_stream().synchronize()          # the staging buffer is reused by the next chunk
        if int(self.bad[0]) != 0:
            raise ValueError("frames.bin: a literal id outside its chunk's literals")
