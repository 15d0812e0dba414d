"""Resumable snapshots without a GPU: the packing format's numpy reference (tests/snapshot_ref.py), the derived literal counts, the meta / directory handling of
agent0_amd/deepq/snapshot.py and the new exports."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import snapshot_ref as ref  # noqa: E402

FB = 64          # frame bytes of the CPU cases (a multiple of 16, like 7 056)


def cases():
    """name -> (rows [R][8][FB], stride): the cases tests/test_gpu_snapshot.py runs through the kernels too."""
    rng = np.random.default_rng(5)
    out = {"random": (rng.integers(0, 256, (24, 8, FB), dtype=np.uint8), 4)}
    out["sliding"] = (ref.window_rows(4, 6, FB)[0], 4)
    out["resets"] = (ref.window_rows(4, 6, FB, resets=[(1, 2), (3, 4), (0, 5)])[0], 4)
    out["nstep3"] = (ref.window_rows(4, 7, FB, n=3, resets=[(2, 3)])[0], 4)
    out["short_chunk"] = (ref.window_rows(8, 1, FB)[0][:5], 8)               # fewer rows than the stride: no row has a previous step in the chunk
    out["wrong_stride"] = (ref.window_rows(4, 6, FB)[0], 3)
    out["constant"] = (np.zeros((6, 8, FB), dtype=np.uint8), 2)               # every frame equal: one literal, chains through the whole chunk
    return out


@pytest.mark.parametrize("name", sorted(cases()))
def test_reference_round_trips(name):
    rows, stride = cases()[name]
    lit_id, n_lit, literals = ref.pack(rows, stride)
    assert literals.shape == (n_lit, FB) and lit_id.max() < n_lit
    assert np.array_equal(ref.unpack(lit_id, literals), rows)
    blob = ref.to_bytes(lit_id, n_lit, literals)
    assert len(blob) == ref.literal_offset(rows.shape[0] * 8) + n_lit * FB


def test_literal_count_is_derived():
    """E envs, S steps, n = 1, no resets, every emitted frame unique: an env's first row has 5 distinct frames (st's 4 + the newest of st_next), every later row 1."""
    E, S = 5, 7
    rows, emitted = ref.window_rows(E, S, FB)
    _, n_lit, _ = ref.pack(rows, E)
    assert n_lit == 5 * E + (S - 1) * E == emitted
    # one env's episode ends at step 3: the observation after it is a fresh stack of four frames instead of the window moved on by one — 3 frames more, all of them
    # first stored in that step's st_next; the next row's st finds them in the row `stride` earlier
    rows, emitted = ref.window_rows(E, S, FB, resets=[(2, 3)])
    _, n_lit2, _ = ref.pack(rows, E)
    assert n_lit2 == n_lit + 3 == emitted
    # with the wrong stride nothing is found in the previous row: every row keeps its 5 distinct frames
    _, n_lit3, _ = ref.pack(ref.window_rows(E, S, FB)[0], E + 1)
    assert n_lit3 == 5 * E * S


def test_meta_round_trip_geometry_and_tmp_dir(tmp_path):
    import torch
    from agent0_amd.deepq import snapshot as snap
    from agent0_amd.deepq.config import ExpConfig, to_dict
    cfg = ExpConfig()
    geo = snap.geometry(to_dict(cfg), "main", "device")
    chunks = [{"buf": "replay", "slot": 0, "rows": 7, "n_lit": 11, "bytes": 1234}]
    meta = snap.make_meta(to_dict(cfg), geo, chunks, 7056, {"seed": 3})
    d = str(tmp_path / "snapshot")
    tmp = snap.begin_write(d)
    for name in ("checkpoint.pth", "frames.bin"):
        open(os.path.join(tmp, name), "wb").close()
    torch.save({"meta": meta}, os.path.join(tmp, "state.pth"))
    with pytest.raises(FileNotFoundError):
        snap.resolve_dir(d)                                   # nothing committed yet: the .tmp directory is not a snapshot
    snap.commit_write(d)
    got = torch.load(os.path.join(snap.resolve_dir(d), "state.pth"), weights_only=True)["meta"]
    assert got == meta
    snap.check_meta(got)
    snap.check_geometry(got["geometry"], geo)
    # a second write killed before its rename: the committed snapshot is the one that loads, and the leftover does not stop the next write
    tmp = snap.begin_write(d)
    open(os.path.join(tmp, "state.pth"), "wb").write(b"half a fi")
    assert snap.resolve_dir(d) == d
    assert torch.load(os.path.join(snap.resolve_dir(d), "state.pth"), weights_only=True)["meta"] == meta
    tmp = snap.begin_write(d)
    assert os.listdir(tmp) == []
    # another geometry: refused, the key named
    cfg2 = ExpConfig()
    cfg2.replay.size = cfg.replay.size // 2
    cfg2.learner.n_step_q = 3
    with pytest.raises(ValueError, match=r"replay\.size.*learner\.n_step_q"):
        snap.check_geometry(got["geometry"], snap.geometry(to_dict(cfg2), "main", "device"))
    with pytest.raises(ValueError, match="schedule"):
        snap.check_geometry(got["geometry"], snap.geometry(to_dict(cfg), "launch", "device"))
    with pytest.raises(ValueError, match="format"):
        snap.check_meta(dict(meta, format=99))


def test_chunk_plan_walks_the_ring_in_age_order():
    from agent0_amd.deepq import snapshot as snap
    assert snap.chunk_plan(500, 192, 192) == [{"slot": 0, "rows": 192}]
    assert snap.chunk_plan(500, 500, 768, chunk_rows=200) == [{"slot": 268, "rows": 200}, {"slot": 468, "rows": 32}, {"slot": 0, "rows": 200}, {"slot": 200, "rows": 68}]
    assert snap.chunk_plan(500, 500, 1000) == [{"slot": 0, "rows": 500}]
    assert snap.chunk_plan(10000, 10000, 10000 + 5)[0] == {"slot": 5, "rows": 4096}
    assert sum(c["rows"] for c in snap.chunk_plan(10000, 10000, 10000 + 5)) == 10000


def test_state_blobs_round_trip():
    from agent0_amd.deepq import snapshot as snap
    rb = dict(size=500, obs_bytes=28224, B=32, prioritize=1, top=500, written=1344, epoch={"top": 384, "nb": 12, "pos": 5, "seed": 0x9ABCDEF0}, rng_seed=(7 << 32) | 12345,
              rng_off=[0, 4, 8, 0, 0, 64, 12, 0], beta_use=0.4000001, sched_cur=0.41, max_p=1.5, alpha=0.5, eps=0.01, beta0=0.4, total_steps=10**7)
    assert snap.parse_replay_blob(snap.replay_blob(**rb)) == rb
    E, T, n, K, ob = 3, 4, 3, 4, 32
    rng = np.random.default_rng(1)
    ad = dict(E=E, T=T, A=4, dueling=1, n_step=n, env_task=1, reset_noise_freq=4, discount=0.99, K=K, cur=2, g=48, steps=48, rng_seed=5, rng_off=[0, 8, 8, 0, 16, 0, 0, 0],
              env_seed=5, rank=0, obs=rng.integers(0, 256, K * E * ob, dtype=np.uint8), ep_ret=rng.random(E, dtype=np.float32), ring_act=rng.integers(0, 4, n * E).astype(np.int32),
              ring_rew=rng.random(n * E, dtype=np.float32), ring_done=np.zeros(n * E, dtype=np.float32), qs=rng.random(T, dtype=np.float32),
              stat_mask=np.ones(T * E, dtype=np.float32), stat_ret=rng.random(T * E, dtype=np.float32))
    got = snap.parse_actor_blob(snap.actor_blob(ad), ob)
    assert set(got) == set(ad)
    for k, v in ad.items():
        assert np.array_equal(got[k], v) if isinstance(v, np.ndarray) else got[k] == v, k
    with pytest.raises(ValueError, match="n_step"):
        snap.check_actor_desc(got, dict(got, n_step=1))


NEW_EXPORTS = ("a0_snapshot_pack_bound", "a0_snapshot_literal_offset", "a0_snapshot_pack", "a0_snapshot_unpack", "a0_rbuf_state_size", "a0_rbuf_state_save", "a0_rbuf_state_load",
               "a0_actor_state_size", "a0_actor_state_save", "a0_actor_state_load", "a0_learner_rng_state")


def test_new_exports_are_declared_bound_and_validated():
    from agent0_amd import _abi
    names = {n for _, n, _ in _abi.parse_header()}
    assert not [n for n in NEW_EXPORTS if n not in names]
    lib = _abi.load()                       # dlopen + argtypes for every prototype; works without a GPU
    for n in NEW_EXPORTS:
        assert getattr(lib, n).argtypes is not None
    ops_src = open(os.path.join(ROOT, "agent0_amd", "ops.py")).read()
    for n in ("a0_snapshot_pack_bound", "a0_snapshot_pack", "a0_snapshot_unpack"):
        assert re.search(rf"self\.lib\.{n}\(", ops_src), n
    # argument validation happens before any HIP call
    F, fb = 8, 7056
    assert lib.a0_snapshot_pack_bound(4096, F, fb) == ref.literal_offset(4096 * F) + 4096 * F * fb == 231_342_096
    assert lib.a0_snapshot_pack_bound(4097, F, fb) == -1 and "32768 frames" in _abi.last_error()
    assert lib.a0_snapshot_pack_bound(16, F, 7000) == -1
    assert lib.a0_snapshot_literal_offset(3, 8) == ref.literal_offset(24)
    assert lib.a0_snapshot_pack(None, 16, F, fb, 16, None, None, None) == -1 and "a0_snapshot_pack" in _abi.last_error()
    assert lib.a0_snapshot_unpack(None, 16, F, fb, None, None, None) == -1
    assert lib.a0_rbuf_state_save(None, None, 0, None) == -1 and lib.a0_actor_state_load(None, None, 0, None) == -1 and lib.a0_learner_rng_state(None, None, 0) == -1
    assert lib.a0_rbuf_state_size(None) == 0 and lib.a0_actor_state_size(None) == 0


def test_the_new_kernels_use_no_scratch():
    from agent0_amd import _abi
    path = os.path.join(os.path.dirname(_abi.LIB_PATH), "kernel_resources.txt")
    rows = [line.split() for line in open(path) if line.startswith("snapshot ")]
    assert len(rows) == 4, rows
    for r in rows:
        kv = dict(x.split("=") for x in r[2:])
        assert int(kv["scratch"]) == 0 and int(kv["vgpr_spill"]) == 0 and int(kv["sgpr_spill"]) == 0, r


def test_snapshot_freq_is_a_config_key_and_off_by_default():
    from agent0_amd.deepq.config import ExpConfig, parse_overrides
    assert ExpConfig().trainer.snapshot_freq == 0
    assert parse_overrides(["trainer.snapshot_freq=25", "wandb=false", "tb=false"]).trainer.snapshot_freq == 25
