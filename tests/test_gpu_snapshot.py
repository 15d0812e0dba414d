"""Resumable snapshots on the GPU: the pack / unpack kernels against the numpy reference (tests/snapshot_ref.py), and ``Trainer.save_snapshot`` /
``load_snapshot``: a fresh Trainer that loaded a snapshot continues THE SAME run, bit for bit, under the library's handles and under the Python classes."""
import csv
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import snapshot_ref as ref  # noqa: E402
from test_snapshot_format import cases  # noqa: E402


def _pack(ops, rows: np.ndarray, stride: int):
    R, F, fb = rows.shape
    dev = torch.from_numpy(rows.reshape(-1).copy()).to(ops.device)
    packed = torch.zeros(ops.snapshot_pack_bound(R, F, fb), dtype=torch.uint8, device=ops.device)
    work = torch.zeros(R * F, dtype=torch.int32, device=ops.device)
    ops.snapshot_pack(dev, R, F, fb, stride, packed, work)
    torch.cuda.synchronize()
    return dev, packed


@pytest.mark.parametrize("name", sorted(cases()))
def test_pack_equals_the_numpy_reference_and_unpack_inverts_it(name):
    from agent0_amd.ops import HipOps
    ops = HipOps()
    rows, stride = cases()[name]
    R, F, fb = rows.shape
    lit_id, n_lit, literals = ref.pack(rows, stride)
    dev, packed = _pack(ops, rows, stride)
    want = torch.from_numpy(np.frombuffer(ref.to_bytes(lit_id, n_lit, literals), dtype=np.uint8).copy())
    off = ref.literal_offset(R * F)
    got = packed.cpu()
    assert torch.equal(got[: R * F * 4].view(torch.int32), want[: R * F * 4].view(torch.int32)), "lit_id"
    assert int(got[R * F * 4: R * F * 4 + 4].view(torch.int32)[0]) == n_lit, "literal count"
    assert torch.equal(got[off: off + n_lit * fb], want[off:]), "literal bytes"
    assert torch.equal(got[: want.numel()], want)
    # packing the same rows twice gives identical bytes
    _, again = _pack(ops, rows, stride)
    assert torch.equal(again, packed)
    out = torch.full_like(dev, 0xA5)
    bad = torch.zeros(1, dtype=torch.int32, device=ops.device)
    ops.snapshot_unpack(packed, R, F, fb, out, bad)
    torch.cuda.synchronize()
    assert torch.equal(out, dev) and int(bad[0]) == 0


def test_pack_at_the_ring_frame_size_and_a_full_chunk():
    """7 056-byte frames (441 vectors: the last pass of a wavefront is partial), 4 096 rows — the largest chunk, 32 768 frames through the one-workgroup resolve."""
    from agent0_amd.ops import HipOps
    ops = HipOps()
    E, S, fb = 256, 16, 7056
    rows, _ = ref.window_rows(E, S, fb, resets=[(3, 4), (200, 9)], seed=3)
    dev, packed = _pack(ops, rows, E)
    n = E * S * 8
    n_lit = int(packed[n * 4: n * 4 + 4].view(torch.int32)[0])
    assert n_lit == 5 * E + (S - 1) * E + 2 * 3, "derived: tests/test_snapshot_format.py::test_literal_count_is_derived"
    out = torch.zeros_like(dev)
    ops.snapshot_unpack(packed, E * S, 8, fb, out)
    torch.cuda.synchronize()
    assert torch.equal(out, dev)
    # a damaged table is caught, not followed
    packed[:4].view(torch.int32)[0] = n_lit + 7
    bad = torch.zeros(1, dtype=torch.int32, device=ops.device)
    ops.snapshot_unpack(packed, E * S, 8, fb, out, bad)
    torch.cuda.synchronize()
    assert int(bad[0]) == 1


def test_a_wrapped_ring_unpacks_into_the_same_slots(tmp_path):
    """``written > size``: the chunks walk the ring in age order across the wrap; a fresh ring gets every row back at its slot."""
    from agent0_amd.deepq import snapshot as snap
    from agent0_amd.ops import HipOps
    ops = HipOps()
    size, E, fb = 300, 16, 7056
    rows, _ = ref.window_rows(E, 26, fb, seed=9)                # 416 rows written into 300 slots
    written = rows.shape[0]
    ring = torch.zeros(size * 8 * fb, dtype=torch.uint8, device=ops.device)
    flat = torch.from_numpy(rows.reshape(written, -1))
    for i in range(written):
        ring[(i % size) * 8 * fb:((i % size) + 1) * 8 * fb] = flat[i].to(ops.device)
    plan = snap.chunk_plan(size, size, written, chunk_rows=128)
    assert plan[0]["slot"] == written % size and sum(c["rows"] for c in plan) == size
    ff = snap.FrameFile(ops, fb, 128)
    with open(tmp_path / "frames.bin", "wb") as f:
        chunks = ff.write(f, ring, plan, E, "replay")
    assert sum(c["bytes"] for c in chunks) == os.path.getsize(tmp_path / "frames.bin") < ring.numel() // 4
    fresh = torch.zeros_like(ring)
    with open(tmp_path / "frames.bin", "rb") as f:
        snap.FrameFile(ops, fb, 128).read(f, fresh, chunks)
    assert torch.equal(fresh, ring)


# ----------------------------------------------------------------------------- the run continues
CONFIGS = {
    "dqn": ("dqn", [], False),
    "rainbow-lite": ("c51", ["learner.noisy_net=true", "learner.n_step_q=3", "replay.policy=prioritize"], False),
    "iqn": ("iqn", [], False),
    "fqf-duel": ("fqf", ["learner.dueling_head=true"], False),
    "dqn-flat-per": ("dqn", ["replay.sumtree=false", "replay.policy=prioritize"], False),
    "dqn-launch": ("dqn", [], True),
}


def _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, seed, tag):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = parse_overrides([f"learner.algo={algo}", "actor.num_envs=16", "actor.sample_steps=12", "learner.batch_size=32", "learner.learner_steps=3", "replay.size=500",
                           "trainer.training_start_steps=100", "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false", "tb=false", f"seed={seed}",
                           f"logdir={tmp_path / tag}"] + list(extra))
    return Trainer(cfg, use_lp=use_lp)


def _state(tr):
    torch.cuda.synchronize()
    eng, rp = tr.learner.engine, tr.replay
    prio = (rp.tree if rp.use_sumtree else rp.priority).clone() if rp.prioritize else torch.zeros(1)
    return [eng.online.flat.clone(), eng.target.flat.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.state.clone(), rp.frames.clone(), rp.act.clone(), rp.rew.clone(),
            rp.done.clone(), prio, rp._pstate.clone()]


def _close(tr):
    tr.test = lambda: None
    tr.final(save=False)


PREFETCH = lambda i: i % 3 != 1          # iterations 0 .. 7: the rollout of iteration 5 has been issued ahead when the snapshot is taken after iteration 4


def _continues(tmp_path, monkeypatch, name, save_native, load_native):
    from agent0_amd.deepq.native_loop import NativeLoop
    algo, extra, use_lp = CONFIGS[name]
    keys = ("loss", "return_train", "qmax", "frames")
    # run A: eight iterations
    tr = _trainer(tmp_path, monkeypatch, save_native, algo, extra, use_lp, 42, "a")
    res_a = [tr.run_iteration(prefetch=PREFETCH(i)) for i in range(8)]
    assert isinstance(tr._nl, NativeLoop) if save_native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    assert tr.replay.written > tr.replay.size, "the ring wrapped"
    want = _state(tr)
    _close(tr)
    # run B: four iterations, snapshot; a NEW Trainer built with another seed loads it and runs four more
    tr = _trainer(tmp_path, monkeypatch, save_native, algo, extra, use_lp, 42, "b")
    for i in range(4):
        tr.run_iteration(prefetch=PREFETCH(i))
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    saved = _state(tr)
    _close(tr)
    assert sorted(os.listdir(snap_dir)) == ["checkpoint.pth", "frames.bin", "state.pth"] and not os.path.exists(snap_dir + ".tmp")
    tr = _trainer(tmp_path, monkeypatch, load_native, algo, extra, use_lp, 7, "c")
    tr.load_snapshot(snap_dir)
    for i, (x, y) in enumerate(zip(_state(tr), saved)):
        assert torch.equal(x, y), f"right after the load: item {i}"
    res_b = [tr.run_iteration(prefetch=PREFETCH(i)) for i in range(4, 8)]
    assert isinstance(tr._nl, NativeLoop) if load_native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    got = _state(tr)
    _close(tr)
    for i, (a, b) in enumerate(zip(res_a[4:], res_b)):
        print(name, "iteration", i + 5, {k: (a[k], b[k]) for k in keys})
        assert all(a[k] == b[k] for k in keys), f"iteration {i + 5}: {[(k, a[k], b[k]) for k in keys]}"
    assert res_a[7]["loss"] is not None, "updates ran"
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), f"after iteration 8: item {i}"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_a_loaded_snapshot_continues_the_same_run(name, native, tmp_path, monkeypatch):
    _continues(tmp_path, monkeypatch, name, native, native)


@pytest.mark.parametrize("save_native,load_native", [(True, False), (False, True)], ids=["handles-to-classes", "classes-to-handles"])
def test_a_snapshot_written_under_one_host_loop_loads_under_the_other(save_native, load_native, tmp_path, monkeypatch):
    _continues(tmp_path, monkeypatch, "rainbow-lite", save_native, load_native)


def test_a_snapshot_of_another_geometry_is_refused(tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, True, "dqn", [], False, 42, "a")
    for i in range(2):
        tr.run_iteration()
    d = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    os.makedirs(d + ".tmp")                                    # an interrupted later write: ignored
    tr = _trainer(tmp_path, monkeypatch, True, "dqn", ["learner.n_step_q=3"], False, 42, "b")
    with pytest.raises(ValueError, match=r"learner\.n_step_q"):
        tr.load_snapshot(d)
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, True, "dqn", [], False, 42, "c")
    tr.load_snapshot(d)
    assert tr.frame_count == 2 * 192 and len(tr.replay) == 384
    _close(tr)


def test_main_entry_point_writes_and_resumes_a_snapshot(tmp_path):
    logdir = str(tmp_path / "runs")
    base = [sys.executable, "-m", "agent0.deepq.main", "env_id=Breakout", "learner.algo=dqn", "actor.num_envs=16", "actor.sample_steps=12", "learner.batch_size=32",
            "learner.learner_steps=3", "replay.size=500", "trainer.training_start_steps=100", "trainer.test_episodes=2", "device=cuda", "wandb=false", "tb=false",
            f"logdir={logdir}", "trainer.snapshot_freq=2"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(base + ["trainer.total_steps=2000"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = glob.glob(os.path.join(logdir, "*"))
    assert len(runs) == 1
    snap_dir = os.path.join(runs[0], "snapshot")
    assert sorted(os.listdir(snap_dir)) == ["checkpoint.pth", "frames.bin", "state.pth"]
    first = [int(float(x["frames"])) for x in csv.DictReader(open(os.path.join(runs[0], "progress.csv")))]
    assert first == [192 * (i + 1) for i in range(11)]
    r = subprocess.run(base + ["trainer.total_steps=3000", "mode=finetune", f"checkpoint={snap_dir}", "seed=9"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    second = [d for d in glob.glob(os.path.join(logdir, "*")) if d != runs[0]]
    assert len(second) == 1
    rows = list(csv.DictReader(open(os.path.join(second[0], "progress.csv"))))
    assert [int(float(x["frames"])) for x in rows] == [first[-1] + 192 * (i + 1) for i in range(5)], "the frame column goes on from the first run's"
    assert rows[0]["loss"] != "" and np.isfinite(float(rows[0]["loss"])), "the resumed run trains from its first iteration: the replay came back full"


def test_host_env_snapshot_restores_learner_and_replay_and_resets_the_envs(tmp_path, monkeypatch):
    """Host environments cannot be saved: learner, replay and sampler come back exactly, the envs are reset, the actor's n-step windows start empty, and the run
    trains on — that, not bit equality of the continuation, is the promise."""
    from test_gpu_native_host_envs import _trainer as host_trainer
    tr, _ = host_trainer(tmp_path, monkeypatch, True, tag="a")
    for i in range(4):
        tr.run_iteration(prefetch=(i % 2 == 0))
    d = tr.save_snapshot(str(tmp_path / "snap"))
    saved, frames, upd = _state(tr), tr.frame_count, tr.learner.update_steps
    tr.final(save=False)
    tr, _ = host_trainer(tmp_path, monkeypatch, True, tag="b")
    try:
        tr.load_snapshot(d)
        for i, (x, y) in enumerate(zip(_state(tr), saved)):
            assert torch.equal(x, y), f"right after the load: item {i}"
        assert tr.frame_count == frames and tr.learner.update_steps == upd and upd > 0
        assert tr.actors[1].steps == 0, "a fresh actor: empty n-step windows over reset envs"
        out = [tr.run_iteration() for _ in range(3)]
        assert all(np.isfinite(o["loss"]) for o in out) and tr.learner.update_steps == upd + 9 and tr.frame_count == frames + 3 * 192
    finally:
        tr.final(save=False)
