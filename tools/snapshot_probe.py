"""Measures the replay snapshot (profiles/r09_snapshot.md): packed size of a ring the device env filled, pack / unpack kernel throughput against a plain
device-to-device copy of the same rows (HIP event pairs), and the wall time of a whole save_snapshot / load_snapshot.

    python tools/snapshot_probe.py [replay.size] [iterations] [directory]
"""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 81920
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_dir = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp()
    mk = lambda seed: Trainer(parse_overrides(["env_id=Breakout", "learner.algo=dqn", "actor.num_envs=256", "actor.sample_steps=80", f"replay.size={size}", "learner.batch_size=512",
                                               "trainer.training_start_steps=20000", "wandb=false", "tb=false", f"seed={seed}", f"logdir={out_dir}/run{seed}"]))
    tr = mk(42)
    for i in range(iters):
        tr.run_iteration()
    rp, ops = tr.replay, tr.ops
    rows, fb = min(4096, rp.top), rp.obs_bytes // 4
    chunk = rp.frames[: rows * rp.row_bytes]
    packed = torch.empty(ops.snapshot_pack_bound(rows, 8, fb), dtype=torch.uint8, device=ops.device)
    work = torch.empty(rows * 8, dtype=torch.int32, device=ops.device)
    dst = torch.empty_like(chunk)
    gb = chunk.numel() / 1e9
    res = {"replay_size": size, "rows_filled": int(rp.top), "chunk_rows": rows,
           "copy_GBps": gb / (timed(lambda: dst.copy_(chunk)) / 1e3),
           "pack_GBps": gb / (timed(lambda: ops.snapshot_pack(chunk, rows, 8, fb, 256, packed, work)) / 1e3),
           "unpack_GBps": gb / (timed(lambda: ops.snapshot_unpack(packed, rows, 8, fb, dst)) / 1e3)}
    assert torch.equal(dst, chunk)
    t0 = time.time()
    d = tr.save_snapshot(os.path.join(out_dir, "snapshot"))
    res["save_s"] = time.time() - t0
    meta = torch.load(os.path.join(d, "state.pth"), weights_only=True)["meta"]
    res.update(packed_bytes=meta["packed_bytes"], ring_bytes=meta["ring_bytes"], ratio=meta["ring_bytes"] / meta["packed_bytes"])
    tr.test = lambda: None
    tr.final(save=False)
    del tr, chunk, dst
    torch.cuda.empty_cache()
    tr = mk(7)
    t0 = time.time()
    tr.load_snapshot(d)
    res["load_s"] = time.time() - t0
    tr.test = lambda: None
    tr.final(save=False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
