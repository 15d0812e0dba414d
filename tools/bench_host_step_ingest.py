"""Device time of the ingest half of a host-env step: ONE a0_host_step_ingest launch against the launches Actor._rollout_host composes today
(a0_env_frame_stack, the observation-ring copy for n > 1, a0_actor_nstep, a0_replay_insert, two statistics copies), alternating, on the same buffers.
Prints one JSON line per (E, n): microseconds per step for both forms (device events around `--iters` steps), the HBM bytes the step has to move and
that floor's time at the 8 TB/s peak.  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times.

    python tools/bench_host_step_ingest.py --iters 200 > events.jsonl
    rocprofv3 --kernel-trace --stats -d trace -o ingest -- python tools/bench_host_step_ingest.py --iters 50 --rounds 1
    python tools/bench_host_step_ingest.py --trace trace/ingest_results.db --events events.jsonl > profiles/r08_host_step_ingest.jsonl

The last form runs nothing on the GPU: it merges the event timings with the trace's per-kernel times (median over the 50 traced steps of each form).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BPS = 8.0e12          # MI355X HBM3E peak (MI355X_MICROARCH.md)


def merge(db: str, events: str, iters: int = 50, warm: int = 20):
    """One line per (E, n): the event timings of ``events`` with the kernel trace of the traced run (``--iters 50 --rounds 1``: per configuration 20 + 20
    warm-up steps, then 50 of the ingest form and 50 of the composed form)."""
    import sqlite3
    import statistics as S
    ev = [json.loads(x) for x in open(events) if x.startswith("{")]
    rows = sqlite3.connect(db).execute("select name, duration, start from kernels order by start").fetchall()
    ing = [r for r in rows if "host_step_ingest" in r[0]]
    per_cfg = warm + iters
    bounds = [ing[i * per_cfg][2] for i in range(len(ev))] + [float("inf")]
    for k, e in enumerate(ev):
        seg = [r for r in rows if bounds[k] <= r[2] < bounds[k + 1]]
        fi = [r for r in seg if "host_step_ingest" in r[0]]
        comp = [r for r in seg if r[2] > fi[-1][2] and "at::native" not in r[0]]      # the composed form's timed steps (not the next configuration's set-up)
        per = {}
        for r in comp:
            per.setdefault("hipMemcpyAsync D2D (copyBuffer)" if "copyBuffer" in r[0] else r[0].split("(")[0], []).append(r[1] / 1e3)
        ingest_us = S.median([r[1] for r in fi[warm:]]) / 1e3
        print(json.dumps({"E": e["E"], "n": e["n"], "ingest_launches_per_step": 1, "ingest_us_median": round(ingest_us, 2),
                          "composed_launches_per_step": round(len(comp) / iters, 2), "composed_kernel_us_per_step": round(sum(r[1] for r in comp) / 1e3 / iters, 2),
                          "composed_kernels": {n: {"per_step": round(len(v) / iters, 2), "median_us": round(S.median(v), 2)} for n, v in per.items()},
                          "event_us_per_step": {"fused": e["fused_us"], "composed": e["composed_us"], "fused_all": e["fused_us_all"], "composed_all": e["composed_us_all"]},
                          "hbm_bytes": e["hbm_bytes"], "hbm_floor_us_at_8TBps": e["hbm_floor_us_at_8TBps"],
                          "effective_rate_over_8TBps": round(e["hbm_floor_us_at_8TBps"] / ingest_us, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", help="rocprofv3 database of a traced run: merge it with --events instead of measuring")
    ap.add_argument("--events", help="the JSON lines of an untraced run")
    args = ap.parse_args()
    if args.trace:
        return merge(args.trace, args.events)
    from agent0_amd.ops import HipOps
    hip = HipOps()
    dev = hip.device
    nstack, fb, gamma = 4, 84 * 84, 0.99
    ob = nstack * fb
    g = torch.Generator(device="cpu").manual_seed(1)
    for E in (16, 256):
        for n in (1, 3):
            R = n + 1 if n > 1 else 1
            cap = 64 * E
            u8 = lambda k: torch.randint(0, 256, (k,), generator=g, dtype=torch.uint8).to(dev)
            obs = [u8(E * ob), u8(E * ob)]
            newest = u8(E * fb)
            scal = torch.zeros(7, E)
            scal[0] = (torch.rand(E, generator=g) < 0.1).float()
            scal[6] = (torch.rand(E, generator=g) < 0.98).float()        # a step of a real emulator: almost every stack merely advances
            scal = scal.to(dev)
            action = torch.zeros(E, dtype=torch.int32, device=dev)
            z = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=dev)
            ring_act, ring_rew, ring_done = z(n * E, torch.int32), z(n * E), z(n * E)
            ring_obs = z(R * E * ob, torch.uint8) if n > 1 else None
            frames, r_act, r_rew, r_done = z(cap * 2 * ob, torch.uint8), z(cap, torch.int32), z(cap), z(cap)
            stat_mask, stat_ret = z(64 * E), z(64 * E)
            out_act, out_rew, out_done = z(E, torch.int32), z(E), z(E)

            def fused(t):
                prev, out = obs[t & 1], obs[(t & 1) ^ 1]
                sl = slice((t % 64) * E, (t % 64 + 1) * E)
                hip.host_step_ingest(prev, newest, scal, out, E, nstack, fb, True, action, n, R, t, gamma, ring_act, ring_rew, ring_done, ring_obs, frames, cap,
                                     (t * E) % cap, r_act, r_rew, r_done, stat_mask[sl], stat_ret[sl])

            def composed(t):
                prev, out = obs[t & 1], obs[(t & 1) ^ 1]
                sl = slice((t % 64) * E, (t % 64 + 1) * E)
                hip.env_frame_stack(prev, newest, scal[6], out, E, nstack, fb)
                stat_mask[sl].copy_(scal[4])
                stat_ret[sl].copy_(scal[5])
                if n > 1:
                    rs = t % R
                    ring_obs[rs * E * ob:(rs + 1) * E * ob].copy_(prev)
                    old = (t - (min(t + 1, n) - 1)) % R
                    obs0 = ring_obs[old * E * ob:(old + 1) * E * ob]
                else:
                    obs0 = prev
                hip.actor_nstep(E, n, t, gamma, action, scal[0], scal[1], scal[2], scal[3], ring_act, ring_rew, ring_done, out_act, out_rew, out_done)
                hip.replay_insert(frames, cap, ob, (t * E) % cap, E, obs0, out, out_act, out_rew, out_done, r_act, r_rew, r_done)

            res = {"fused": [], "composed": []}
            for name, fn in (("fused", fused), ("composed", composed)):          # warm-up of both forms
                for t in range(20):
                    fn(t)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in (("fused", fused), ("composed", composed)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for t in range(args.iters):
                        fn(t + 20)
                    b.record()
                    b.synchronize()
                    res[name].append(a.elapsed_time(b) * 1e3 / args.iters)
            adv = float(scal[6].sum())
            # bytes the step must move: prev read, the newest frame of the advanced rows, out written for the advanced rows (the others were uploaded whole and
            # are read instead), the 2 x ob replay row; n > 1: the ring entry written and the oldest entry read
            moved = E * ob + adv * (fb + ob) + (E - adv) * ob + E * 2 * ob + (2 * E * ob if n > 1 else 0)
            print(json.dumps({"E": E, "n": n, "fused_us": round(min(res["fused"]), 2), "composed_us": round(min(res["composed"]), 2),
                              "fused_us_all": [round(x, 2) for x in res["fused"]], "composed_us_all": [round(x, 2) for x in res["composed"]],
                              "hbm_bytes": int(moved), "hbm_floor_us_at_8TBps": round(moved / PEAK_BPS * 1e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
