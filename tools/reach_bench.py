"""pwn_trace_reach_device against pwn_trace_hits_device, the existing, unchanged call that is the yardstick: the same 2^20
crosshair-like rays -- one ray each of 2^20 viewers that stand around a point and look about -- at reach 0.35, 2, 20 and +inf, on
level.txt (the golden spheres) and on the hall of mirrors (a corridor closed on itself by a portal pair, where a ray that meets no
floor walks to the step limit).

One JSON line per scene: device time by HIP events around each launch on one stream, the five calls ALTERNATING in one run, median,
minimum and the 10th / 90th percentile of --reps after --warmup; the `steps` counter of each call from one launch more with
PWN_OPT_COUNTERS on (a counting kernel is another kernel: not timed); the kinds of the records.

    python tools/reach_bench.py [--reps 30] [--warmup 5] [--rays 1048576] [--out file.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
LEVEL = os.path.join(GOLD, "levels", "pwnfps_level.txt")
MIRRORS = ".........\n.A;;*;;A.\n.........\n"
REACHES = (0.35, 2.0, 20.0, float("inf"))


def crosshair_rays(n, centre, spread, yaw_range, pitch, seed):
    """n ray records: origins within `spread` of centre (x, y, z) in x and z, yaws uniform in yaw_range, pitches within +-pitch"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0] = centre[0] + rng.uniform(-spread, spread, n)
    rec[:, 1] = centre[1]
    rec[:, 2] = centre[2] + rng.uniform(-spread, spread, n)
    rec[:, 3] = 1.0
    yaw = rng.uniform(yaw_range[0], yaw_range[1], n)
    p = rng.uniform(-pitch, pitch, n)
    rec[:, 4] = np.sin(yaw) * np.cos(p)
    rec[:, 5] = np.sin(p)
    rec[:, 6] = np.cos(yaw) * np.cos(p)
    # (neighbouring rays look the same way, as the crosshairs of viewers in one room do: sorted by yaw, the caller's order is the
    # coherence a batch of rays has -- include/pwnhip.h)
    return np.ascontiguousarray(rec[np.argsort(yaw, kind="stable")])


def scene(name, r, n):
    import pwnfps_amd
    if name == "level":
        r.level_load(LEVEL)
        r.set_objects(np.load(os.path.join(GOLD, "spheres_t0.npy")))
        _, _, spawn = r.get_level()
        return crosshair_rays(n, (spawn[0] + 0.5, 0.5, spawn[1] + 0.5), 0.3, (0.0, 2.0 * np.pi), 0.25, 1)
    r.level_load_text(MIRRORS)
    r.set_objects(np.zeros(0, pwnfps_amd.SPHERE_DTYPE))
    # along the corridor, both ways, nearly level: most rays walk for hundreds of cells
    rays = crosshair_rays(n, (4.5, 0.5, 1.5), 0.2, (0.5 * np.pi - 0.05, 0.5 * np.pi + 0.05), 0.002, 2)
    rays[::2, 4] *= -1.0
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import pwnfps_amd
    assert torch.cuda.is_available(), "reach_bench.py measures on the GPU"
    out = open(args.out, "w") if args.out else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = args.rays
    for name in ("level", "mirrors"):
        r = pwnfps_amd.Renderer(64, 64)
        rays = scene(name, r, n)
        t_rays = torch.from_numpy(rays).to(dev)
        t_hits = torch.zeros((n, 12), dtype=torch.int32, device=dev)
        t_reach = {v: torch.full((n,), v, dtype=torch.float32, device=dev) for v in REACHES}
        fns = {"hits": lambda: r.trace_hits_device(t_rays, t_hits, stream=stream)}
        for v in REACHES:
            fns["reach_%g" % v] = (lambda v=v: r.trace_reach_device(t_rays, t_reach[v], t_hits, stream=stream))
        ts = {k: [] for k in fns}
        for i in range(args.warmup + args.reps):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    a.record(stream)
                    fn()
                    b.record(stream)
                b.synchronize()
                if i >= args.warmup:
                    ts[k].append(a.elapsed_time(b))
        res = {"scene": name, "rays": n, "reps": args.reps, "warmup": args.warmup}
        r.set_counters(True)
        for k, fn in fns.items():
            with torch.cuda.stream(stream):
                fn()
            stream.synchronize()
            st = r.stats()
            kinds = [int((t_hits[:, 0] == q).sum().item()) for q in range(4)]
            v = np.array(ts[k])
            res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                      "p90_ms": round(float(np.percentile(v, 90)), 4), "steps": int(st["steps"]), "kinds_none_wall_sphere_free": kinds}
        base = res["hits"]
        for k in fns:
            res[k]["time_over_hits"] = round(res[k]["median_ms"] / base["median_ms"], 3)
            res[k]["steps_over_hits"] = round(res[k]["steps"] / base["steps"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        r.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
