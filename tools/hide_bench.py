"""What one hidden sphere per view costs: pwn_trace_views_hide_device beside pwn_trace_views_device, on the batch of
tools/views_bench.py --device-form (the level.txt scene with the t0 spheres, that tool's seeded cameras around the spawn).

Four variants take turns inside every repetition (the order moves on by one with every repetition, so that none always runs behind
the same neighbour), in one process, on one context and one stream, blur off -- so that what is timed is the camera set-up launch
and the trace launch, nothing else:
  plain_a, plain_b   pwn_trace_views_device, twice: the difference between the two is the run-to-run spread of the SAME code
  hide_none          pwn_trace_views_hide_device with every entry PWN_HIDE_NONE (the HIDE kernels, nothing hidden)
  hide_real          pwn_trace_views_hide_device with hide[i] = i mod (number of spheres)
Each is timed by HIP events on the stream around the call (median over --reps, after --warmup).  The plain call's kernels are the
parent commit's instruction for instruction (profiles/hide/isa_resources.txt), so plain_a / plain_b stand for the parent.
One JSON line per case; --out also writes them to a file.

    python tools/hide_bench.py [--reps 1000] [--sizes 320x240] [--views 64,256] [--out profiles/hide/bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="320x240")
    ap.add_argument("--views", default="64,256")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import pwnfps_amd
    from views_bench import cameras
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = open(args.out, "w") if args.out else None
    names = ("plain_a", "hide_none", "hide_real", "plain_b")
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = pwnfps_amd.Renderer(w, h)
        r.level_load(level)
        r.set_objects(sph)
        r.set_blur_passes(0)
        _, _, spawn = r.get_level()
        for n in (int(v) for v in args.views.split(",")):
            cams, secs = cameras(spawn, n, args.seed + n)
            with torch.cuda.stream(stream):
                t_cams = torch.from_numpy(cams.reshape(n, 16)).to(dev)
                t_secs = torch.from_numpy(secs).to(dev)
                t_sb = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
                t_z = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
                hides = {"plain_a": None, "plain_b": None,
                         "hide_none": torch.full((n,), -1, dtype=torch.int32, device=dev),
                         "hide_real": (torch.arange(n, dtype=torch.int32, device=dev) % len(sph)).contiguous()}
            stream.synchronize()
            ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in names}
            ms = {k: [] for k in names}
            planes = {}
            for rep in range(args.warmup + args.reps):
                for k in names[rep % 4:] + names[:rep % 4]:
                    ev[k][0].record(stream)
                    r.trace_views_device(t_cams, t_secs, t_sb, t_z, stream=stream, hide=hides[k])
                    ev[k][1].record(stream)
                    if rep == 0:
                        stream.synchronize()
                        planes[k] = t_sb.cpu().numpy().copy()
                stream.synchronize()
                if rep >= args.warmup:
                    for k in names:
                        ms[k].append(ev[k][0].elapsed_time(ev[k][1]))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            plain = 0.5 * (med["plain_a"] + med["plain_b"])
            rec = {"w": w, "h": h, "views": n, "reps": args.reps, "spheres": int(len(sph)),
                   "plain_a_ms": round(med["plain_a"], 5), "plain_b_ms": round(med["plain_b"], 5),
                   "hide_none_ms": round(med["hide_none"], 5), "hide_real_ms": round(med["hide_real"], 5),
                   "plain_spread_pct": round(100.0 * abs(med["plain_a"] - med["plain_b"]) / plain, 2),
                   "plain_p10_p90_ms": [round(float(np.percentile(ms["plain_a"] + ms["plain_b"], q)), 5) for q in (10, 90)],
                   "min_ms": {k: round(float(np.min(ms[k])), 5) for k in names},
                   "hide_none_over_plain_pct": round(100.0 * (med["hide_none"] / plain - 1.0), 2),
                   "hide_real_over_plain_pct": round(100.0 * (med["hide_real"] / plain - 1.0), 2),
                   "hide_none_same_pixels": bool((planes["hide_none"] == planes["plain_a"]).all()),
                   "hide_real_pixels_changed": int((planes["hide_real"] != planes["plain_a"]).sum())}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()
        r.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
