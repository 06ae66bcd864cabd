"""What one hidden sphere per rectangle or ray costs when nothing is hidden: pwn_trace_viewports_hide_device,
pwn_trace_viewport_hits_hide_device and pwn_trace_rays_hide_device beside the calls they shadow (tools/hide_bench.py's method, for
the other three families).  The level.txt scene with the t0 spheres, tools/views_bench.py's seeded cameras around the spawn.

Workloads: `grid64`, a 64-view atlas of 64 x 48 views (a frame of 512 x 384), and `L1`, layout L1 of tools/viewports_bench.py (eight
views of 4 x 4 to 196 x 108 pixels that tile 336 x 208), each as colour (blur off) and as first-hit planes; `rays`, the pixel rays of
the grid's 64 cameras at 64 x 48 (196 608 rays) as colour rays.

Four variants take turns inside every repetition (the order moves on by one with every repetition), in one process, on one context and
one stream:
  plain_a, plain_b   the call without `_hide`, twice: the difference between the two is the run-to-run spread of the SAME code
  hide_none          the `_hide` call with every entry PWN_HIDE_NONE (the HIDE kernels, nothing hidden)
  hide_real          the `_hide` call with hide[i] = i mod (number of spheres)
Each is timed by HIP events on the stream around the call (median over --reps, after --warmup); the whole measurement is made
--repeats times.  The plain calls' kernels are the parent commit's instruction for instruction
(profiles/hide_viewports/isa_resources.txt), so plain_a / plain_b stand for the parent.  One JSON line per case and repeat.

    python tools/hide_viewports_bench.py [--reps 1000] [--repeats 2] [--out profiles/hide_viewports/bench.txt]
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
L1 = (336, 208, [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
                 (100, 138, 36, 70), (140, 100, 196, 108)])
GRID64 = (512, 384, [(64 * (i % 8), 48 * (i // 8), 64, 48) for i in range(64)])
NAMES = ("plain_a", "hide_none", "hide_real", "plain_b")


def measure(torch, stream, call, result, reps, warmup):
    """call(name) enqueues one variant; result() -> the plane to compare, as numpy"""
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in NAMES}
    ms = {k: [] for k in NAMES}
    planes = {}
    for rep in range(warmup + reps):
        for k in NAMES[rep % 4:] + NAMES[:rep % 4]:
            ev[k][0].record(stream)
            call(k)
            ev[k][1].record(stream)
            if rep == 0:
                stream.synchronize()
                planes[k] = result().copy()
        stream.synchronize()
        if rep >= warmup:
            for k in NAMES:
                ms[k].append(ev[k][0].elapsed_time(ev[k][1]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    plain = 0.5 * (med["plain_a"] + med["plain_b"])
    return {"reps": reps, "plain_a_ms": round(med["plain_a"], 5), "plain_b_ms": round(med["plain_b"], 5),
            "hide_none_ms": round(med["hide_none"], 5), "hide_real_ms": round(med["hide_real"], 5),
            "plain_spread_pct": round(100.0 * abs(med["plain_a"] - med["plain_b"]) / plain, 2),
            "plain_p10_p90_ms": [round(float(np.percentile(ms["plain_a"] + ms["plain_b"], q)), 5) for q in (10, 90)],
            "min_ms": {k: round(float(np.min(ms[k])), 5) for k in NAMES},
            "hide_none_over_plain_pct": round(100.0 * (med["hide_none"] / plain - 1.0), 2),
            "hide_real_over_plain_pct": round(100.0 * (med["hide_real"] / plain - 1.0), 2),
            "hide_none_same_words": bool((planes["hide_none"] == planes["plain_a"]).all()),
            "hide_real_words_changed": int((planes["hide_real"] != planes["plain_a"]).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=20)
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

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    r = pwnfps_amd.Renderer(64, 48)
    r.level_load(level)
    r.set_objects(sph)
    r.set_blur_passes(0)
    _, _, spawn = r.get_level()

    def hides(n):
        return {"plain_a": None, "plain_b": None, "hide_none": torch.full((n,), -1, dtype=torch.int32, device=dev),
                "hide_real": (torch.arange(n, dtype=torch.int32, device=dev) % len(sph)).contiguous()}

    for repeat in range(args.repeats):
        for name, (W, H, rects) in (("grid64", GRID64), ("L1", L1)):
            n = len(rects)
            cams, secs = cameras(spawn, n, args.seed + n)
            with torch.cuda.stream(stream):
                t_cams = torch.from_numpy(cams.reshape(n, 16).copy()).to(dev)
                t_secs = torch.from_numpy(secs.copy()).to(dev)
                t_a = torch.zeros((H, W), dtype=torch.int32, device=dev)
                t_z = torch.zeros((H, W), dtype=torch.float32, device=dev)
                hd = hides(n)
            stream.synchronize()
            lay = r.viewports_layout(W, H, rects)
            rec = measure(torch, stream, lambda k: r.trace_viewports_device(lay, t_cams, t_secs, t_a, t_z, stream=stream, hide=hd[k]),
                          lambda: t_a.cpu().numpy(), args.reps, args.warmup)
            say(dict({"case": name + " colour", "repeat": repeat, "W": W, "H": H, "views": n, "spheres": int(len(sph))}, **rec))
            rec = measure(torch, stream, lambda k: r.trace_viewport_hits_device(lay, t_cams, t_a, stream=stream, hide=hd[k]),
                          lambda: t_a.cpu().numpy(), args.reps, args.warmup)
            say(dict({"case": name + " hits", "repeat": repeat, "W": W, "H": H, "views": n, "spheres": int(len(sph))}, **rec))
            lay.free()
        # the colour rays: the pixel rays of the grid's cameras
        cams, _ = cameras(spawn, 64, args.seed + 64)
        made = [pwnfps_amd.pixel_rays(64, 48, cam) for cam in cams]
        rays = np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 8) for m in made])
        seeds = np.concatenate([np.asarray(m[1], np.uint32) for m in made])
        n = len(rays)
        with torch.cuda.stream(stream):
            t_rays = torch.from_numpy(rays).to(dev)
            t_seeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
            t_col = torch.zeros((n,), dtype=torch.int32, device=dev)
            t_z = torch.zeros((n,), dtype=torch.float32, device=dev)
            hd = hides(n)
        stream.synchronize()
        rec = measure(torch, stream, lambda k: r.trace_rays_device(t_rays, t_col, t_z, seeds=t_seeds, sec_current=1.25, stream=stream, hide=hd[k]),
                      lambda: t_col.cpu().numpy(), args.reps, args.warmup)
        say(dict({"case": "rays colour", "repeat": repeat, "rays": n, "spheres": int(len(sph))}, **rec))
    r.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
