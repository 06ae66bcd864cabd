"""Views of their own sizes in one frame (pwn_trace_viewports) against the same pixels from per-size contexts, on the level.txt scene.

Layouts (--layouts):
  grid16, grid64  16 / 64 rectangles of 320x240 tiling one frame; also against pwn_trace_views with the same n on a 320x240 context
  split           two 3840x1080 halves of a 3840x2160 frame; also against one 3840x2160 blocking frame
  mixed           one 2880x2160 view beside a column of eight 960x270 previews in a 3840x2160 frame
Every figure is the median of --reps calls, and every layout is measured --repeats times (one JSON line each):
  vp_wall_ms, vp_trace_ms, vp_blur_ms, vp_dev_ms     one pwn_trace_viewports call: host clock, pwn_get_stats' timings, their sum
  single_wall_ms, single_dev_ms                      the n blocking pwn_trace_screen_centred calls on contexts of the views' sizes
  views_wall_ms, views_dev_ms                        (grids) one pwn_trace_views call of n views on a 320x240 context
  frame_wall_ms, frame_dev_ms                        (split) one blocking frame of the whole context
  same_pixels                                        every rectangle equals its per-size context's frame (checked on the first call)
Colour only (no depth plane to the host); the frame buffers are registered with the device (pwn_host_register) unless --no-register.

    python tools/viewports_bench.py [--reps 20] [--repeats 3] [--layouts grid16,grid64,split,mixed] [--out profiles/viewports/bench.jsonl]

--device-form measures pwn_trace_viewports_device instead (stream time between two events around the call, trace and blur; the two
sides of each comparison alternate call by call in one run, medians of --reps, --repeats lines each) and writes text:
  atlas   64 views of 160x120 into a 1280x960 atlas on a 3840x2160 context, against the same pixels through pwn_trace_views_device
          on a 160x120 context -- what the library could do before this call existed
  host    layout L1 of tests/test_gpu_viewports.py (eight views that tile 336x208) on a 3840x2160 context: the device form's stream
          time against the host form pwn_trace_viewports' total_ms on a 336x208 context (which includes its copy to the host)

    python tools/viewports_bench.py --device-form [--out profiles/viewports/device_form.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def layout(name):
    if name.startswith("grid"):
        n = int(name[4:])
        k = int(round(n ** 0.5))
        assert k * k == n, name
        return 320 * k, 240 * k, [(320 * (i % k), 240 * (i // k), 320, 240) for i in range(n)]
    if name == "split":
        return 3840, 2160, [(0, 0, 3840, 1080), (0, 1080, 3840, 1080)]
    if name == "mixed":
        return 3840, 2160, [(0, 0, 2880, 2160)] + [(2880, 270 * i, 960, 270) for i in range(8)]
    raise SystemExit("unknown layout " + name)


def cameras(spawn, n, seed):
    import pwnfps_amd
    rng = np.random.default_rng(seed)
    cams = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        cam = pwnfps_amd.spawn_camera(spawn, ang_y=float(rng.uniform(0, 6.28)), ang_x=float(rng.uniform(-0.4, 0.4)))
        cam[3, 0] += np.float32(rng.uniform(-0.35, 0.35))
        cam[3, 2] += np.float32(rng.uniform(-0.35, 0.35))
        cams[i] = cam
    return cams, np.zeros(n, np.float32)


def device_form(args):
    import torch
    import pwnfps_amd
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    dev = torch.device("cuda", 0)
    out = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    def renderer(w, h):
        r = pwnfps_amd.Renderer(w, h)
        r.level_load(level)
        r.set_objects(sph)
        r.set_blur_passes(args.blur)
        return r

    def timed(fn, stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    med = lambda v: float(np.median(v))       # noqa: E731
    say("# tools/viewports_bench.py --device-form: blur %d, medians of %d calls, the two sides alternating call by call, %d repeats" % (args.blur, args.reps, args.repeats))
    big = renderer(3840, 2160)
    _, _, spawn = big.get_level()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        # (a) the atlas against the parent's route
        n, vw, vh = 64, 160, 120
        W, H = 8 * vw, 8 * vh
        rects = [(vw * (i % 8), vh * (i // 8), vw, vh) for i in range(n)]
        cams, secs = cameras(spawn, n, args.seed + n)
        t_cams = torch.from_numpy(cams.reshape(n, 16).copy()).to(dev)
        t_secs = torch.from_numpy(secs.copy()).to(dev)
        lay = big.viewports_layout(W, H, rects)
        a_sb, a_work = (torch.zeros((H, W), dtype=torch.int32, device=dev) for _ in range(2))
        a_z = torch.zeros((H, W), dtype=torch.float32, device=dev)
        small = renderer(vw, vh)
        v_sb, v_work = (torch.zeros((n, vh, vw), dtype=torch.int32, device=dev) for _ in range(2))
        v_z = torch.zeros((n, vh, vw), dtype=torch.float32, device=dev)
        f_atlas = lambda: big.trace_viewports_device(lay, t_cams, t_secs, a_sb, a_z, work=a_work)      # noqa: E731
        f_views = lambda: small.trace_views_device(t_cams, t_secs, v_sb, v_z, work=v_work)             # noqa: E731
        f_atlas(); f_views()
        stream.synchronize()
        same = all(bool((a_sb[y:y + h, x:x + w] == v_sb[i]).all()) for i, (x, y, w, h) in enumerate(rects))
        say("(a) atlas: %d views of %d x %d into %d x %d on a 3840 x 2160 context (new) / pwn_trace_views_device on a %d x %d context (parent's route); same pixels: %s"
            % (n, vw, vh, W, H, vw, vh, same))
        for rep_no in range(args.repeats):
            ta, tv = [], []
            for rep in range(args.warmup + args.reps):
                x, y = timed(f_atlas, stream), timed(f_views, stream)
                if rep >= args.warmup:
                    ta.append(x); tv.append(y)
            say("    repeat %d: atlas %.4f ms (min %.4f max %.4f)   views %.4f ms (min %.4f max %.4f)   atlas / views %.3f"
                % (rep_no, med(ta), min(ta), max(ta), med(tv), min(tv), max(tv), med(ta) / med(tv)))
        lay.free()
        small.close()
        # (b) the device form against the host form
        # (layout L1 of tests/test_gpu_viewports.py: eight views that tile 336 x 208, from 4 x 4 pixels to 196 x 108)
        W, H, rects = 336, 208, [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
                                 (100, 138, 36, 70), (140, 100, 196, 108)]
        n = len(rects)
        cams, secs = cameras(spawn, n, args.seed + n)
        t_cams = torch.from_numpy(cams.reshape(n, 16).copy()).to(dev)
        t_secs = torch.from_numpy(secs.copy()).to(dev)
        lay = big.viewports_layout(W, H, rects)
        d_sb, d_work = (torch.zeros((H, W), dtype=torch.int32, device=dev) for _ in range(2))
        d_z = torch.zeros((H, W), dtype=torch.float32, device=dev)
        host = renderer(W, H)
        frame = np.empty((H, W), np.uint32)
        host.host_register(frame)
        f_dev = lambda: big.trace_viewports_device(lay, t_cams, t_secs, d_sb, d_z, work=d_work)        # noqa: E731
        f_dev()
        host.trace_viewports(rects, cams, secs, want_z=False, sbuf=frame)
        stream.synchronize()
        same = bool((d_sb.cpu().numpy().view(np.uint32) == frame).all())
        say("(b) L1: %d views of their own sizes into %d x %d: the device form on a 3840 x 2160 context (stream time) / pwn_trace_viewports on a %d x %d context (its trace + blur, its total_ms with the copy to the host); same pixels: %s"
            % (n, W, H, W, H, same))
        for rep_no in range(args.repeats):
            td, tk, tt = [], [], []
            for rep in range(args.warmup + args.reps):
                x = timed(f_dev, stream)
                host.trace_viewports(rects, cams, secs, want_z=False, sbuf=frame)
                st = host.stats()
                if rep >= args.warmup:
                    td.append(x); tk.append(st["trace_ms"] + st["blur_ms"]); tt.append(st["total_ms"])
            say("    repeat %d: device form %.4f ms (min %.4f max %.4f)   host form kernels %.4f ms, total %.4f ms (min %.4f max %.4f)   device / host total %.3f, device / host kernels %.3f"
                % (rep_no, med(td), min(td), max(td), med(tk), med(tt), min(tt), max(tt), med(td) / med(tt), med(td) / med(tk)))
        lay.free()
        host.close()
    big.close()
    out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", default="grid16,grid64,split,mixed")
    ap.add_argument("--blur", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-register", action="store_true")
    ap.add_argument("--device-form", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "viewports", "device_form.txt" if args.device_form else "bench.jsonl")
    if args.device_form:
        return device_form(args)
    import pwnfps_amd
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    med = lambda v: round(float(np.median(v)), 4)       # noqa: E731

    def renderer(w, h):
        r = pwnfps_amd.Renderer(w, h)
        r.level_load(level)
        r.set_objects(sph)
        r.set_blur_passes(args.blur)
        return r

    for name in args.layouts.split(","):
        W, H, rects = layout(name)
        n = len(rects)
        rv = renderer(W, H)
        _, _, spawn = rv.get_level()
        cams, secs = cameras(spawn, n, args.seed + n)
        frame = np.empty((H, W), np.uint32)
        sizes = sorted({(w, h) for _, _, w, h in rects})
        singles = {s: renderer(*s) for s in sizes}
        bufs = {s: np.empty((s[1], s[0]), np.uint32) for s in sizes}
        rbatch = renderer(320, 240) if name.startswith("grid") else None
        if not args.no_register:
            rv.host_register(frame)
            for s in sizes:
                singles[s].host_register(bufs[s])
        same = True
        for rep_no in range(args.repeats):
            t = {k: [] for k in ("vp_wall", "vp_trace", "vp_blur", "single_wall", "single_dev", "views_wall", "views_dev", "frame_wall", "frame_dev")}
            for rep in range(args.warmup + args.reps):
                keep = rep >= args.warmup
                t0 = time.perf_counter()
                rv.trace_viewports(rects, cams, secs, want_z=False, sbuf=frame)
                t1 = time.perf_counter()
                st = rv.stats()
                first = rep_no == 0 and rep == 0
                dev = 0.0
                wall = 0.0
                for i, (x, y, w, h) in enumerate(rects):
                    r1, b1 = singles[(w, h)], bufs[(w, h)]
                    t2 = time.perf_counter()
                    r1.trace_screen_centred(cams[i], secs[i], want_z=False, sbuf=b1)
                    wall += time.perf_counter() - t2
                    s1 = r1.stats()
                    dev += s1["trace_ms"] + s1["blur_ms"]
                    if first:
                        same = same and bool((frame[y:y + h, x:x + w] == b1).all())
                if keep:
                    t["vp_wall"].append((t1 - t0) * 1e3); t["vp_trace"].append(st["trace_ms"]); t["vp_blur"].append(st["blur_ms"])
                    t["single_wall"].append(wall * 1e3); t["single_dev"].append(dev)
                if rbatch is not None:
                    t0 = time.perf_counter()
                    rbatch.trace_views(cams, secs, want_z=False)
                    t1 = time.perf_counter()
                    s1 = rbatch.stats()
                    if keep:
                        t["views_wall"].append((t1 - t0) * 1e3); t["views_dev"].append(s1["trace_ms"] + s1["blur_ms"])
                if name == "split":
                    t0 = time.perf_counter()
                    rv.trace_screen_centred(cams[0], secs[0], want_z=False, sbuf=frame)
                    t1 = time.perf_counter()
                    s1 = rv.stats()
                    if keep:
                        t["frame_wall"].append((t1 - t0) * 1e3); t["frame_dev"].append(s1["trace_ms"] + s1["blur_ms"])
            rec = {"layout": name, "W": W, "H": H, "views": n, "blur": args.blur, "reps": args.reps, "repeat": rep_no,
                   "registered": not args.no_register, "same_pixels": same}
            for k, v in t.items():
                if v:
                    rec[k + "_ms"] = med(v)
            rec["vp_dev_ms"] = round(rec["vp_trace_ms"] + rec["vp_blur_ms"], 4)
            rec["single_over_vp_dev"] = round(rec["single_dev_ms"] / rec["vp_dev_ms"], 3)
            if "views_dev_ms" in rec:
                rec["vp_over_views_dev"] = round(rec["vp_dev_ms"] / rec["views_dev_ms"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n"); out.flush()
        for r in [rv, rbatch] + list(singles.values()):
            if r is not None:
                r.close()
    out.close()


if __name__ == "__main__":
    main()
