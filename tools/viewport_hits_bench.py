"""First-hit planes of views of their own sizes (pwn_trace_viewport_hits_device) against its neighbours, on the level.txt scene.
Stream time between two HIP events around the call, medians of --reps calls, the two sides of a comparison alternating call by
call, one line per repeat; --append adds to --out, so that a job may run every repeat as a process with a time limit of its own.

  --part a   64 views of 160x120 into a 1280x960 label atlas on a 3840x2160 context, against the same planes through
             pwn_trace_view_hits_device on a 160x120 context
  --part b   layout L1 of tools/viewports_bench.py (eight views that tile 336x208) on a 3840x2160 context, against
             pwn_trace_viewports_device with blur 0 on the same layout: the primary segments' share of the colour call

    python tools/viewport_hits_bench.py --part a [--reps 20] [--repeats 3] [--append] [--out profiles/viewport_hits/bench.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewport_hits", "bench.txt"))
    args = ap.parse_args()
    import torch
    import pwnfps_amd
    from viewports_bench import cameras
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a" if args.append else "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    def renderer(w, h):
        r = pwnfps_amd.Renderer(w, h)
        r.level_load(level)
        r.set_objects(sph)
        r.set_blur_passes(0)
        return r

    def timed(fn, stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    med = lambda v: float(np.median(v))       # noqa: E731
    planes = lambda *shape: [torch.zeros(shape, dtype=torch.int32, device=dev) for _ in range(3)]      # noqa: E731
    big = renderer(3840, 2160)
    _, _, spawn = big.get_level()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        if args.part == "a":
            n, vw, vh = 64, 160, 120
            W, H = 8 * vw, 8 * vh
            rects = [(vw * (i % 8), vh * (i // 8), vw, vh) for i in range(n)]
            cams, _ = cameras(spawn, n, args.seed + n)
            t_cams = torch.from_numpy(cams.reshape(n, 16).copy()).to(dev)
            lay = big.viewports_layout(W, H, rects)
            a = planes(H, W)
            small = renderer(vw, vh)
            v = planes(n, vh, vw)
            f_new = lambda: big.trace_viewport_hits_device(lay, t_cams, a[0], a[1], a[2].view(torch.float32))      # noqa: E731
            f_old = lambda: small.trace_view_hits_device(t_cams, v[0], v[1], v[2].view(torch.float32))             # noqa: E731
            f_new(); f_old()
            stream.synchronize()
            same = all(bool((a[k][y:y + h, x:x + w] == v[k][i]).all()) for k in range(3) for i, (x, y, w, h) in enumerate(rects))
            head = ("(a) label atlas: %d views of %d x %d into %d x %d on a 3840 x 2160 context (viewport_hits) / pwn_trace_view_hits_device on a %d x %d "
                    "context (view_hits); same planes: %s" % (n, vw, vh, W, H, vw, vh, same))
            names = ("viewport_hits", "view_hits")
        else:
            W, H, rects = 336, 208, [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
                                     (100, 138, 36, 70), (140, 100, 196, 108)]
            n = len(rects)
            cams, secs = cameras(spawn, n, args.seed + n)
            t_cams = torch.from_numpy(cams.reshape(n, 16).copy()).to(dev)
            t_secs = torch.from_numpy(secs.copy()).to(dev)
            lay = big.viewports_layout(W, H, rects)
            a = planes(H, W)
            c_sb = torch.zeros((H, W), dtype=torch.int32, device=dev)
            c_z = torch.zeros((H, W), dtype=torch.float32, device=dev)
            f_new = lambda: big.trace_viewport_hits_device(lay, t_cams, a[0], a[1], a[2].view(torch.float32))      # noqa: E731
            f_old = lambda: big.trace_viewports_device(lay, t_cams, t_secs, c_sb, c_z)                             # noqa: E731
            f_new(); f_old()
            stream.synchronize()
            hit = a[0] != 0
            same = bool((a[2].view(torch.float32)[hit] == c_z[hit]).all())
            head = ("(b) L1: %d views of their own sizes into %d x %d on a 3840 x 2160 context: first-hit planes (viewport_hits) / colour and depth, blur 0 "
                    "(viewports); distance plane equals the depth plane where a ray ends on something: %s" % (n, W, H, same))
            names = ("viewport_hits", "viewports")
        if not args.append:
            say("# tools/viewport_hits_bench.py: stream time between HIP events, medians of %d calls after %d warm-up, the two sides alternating call by call" % (args.reps, args.warmup))
        say(head)
        for rep_no in range(args.repeats):
            tn, to = [], []
            for rep in range(args.warmup + args.reps):
                x, y = timed(f_new, stream), timed(f_old, stream)
                if rep >= args.warmup:
                    tn.append(x); to.append(y)
            say("    %s %.4f ms (min %.4f max %.4f)   %s %.4f ms (min %.4f max %.4f)   ratio %.3f"
                % (names[0], med(tn), min(tn), max(tn), names[1], med(to), min(to), max(to), med(tn) / med(to)))
        lay.free()
        if args.part == "a":
            small.close()
    big.close()
    out.close()


if __name__ == "__main__":
    main()
