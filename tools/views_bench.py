"""A batch of views (pwn_trace_views) against the same pixels as blocking calls, on the level.txt scene.

For 320x200 (the reference's own frame, defs.h DEF_RWIDTH / DEF_RHEIGHT) and 320x240, n views in {1, 4, 16, 64, 256} of
seeded cameras around the spawn (position jittered inside the spawn room, turned and tilted), with the depth planes copied
to the host and without.  One JSON line per case:
  batch_wall_ms       host clock around one pwn_trace_views call (median of --reps)
  batch_dev_ms        trace_ms + blur_ms of that call (pwn_get_stats; median)
  single_wall_ms      host clock around the n blocking pwn_trace_screen_centred calls that render the same views (median)
  single_dev_ms       the sum of their trace_ms + blur_ms (median)
  *_mpix_s            n x w x h pixels over each of the four
  same_pixels         the batch's colour (and depth) planes equal the blocking calls' (checked on the first rep)

    python tools/views_bench.py [--reps 20] [--sizes 320x200,320x240] [--views 1,4,16,64,256] [--out file.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="320x200,320x240")
    ap.add_argument("--views", default="1,4,16,64,256")
    ap.add_argument("--blur", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pwnfps_amd
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    out = open(args.out, "w") if args.out else None
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rb = pwnfps_amd.Renderer(w, h)         # the batch
        rs = pwnfps_amd.Renderer(w, h)         # the blocking calls
        for r in (rb, rs):
            r.level_load(level)
            r.set_objects(sph)
            r.set_blur_passes(args.blur)
        _, _, spawn = rb.get_level()
        for n in (int(v) for v in args.views.split(",")):
            cams, secs = cameras(spawn, n, args.seed + n)
            for want_z in (True, False):
                sbuf = np.empty((n, h, w), np.uint32)
                zbuf = np.empty((n, h, w), np.float32)
                bw, bd, sw, sd = [], [], [], []
                same = True
                for rep in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    got = rb.trace_views(cams, secs, want_z=want_z)
                    t1 = time.perf_counter()
                    st = rb.stats()
                    dev_b = st["trace_ms"] + st["blur_ms"]
                    dev_s = 0.0
                    t2 = time.perf_counter()
                    for i in range(n):
                        rs.trace_screen_centred(cams[i], secs[i], want_z=want_z, sbuf=sbuf[i], zbuf=zbuf[i] if want_z else None)
                        s = rs.stats()
                        dev_s += s["trace_ms"] + s["blur_ms"]
                    t3 = time.perf_counter()
                    if rep == 0:
                        gs = got[0] if want_z else got
                        same = bool((gs == sbuf).all())
                        if want_z:
                            same = same and bool((got[1].view(np.uint32) == zbuf.view(np.uint32)).all())
                    if rep >= args.warmup:
                        bw.append((t1 - t0) * 1e3); bd.append(dev_b); sw.append((t3 - t2) * 1e3); sd.append(dev_s)
                px = n * w * h
                med = lambda v: float(np.median(v))       # noqa: E731
                rec = {"w": w, "h": h, "views": n, "zbuf": want_z, "blur": args.blur, "reps": args.reps,
                       "batch_wall_ms": round(med(bw), 4), "batch_dev_ms": round(med(bd), 4),
                       "single_wall_ms": round(med(sw), 4), "single_dev_ms": round(med(sd), 4),
                       "batch_wall_mpix_s": round(px / med(bw) / 1e3, 1), "batch_dev_mpix_s": round(px / med(bd) / 1e3, 1),
                       "single_wall_mpix_s": round(px / med(sw) / 1e3, 1), "single_dev_mpix_s": round(px / med(sd) / 1e3, 1),
                       "same_pixels": same}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n"); out.flush()
        rb.close()
        rs.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
