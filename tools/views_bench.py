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

--device-form measures pwn_trace_views_device beside pwn_trace_views instead, in the same run, on one context each; one JSON line
per case (both forms render colour and depth):
  host_wall_ms        host clock around one pwn_trace_views call, which returns with the planes in (pageable) host memory
  host_dev_ms         trace_ms + blur_ms of that call (its own HIP events around the kernels); host_total_ms with the copies
  device_wall_ms      host clock around one Renderer.trace_views_device call on torch tensors and ONE stream synchronise
  device_event_ms     HIP events on the stream around that call
  wall_over_host_dev  device_wall_ms / host_dev_ms: the two run the same trace and blur kernels
  same_pixels         the device form's colour and depth planes equal the host form's (checked on the first rep)
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


def device_form(args, out):
    import torch
    import pwnfps_amd
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    med = lambda v: float(np.median(v))       # noqa: E731
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rh = pwnfps_amd.Renderer(w, h)         # the host form
        rd = pwnfps_amd.Renderer(w, h)         # the device form
        for r in (rh, rd):
            r.level_load(level)
            r.set_objects(sph)
            r.set_blur_passes(args.blur)
        _, _, spawn = rh.get_level()
        for n in (int(v) for v in args.views.split(",")):
            cams, secs = cameras(spawn, n, args.seed + n)
            with torch.cuda.stream(stream):
                t_cams = torch.from_numpy(cams.reshape(n, 16)).to(dev)
                t_secs = torch.from_numpy(secs).to(dev)
                t_sb = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
                t_z = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
                t_work = torch.zeros((n, h, w), dtype=torch.int32, device=dev) if args.blur > 0 else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            hw, hd, ht, dw, de = [], [], [], [], []
            same = True
            for rep in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                sb, zb = rh.trace_views(cams, secs)
                t1 = time.perf_counter()
                st = rh.stats()
                t2 = time.perf_counter()
                e0.record(stream)
                rd.trace_views_device(t_cams, t_secs, t_sb, t_z, work=t_work, stream=stream)
                e1.record(stream)
                stream.synchronize()
                t3 = time.perf_counter()
                if rep == 0:
                    same = bool((t_sb.cpu().numpy().view(np.uint32) == sb).all()) and \
                        bool((t_z.cpu().numpy().view(np.uint32) == zb.view(np.uint32)).all())
                if rep >= args.warmup:
                    hw.append((t1 - t0) * 1e3); hd.append(st["trace_ms"] + st["blur_ms"]); ht.append(st["total_ms"])
                    dw.append((t3 - t2) * 1e3); de.append(e0.elapsed_time(e1))
            px = n * w * h
            rec = {"w": w, "h": h, "views": n, "blur": args.blur, "reps": args.reps,
                   "host_wall_ms": round(med(hw), 4), "host_dev_ms": round(med(hd), 4), "host_total_ms": round(med(ht), 4),
                   "device_wall_ms": round(med(dw), 4), "device_event_ms": round(med(de), 4),
                   "host_wall_mpix_s": round(px / med(hw) / 1e3, 1), "host_dev_mpix_s": round(px / med(hd) / 1e3, 1),
                   "device_wall_mpix_s": round(px / med(dw) / 1e3, 1), "device_event_mpix_s": round(px / med(de) / 1e3, 1),
                   "wall_over_host_dev": round(med(dw) / med(hd), 3), "same_pixels": same}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()
        rh.close()
        rd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="320x200,320x240")
    ap.add_argument("--views", default="1,4,16,64,256")
    ap.add_argument("--blur", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-form", action="store_true", help="pwn_trace_views_device beside pwn_trace_views")
    args = ap.parse_args()
    import pwnfps_amd
    if args.device_form:
        out = open(args.out, "w") if args.out else None
        device_form(args, out)
        if out:
            out.close()
        return
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
