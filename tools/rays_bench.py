"""pwn_trace_rays on the level.txt scene (the golden spheres): what caller-supplied rays cost against the frame kernel.

One JSON line per case:
  frame4k_units     (a) every pixel ray of the 3840x2160 spawn frame (pwn_pixel_rays) in the frame kernel's unit order, through
                    pwn_trace_rays_device; next to the frame kernel of the same camera (pwn_trace_rows_device, all rows).  Device
                    time by HIP events around the launch on one stream, median of --reps after --warmup.
  frame4k_rows      (b) the same rays in row order.
  host_small        (c) host clock around pwn_trace_rays at n = 1, 64 and 4096 (the first rays of the 320x240 spawn frame), median
                    of --reps after --warmup, next to a 320x240 pwn_trace_screen_centred on the same context (blur on).
  panorama          (d) a 4096x2048 equirectangular panorama from the spawn (rays made in torch on the GPU), device form: rays per
                    second of device time.
  same_pixels       (a, b) the rays' colour and depth equal the frame kernel's at every pixel.

    python tools/rays_bench.py [--reps 20] [--warmup 3] [--out file.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import pwnfps_amd
    level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    out = open(args.out, "w") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def dev_ms(fn):
        ts = []
        for i in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            b.synchronize()
            if i >= args.warmup:
                ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    # (a), (b): 4K
    w, h = 3840, 2160
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level)
    r.set_objects(sph)
    _, _, spawn = r.get_level()
    cam = pwnfps_amd.spawn_camera(spawn)
    sb = torch.zeros((h, w), dtype=torch.int32, device=dev)
    zb = torch.zeros((h, w), dtype=torch.float32, device=dev)
    frame_ms = dev_ms(lambda: r.trace_rows_device(cam, 0.0, 0, h, sb.data_ptr(), zb.data_ptr(), stream.cuda_stream))
    for order in ("units", "rows"):
        rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, cam, order=order)
        t_rays = torch.from_numpy(rays).to(dev)
        t_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        t_col = torch.zeros(len(rays), dtype=torch.int32, device=dev)
        t_z = torch.zeros(len(rays), dtype=torch.float32, device=dev)
        ms = dev_ms(lambda: r.trace_rays_device(t_rays, t_col, t_z, seeds=t_seeds, stream=stream))
        torch.cuda.synchronize()
        idx = torch.from_numpy((xy[:, 1].astype(np.int64) * w + xy[:, 0])).to(dev)
        same = bool((sb.view(-1)[idx] == t_col).all().item()) and bool((zb.view(-1)[idx].view(torch.int32) == t_z.view(torch.int32)).all().item())
        emit({"case": "frame4k_" + order, "w": w, "h": h, "rays": len(rays), "rays_dev_ms": round(ms, 4),
              "frame_dev_ms": round(frame_ms, 4), "ratio": round(ms / frame_ms, 3), "same_pixels": same})
        del t_rays, t_seeds, t_col, t_z
    # (d): a 4096 x 2048 equirectangular panorama from the spawn, rays made on the GPU
    pw, ph = 4096, 2048
    lon = (torch.arange(pw, device=dev, dtype=torch.float32) + 0.5) / pw * (2 * np.pi) - np.pi
    lat = np.pi / 2 - (torch.arange(ph, device=dev, dtype=torch.float32) + 0.5) / ph * np.pi
    la, lo = torch.meshgrid(lat, lon, indexing="ij")
    pr = torch.zeros((ph * pw, 8), dtype=torch.float32, device=dev)
    pr[:, 0], pr[:, 1], pr[:, 2], pr[:, 3] = float(cam[3, 0]), float(cam[3, 1]), float(cam[3, 2]), 1.0
    pr[:, 4] = (torch.cos(la) * torch.sin(lo)).reshape(-1)
    pr[:, 5] = torch.sin(la).reshape(-1)
    pr[:, 6] = (torch.cos(la) * torch.cos(lo)).reshape(-1)
    p_col = torch.zeros(ph * pw, dtype=torch.int32, device=dev)
    p_z = torch.zeros(ph * pw, dtype=torch.float32, device=dev)
    ms = dev_ms(lambda: r.trace_rays_device(pr, p_col, p_z, stream=stream))
    emit({"case": "panorama", "w": pw, "h": ph, "rays": pw * ph, "rays_dev_ms": round(ms, 4),
          "grays_per_s": round(pw * ph / ms / 1e6, 3)})
    r.close()
    # (c): small host calls next to a 320x240 blocking frame
    w, h = 320, 240
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level)
    r.set_objects(sph)
    rays, seeds, _ = pwnfps_amd.pixel_rays(w, h, cam, order="units")

    def wall_ms(fn):
        ts = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    block = wall_ms(lambda: r.trace_screen_centred(cam, 0.0))
    for n in (1, 64, 4096):
        ms = wall_ms(lambda: r.trace_rays(rays[:n], seeds[:n], 0.0))
        emit({"case": "host_small", "rays": n, "host_wall_ms": round(ms, 4), "blocking_320x240_wall_ms": round(block, 4),
              "ratio": round(ms / block, 3)})
    r.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
