#!/usr/bin/env python3
"""What pwn_pixel_rays_device costs (profiles/pixel_rays/bench.txt), and beside it the host route it replaces on the same inputs: the
cameras copied down, pwn_pixel_rays per camera on one CPU thread, the ray records copied up.

Crosshair: one shared pixel (w/2, h/2) of a 160x120 frame for n = 4096, 65536 and 2^20 cameras.  Whole frame: 64 cameras x 160x120
(d_xy NULL).  Seeds are written in every case.

Device: the time between two HIP events around ONE call (its two launches), median of 20 after 5 warm-ups, and around a run of 20
calls, divided by 20 -- at the small sizes the first is the launches themselves, the second what a stream that is kept busy pays.
The result is compared with the host's bit for bit before a time is printed.
Bytes: what the two launches have to move to and from device memory, from the shapes: per camera 64 B read and 80 B written by the
set-up, the pixel pairs given, per ray 32 B of record and 4 B of seed.  (The 80 B a ray reads of its camera's record are not
counted: the set-up has just written them, and the rays of a wave share them where they share the camera.)
Host: a wall clock around each leg, every leg ending in a synchronise where it is a copy; median of 5 (2^20 cameras: of 2).  The
loop calls pwn_pixel_rays through ctypes; "call overhead" is the same loop with n = 0, the part that is the binding's, not the
arithmetic's.

    python tools/pixel_rays_bench.py [--commit TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 160, 120
HBM_MEASURED_TBS = 6.29          # MI355X: float4 copy, 79 % of the 8.0 TB/s of the specification
CASES = (("crosshair", 4096, 1), ("crosshair", 65536, 1), ("crosshair", 1 << 20, 1), ("frame", 64, W * H))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("pixel_rays_bench: no GPU; nothing is measured without one")
    import pwnfps_amd
    from pwnfps_amd._lib import lib
    dev = torch.device("cuda", 0)
    lines = ["# tools/pixel_rays_bench.py: pwn_pixel_rays_device, %dx%d frame, seeds written" % (W, H),
             "# commit: %s" % a.commit, "# command: python tools/pixel_rays_bench.py --out profiles/pixel_rays/bench.txt",
             "# device: %s; torch %s; host CPU thread: 1" % (torch.cuda.get_device_name(0), torch.__version__),
             "# one_us: HIP events around one call, median of 20 after 5 warm-ups; run_us: around 20 calls, / 20; GB/s: the bytes both launches",
             "#         move (MB) over run_us -- HBM measures %.2f TB/s on this part (float4 copy)" % HBM_MEASURED_TBS,
             "# host route: d2h_ms n x 64 B of cameras down; loop_ms pwn_pixel_rays per camera through ctypes (overhead_ms: the same loop with no",
             "#         pixels); h2d_ms the records and seeds up; host/device = (d2h + loop + h2d) / run_us",
             "%-9s %8s %6s %8s %9s %9s %8s %8s %9s %12s %8s %12s" % ("case", "n", "m", "MB", "one_us", "run_us", "GB/s", "d2h_ms", "loop_ms", "overhead_ms",
                                                                   "h2d_ms", "host/device")]
    r = pwnfps_amd.Renderer(W, H)

    for case, n, m in CASES:
        T = n * m
        rng = np.random.default_rng(n)
        cams = np.stack([pwnfps_amd.spawn_camera((9, 4), ang_y=float(v)).reshape(16) for v in rng.uniform(0, 6.28, min(n, 4096))]).astype(np.float32)
        cams = np.ascontiguousarray(np.tile(cams, ((n + len(cams) - 1) // len(cams), 1))[:n])
        cams[:, 12] += rng.uniform(0, 20, n).astype(np.float32)
        cross = np.array([[W // 2, H // 2]], np.int32)
        t_cams = torch.from_numpy(cams).to(dev)
        t_xy = torch.from_numpy(cross).to(dev) if case == "crosshair" else None
        t_rays = torch.empty((T, 8), dtype=torch.float32, device=dev)
        t_seeds = torch.empty(T, dtype=torch.int32, device=dev)
        t_work = torch.empty((n, 20), dtype=torch.float32, device=dev)
        mb = (n * (64 + 80) + T * (32 + 4) + (8 * m if t_xy is not None else 0)) / 1e6

        # the host route, leg by leg
        h_cams = torch.empty((n, 16), dtype=torch.float32).pin_memory()
        h_rays = torch.empty((T, 8), dtype=torch.float32).pin_memory()
        h_seeds = torch.empty(T, dtype=torch.int32).pin_memory()
        xy = cross if case == "crosshair" else pwnfps_amd.pixel_rays(W, H, cams[0])[2]
        fn = lib.pwn_pixel_rays
        p_cam, p_ray, p_seed, p_xy = h_cams.data_ptr(), h_rays.data_ptr(), h_seeds.data_ptr(), xy.ctypes.data
        reps = 2 if n >= (1 << 20) else 5
        d2h, loop, over, h2d = [], [], [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            h_cams.copy_(t_cams, non_blocking=True)
            torch.cuda.synchronize()
            d2h.append((time.perf_counter() - c0) * 1e3)
            c0 = time.perf_counter()
            for i in range(n):
                fn(W, H, p_cam + 64 * i, m, p_xy, p_ray + 32 * m * i, p_seed + 4 * m * i)
            loop.append((time.perf_counter() - c0) * 1e3)
            c0 = time.perf_counter()
            for i in range(n):
                fn(W, H, p_cam + 64 * i, 0, p_xy, p_ray + 32 * m * i, p_seed + 4 * m * i)
            over.append((time.perf_counter() - c0) * 1e3)
            c0 = time.perf_counter()
            t_rays.copy_(h_rays, non_blocking=True)
            t_seeds.copy_(h_seeds, non_blocking=True)
            torch.cuda.synchronize()
            h2d.append((time.perf_counter() - c0) * 1e3)
        want_r, want_s = h_rays.numpy().view(np.uint32).copy(), h_seeds.numpy().view(np.uint32).copy()

        one, run = [], []
        for it in range(25):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            r.pixel_rays_device(t_cams, t_xy, rays=t_rays, seeds=t_seeds, work=t_work)
            e[1].record()
            e[2].record()
            for _ in range(20):
                r.pixel_rays_device(t_cams, t_xy, rays=t_rays, seeds=t_seeds, work=t_work)
            e[3].record()
            e[3].synchronize()
            if it == 0:          # (a timing of a wrong answer is no timing)
                assert (t_rays.cpu().numpy().view(np.uint32) == want_r).all() and (t_seeds.cpu().numpy().view(np.uint32) == want_s).all(), (case, n)
            if it >= 5:
                one.append(e[0].elapsed_time(e[1]) * 1e3)
                run.append(e[2].elapsed_time(e[3]) * 1e3 / 20)
        med = statistics.median
        host_ms = med(d2h) + med(loop) + med(h2d)
        lines.append("%-9s %8d %6d %8.2f %9.1f %9.1f %8.1f %8.3f %9.3f %12.3f %8.3f %12.1f" % (
            case, n, m, mb, med(one), med(run), mb * 1e3 / med(run), med(d2h), med(loop), med(over), med(h2d), host_ms * 1e3 / med(run)))
        print(lines[-1], flush=True)
    r.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
