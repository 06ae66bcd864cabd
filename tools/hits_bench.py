"""pwn_trace_hits on the level.txt scene (the golden spheres): what first-hit records cost against pwn_trace_rays on the same rays.

One JSON line per case:
  predict           (no GPU) what the oracle says the hit kernel is spared: the walk steps of the primary segments over the walk
                    steps of all segments of the 3840x2160 spawn frame (pwno_step_map), and the same for rays.
  frame4k_units     every pixel ray of the 3840x2160 spawn frame (pwn_pixel_rays) in the frame kernel's unit order through
                    pwn_trace_hits_device and through pwn_trace_rays_device, ALTERNATING in one run.  Device time by HIP events
                    around each launch on one stream, median of --reps after --warmup.  same_hits: kind == 0 exactly where the
                    ray kept its sentinel depth, dist the ray's depth bits elsewhere.
  host_small        host clock around pwn_trace_hits and pwn_trace_rays at n = 1, 64 and 4096 (the first rays of the 320x240
                    spawn frame), alternating, median of --reps after --warmup.

    python tools/hits_bench.py [--reps 20] [--warmup 3] [--out file.jsonl] [--predict-only | --no-predict]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
LEVEL = os.path.join(GOLD, "levels", "pwnfps_level.txt")


def spawn_cam(spawn):
    cam = np.eye(4, dtype=np.float32)
    cam[3, :3] = (spawn[0] + 0.5, 0.5, spawn[1] + 0.5)
    return cam


def predict(w, h):
    import oracle
    O = oracle.Oracle()
    O.load_level(LEVEL)
    O.set_spheres(np.load(os.path.join(GOLD, "spheres_t0.npy")))
    _, _, spawn = O.get_level()
    smap = np.zeros((h, w, 3), np.uint16)
    O.L.pwno_step_map.argtypes = [C.c_void_p]
    O.L.pwno_step_map(smap.ctypes.data)
    try:
        _, _, st = O.trace_rows(w, h, 0, h, spawn_cam(spawn))
    finally:
        O.L.pwno_step_map(None)
    steps = smap.reshape(-1, 3).astype(np.int64).sum(0)
    assert int(steps.sum()) == st.steps
    return {"case": "predict", "w": w, "h": h, "steps_by_segment": steps.tolist(), "rays_by_segment": (smap.reshape(-1, 3) > 0).sum(0).tolist(),
            "primary_steps_share": round(float(steps[0]) / float(steps.sum()), 4), "primary_rays_share": round(w * h / float(st.rays), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w, h = 3840, 2160
    if not args.no_predict:
        emit(predict(w, h))
    if args.predict_only:
        return
    import torch
    import pwnfps_amd
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(LEVEL)
    r.set_objects(sph)
    _, _, spawn = r.get_level()
    cam = spawn_cam(spawn)
    rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, cam, order="units")
    n = len(rays)
    t_rays = torch.from_numpy(rays).to(dev)
    t_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
    t_col = torch.zeros(n, dtype=torch.int32, device=dev)
    sentinel = 0x7fc12345
    t_z = torch.full((n,), sentinel, dtype=torch.int32, device=dev).view(torch.float32)
    t_hits = torch.zeros((n, 12), dtype=torch.int32, device=dev)
    fns = {"hits": lambda: r.trace_hits_device(t_rays, t_hits, stream=stream),
           "rays": lambda: r.trace_rays_device(t_rays, t_col, t_z, seeds=t_seeds, stream=stream)}
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
    torch.cuda.synchronize()
    kind, dist = t_hits[:, 0], t_hits[:, 4]
    zi = t_z.view(torch.int32)
    same = bool(((kind == 0) == (zi == sentinel)).all().item()) and bool(((dist == zi) | (kind == 0)).all().item())
    hm, rm = float(np.median(ts["hits"])), float(np.median(ts["rays"]))
    emit({"case": "frame4k_units", "w": w, "h": h, "rays": n, "hits_dev_ms": round(hm, 4), "rays_dev_ms": round(rm, 4),
          "hits_min_ms": round(min(ts["hits"]), 4), "rays_min_ms": round(min(ts["rays"]), 4), "ratio": round(hm / rm, 3),
          "hit_kinds": [int((kind == k).sum().item()) for k in (0, 1, 2)], "same_hits": same})
    del t_rays, t_seeds, t_col, t_z, t_hits
    r.close()
    # host form, small batches
    w, h = 320, 240
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(LEVEL)
    r.set_objects(sph)
    rays, seeds, _ = pwnfps_amd.pixel_rays(w, h, cam, order="units")
    for n in (1, 64, 4096):
        fns = {"hits": lambda: r.trace_hits(rays[:n]), "rays": lambda: r.trace_rays(rays[:n], seeds[:n], 0.0)}
        ts = {k: [] for k in fns}
        for i in range(args.warmup + args.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                if i >= args.warmup:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        hm, rm = float(np.median(ts["hits"])), float(np.median(ts["rays"]))
        emit({"case": "host_small", "rays": n, "hits_host_wall_ms": round(hm, 4), "rays_host_wall_ms": round(rm, 4), "ratio": round(hm / rm, 3)})
    r.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
