"""pwn_trace_view_hits on the level.txt scene (the golden spheres): what the first-hit planes of views cost against the two calls
they stand between -- the same primary segments as first-hit records of uploaded rays, and the same views traced to the end.

One JSON line per case:
  predict           (no GPU; tools/hits_bench.py) what the oracle says a primary-segment kernel is spared on the 3840x2160 spawn
                    frame: its share of the walk steps and of the ray set-ups of all segments.
  frame4k           the 3840x2160 spawn frame as a one-view batch.
  views64           64 views of 320x240 from cameras turned about the spawn cell's centre.
Each of the two times, ALTERNATING in one run, by HIP events around each call on one stream, median of --reps after --warmup:
  a  view_hits      pwn_trace_view_hits_device (label, cell and dist planes: 12 B a pixel out);
  b  hits           pwn_trace_hits_device on the same views' pixel_rays(order="units"), already uploaded (32 B in, 48 B out);
  c  views          pwn_trace_views_device with PWN_OPT_BLUR_PASSES 0 (every segment, shading; 8 B a pixel out).
*_ms the medians, *_min_ms / *_max_ms and *_iqr_ms the run-to-run spread in the same run; same: the planes of (a) are (b)'s
records packed, pixel for pixel.

    python tools/view_hits_bench.py [--reps 20] [--warmup 3] [--out file.jsonl] [--predict-only | --no-predict]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hits_bench import GOLD, LEVEL, predict, spawn_cam  # noqa: E402


def turned(cam, yaw):
    """cam turned about y by yaw, in place of its rows x and z (the position stays)"""
    c, s = np.float32(math.cos(yaw)), np.float32(math.sin(yaw))
    out = cam.copy()
    out[0, :3] = (c, 0, -s)
    out[2, :3] = (s, 0, c)
    return out


def timed_case(name, w, h, cams, sph, reps, warmup):
    import torch
    import pwnfps_amd
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(LEVEL)
    r.set_objects(sph)
    r.set_blur_passes(0)
    n, plane = len(cams), w * h
    rays, xy = [], None
    for cam in cams:
        ry, _, xy = pwnfps_amd.pixel_rays(w, h, cam, order="units")
        rays.append(ry)
    rays = np.concatenate(rays)
    t_cams = torch.from_numpy(np.ascontiguousarray(cams.reshape(n, 16))).to(dev)
    t_secs = torch.zeros(n, dtype=torch.float32, device=dev)
    t_rays = torch.from_numpy(rays).to(dev)
    del rays
    t_hits = torch.zeros((n * plane, 12), dtype=torch.int32, device=dev)
    t_label, t_cell = (torch.zeros((n, h, w), dtype=torch.int32, device=dev) for _ in range(2))
    t_dist = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    t_sbuf = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    t_zbuf = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    fns = {"view_hits": lambda: r.trace_view_hits_device(t_cams, t_label, t_cell, t_dist, stream=stream),
           "hits": lambda: r.trace_hits_device(t_rays, t_hits, stream=stream),
           "views": lambda: r.trace_views_device(t_cams, t_secs, t_sbuf, t_zbuf, stream=stream)}
    ts = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            b.synchronize()
            if i >= warmup:
                ts[k].append(a.elapsed_time(b))
    torch.cuda.synchronize()
    # (a)'s planes against (b)'s records: ray j of view v is pixel xy[j] of that view
    t_xy = torch.from_numpy(xy.astype(np.int64)).to(dev)
    hits = t_hits.view(n, plane, 12)
    at = lambda t: t.view(torch.int32)[:, t_xy[:, 1], t_xy[:, 0]]
    packed = hits[..., 0] | ((hits[..., 1] + 1) << 2) | ((hits[..., 2] + 1) << 5) | (hits[..., 3] << 19)
    same = bool((at(t_label) == packed).all().item()) and bool((at(t_cell) == hits[..., 11]).all().item()) and \
        bool((at(t_dist) == hits[..., 4]).all().item())
    d = {"case": name, "w": w, "h": h, "views": n, "pixels": n * plane, "reps": reps}
    for k, v in ts.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, (25, 50, 75)))
        d.update({k + "_ms": round(med, 4), k + "_min_ms": round(min(v), 4), k + "_max_ms": round(max(v), 4), k + "_iqr_ms": round(q3 - q1, 4)})
    d["view_hits_over_hits"] = round(d["view_hits_ms"] / d["hits_ms"], 3)
    d["view_hits_over_views"] = round(d["view_hits_ms"] / d["views_ms"], 3)
    d["hit_kinds"] = [int(((t_label & 3) == k).sum().item()) for k in (0, 1, 2)]
    d["same"] = same
    r.close()
    return d


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

    if not args.no_predict:
        emit(predict(3840, 2160))
    if args.predict_only:
        return
    import oracle
    O = oracle.Oracle()
    O.load_level(LEVEL)
    _, _, spawn = O.get_level()
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))
    cam = spawn_cam(spawn)
    emit(timed_case("frame4k", 3840, 2160, cam[None], sph, args.reps, args.warmup))
    cams = np.stack([turned(cam, 2.0 * math.pi * i / 64) for i in range(64)])
    emit(timed_case("views64", 320, 240, cams, sph, args.reps, args.warmup))
    if out:
        out.close()


if __name__ == "__main__":
    main()
