"""Sphere tables in device memory (tables.h PWN_LF_GLOBAL): what the form costs where it is not needed, and what it buys.

Everything is generated from the seeds of tests/big_scenes.py.  Frames are 3840x2160 without blur; a time is the device time of
ONE trace launch over the whole frame (pwn_trace_rows_device) between two HIP events on one stream, median of --reps after --warmup.
One JSON line per case:
  price   t0 on level.txt, then synth64's own spheres on synth64: a context with the default form against a context created
          with PWN_SPHERE_LISTS=global, launches ALTERNATING in one run.  ratio = global / default.  same_frame: the two colour
          and depth planes are equal.
  buys    swarm_all (on synth64) and fat (on level.txt): launch time, Mpixels/s, the tables' form and sizes, and what their
          upload takes: upload_call_ms is the host's time inside the upload call (binning, packing, staging, enqueue),
          upload_done_ms the time from the call's start until the device has the tables (the call, then a wait for the
          upload stream on an otherwise idle device).

    python tools/big_bench.py [--reps 20] [--warmup 3] [--case price|buys|all] [--width 3840 --height 2160] [--out file.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def level_file(name):
    return os.path.join(GOLD, "levels", name + ".txt")


def spheres_of(key):
    return np.load(os.path.join(GOLD, "spheres_t0.npy" if key == "t0" else os.path.join("levels", key + "_spheres.npy")))


class Ctx:
    """a context, its planes on the device, and one timed launch of the whole frame"""

    def __init__(self, torch, w, h, level, spheres, env=None):
        import pwnfps_amd
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.r = pwnfps_amd.Renderer(w, h)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.torch, self.w, self.h = torch, w, h
        self.r.level_load(level_file(level))
        self.r.set_blur_passes(0)
        self.r.set_objects(spheres)
        dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(dev)
        self.col = torch.zeros((h, w), dtype=torch.int32, device=dev)
        self.z = torch.zeros((h, w), dtype=torch.float32, device=dev)

    def launch_ms(self, cam):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            a.record(self.stream)
            self.r.trace_rows_device(cam, 0.0, 0, self.h, self.col.data_ptr(), self.z.data_ptr(), self.stream.cuda_stream)
            b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b)

    def close(self):
        self.r.close()


def alternate(ctxs, cam, warmup, reps):
    ts = {k: [] for k in ctxs}
    for i in range(warmup + reps):
        for k, c in ctxs.items():
            t = c.launch_ms(cam)
            if i >= warmup:
                ts[k].append(t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=("price", "buys", "all"), default="all")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    import torch
    import oracle
    import big_scenes as BS
    w, h = args.width, args.height

    if args.case in ("price", "all"):
        for level, key in (("pwnfps_level", "t0"), ("synth64", "synth64")):
            sph = spheres_of(key)
            ctxs = {"default": Ctx(torch, w, h, level, sph), "global": Ctx(torch, w, h, level, sph, {"PWN_SPHERE_LISTS": "global"})}
            _, _, spawn = ctxs["default"].r.get_level()
            cam = BS.cameras(spawn, oracle)[0]
            ts = alternate(ctxs, cam, args.warmup, args.reps)
            torch.cuda.synchronize()
            same = bool((ctxs["default"].col == ctxs["global"].col).all().item()) and \
                bool((ctxs["default"].z.view(torch.int32) == ctxs["global"].z.view(torch.int32)).all().item())
            d, g = float(np.median(ts["default"])), float(np.median(ts["global"]))
            emit({"case": "price", "level": level, "spheres": key, "w": w, "h": h,
                  "default_form": ctxs["default"].r.sphere_tables()["form"], "global_form": ctxs["global"].r.sphere_tables()["form"],
                  "default_ms": round(d, 4), "global_ms": round(g, 4), "default_min_ms": round(min(ts["default"]), 4),
                  "global_min_ms": round(min(ts["global"]), 4), "ratio": round(g / d, 3), "same_frame": same,
                  "default_tables": ctxs["default"].r.sphere_tables(), "global_tables": ctxs["global"].r.sphere_tables()})
            for c in ctxs.values():
                c.close()

    if args.case in ("buys", "all"):
        for name in ("swarm_all", "fat"):
            sc = BS.scene(name, oracle)
            c = Ctx(torch, w, h, sc.level, sc.spheres)
            cam = BS.cameras(sc.spawn, oracle)[0]
            ts = alternate({"x": c}, cam, args.warmup, args.reps)["x"]
            ms = float(np.median(ts))
            up_call, up_done = [], []
            for i in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.r.set_objects(sc.spheres)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if i >= args.warmup:
                    up_call.append((t1 - t0) * 1e3)
                    up_done.append((t2 - t0) * 1e3)
            emit({"case": "buys", "scene": name, "level": sc.level, "spheres": len(sc.spheres), "w": w, "h": h,
                  "launch_ms": round(ms, 4), "launch_min_ms": round(min(ts), 4), "mpixels_per_s": round(w * h / ms / 1e3, 1),
                  "tables": c.r.sphere_tables(), "upload_call_ms": round(float(np.median(up_call)), 4),
                  "upload_done_ms": round(float(np.median(up_done)), 4)})
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
