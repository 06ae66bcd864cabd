#!/usr/bin/env python3
"""A/B of the bounding balls of long sphere lists (sphere_bound.h; PWN_SPHERE_BOUNDS=0 sends a launch none) in one process: per scene
the trace launch by itself (frames on ONE compute stream, HIP events around every launch) and the frame on two streams, with the
balls and without, alternating.  Run from a checkout of the parent commit, which does not read the variable, the two settings are
the same build twice: its spread.  -> profiles/sphere_bounds/ab.txt
    python3 tools/sphere_bounds_ab.py LABEL [ROUNDS]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pwnfps_amd
GOLD = os.path.join(ROOT, "tests", "golden")
label = sys.argv[1] if len(sys.argv) > 1 else "build"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2


def measure(level, w, h, bounds):
    os.environ["PWN_SPHERE_BOUNDS"] = "1" if bounds else "0"
    sph = np.load(os.path.join(GOLD, "spheres_t0.npy")) if level == "pwnfps_level" else np.load(os.path.join(GOLD, "levels", level + "_spheres.npy"))
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(os.path.join(GOLD, "levels", level + ".txt"))
    r.set_objects(sph)
    _, _, spawn = r.get_level()
    cam = pwnfps_amd.spawn_camera(spawn) if level == "pwnfps_level" else np.load(os.path.join(GOLD, "levels", level + "_cams.npy"))[0]
    out = {}
    for two in (False, True):
        r.set_frame_overlap(two)
        r.set_frame_timing(1 if not two else 0)
        r.frames_config(3, sbuf=False)
        ms = []
        for rep in range(3):
            t0 = time.perf_counter()
            n = 300
            for i in range(n):
                s = i % 3
                r.set_objects(sph)
                if i >= 3:
                    f = r.wait_frame(s)
                    if f["timed"] and rep:
                        ms.append(f["trace_ms"])
                r.submit_frame(cam, 0.0, s)
            for i in range(n - 3, n):
                r.wait_frame(i % 3)
            dt = (time.perf_counter() - t0) / n * 1e3
        out["two" if two else "one"] = (dt, float(np.median(ms)) if ms else 0.0)
        r.frames_config(0)
    r.close()
    return out


for level, w, h in (("pwnfps_level", 3840, 2160), ("pwnfps_level", 1280, 720), ("synth64", 1920, 1080), ("synth256", 3840, 2160)):
    for rep in range(rounds):
        for bounds in (True, False):
            o = measure(level, w, h, bounds)
            print("%-8s %-13s %4dx%-4d PWN_SPHERE_BOUNDS=%d: trace launch alone %.4f ms (frame on one stream %.4f ms); frame on two streams %.4f ms" % (
                label, level, w, h, 1 if bounds else 0, o["one"][1], o["one"][0], o["two"][0]), flush=True)
