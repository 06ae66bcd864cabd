#!/usr/bin/env python3
"""A/B of how the trace kernel's walk loop ends (trace_kernel.hip: the step limit carried in ev): per scene the trace launch by
itself (frames on ONE compute stream, HIP events around every launch) and the frame on two streams.  One process per build -- the
library is chosen by PWNHIP_LIB -- run alternately for the parent commit's library and this tree's.  -> profiles/walk_exit/ab.txt
    PWNHIP_LIB=path python3 tools/walk_exit_ab.py LABEL [ROUNDS [8k]]        (8k: level.txt at 7680 x 4320 as well)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pwnfps_amd
GOLD = os.path.join(ROOT, "tests", "golden")
label = sys.argv[1] if len(sys.argv) > 1 else "build"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2


def measure(level, w, h, hasw):
    # (the 4-lane variants of the kernels: read when a context is created)
    if hasw:
        os.environ["PWN_DBG_FORCE_HASW"] = "1"
    else:
        os.environ.pop("PWN_DBG_FORCE_HASW", None)
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


CASES = [("pwnfps_level", 3840, 2160, False), ("pwnfps_level", 3840, 2160, True), ("pwnfps_level", 1280, 720, False),
         ("synth64", 1920, 1080, False), ("synth256", 3840, 2160, False)]
if "8k" in sys.argv[3:]:
    CASES.append(("pwnfps_level", 7680, 4320, False))
for level, w, h, hasw in CASES:
    for rep in range(rounds):
        o = measure(level, w, h, hasw)
        print("%-8s %-13s %4dx%-4d %s: trace launch alone %.4f ms (frame on one stream %.4f ms); frame on two streams %.4f ms" % (
            label, level, w, h, "4-lane" if hasw else "3-lane", o["one"][1], o["one"][0], o["two"][0]), flush=True)
