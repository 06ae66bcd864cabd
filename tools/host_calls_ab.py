#!/usr/bin/env python3
"""Host-side cost of the blocking entry points, for an A/B of two builds of the library (chosen by PWNHIP_LIB, one process per
build, run alternately): the 4K blocking call (pwn_trace_screen_centred into registered buffers) and a batch of 8 views of
1280 x 720 (pwn_trace_views), each as the median host clock around one call and, beside it, the call's own device time, so that
what is left is the host's share.  One line per workload.  -> profiles/host_calls/ab.txt
    PWNHIP_LIB=path python3 tools/host_calls_ab.py LABEL [CALLS]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pwnfps_amd
from tools.views_bench import cameras
GOLD = os.path.join(ROOT, "tests", "golden")
label = sys.argv[1] if len(sys.argv) > 1 else "build"
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
level = os.path.join(GOLD, "levels", "pwnfps_level.txt")
sph = np.load(os.path.join(GOLD, "spheres_t0.npy"))


def timed(fn, stats, n):
    wall, dev = [], []
    for i in range(n + n // 4):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= n // 4:
            wall.append((t1 - t0) * 1e3)
            dev.append(stats()["total_ms"])
    return float(np.median(wall)), float(np.median(dev))


r = pwnfps_amd.Renderer(3840, 2160)
r.level_load(level)
r.set_objects(sph)
_, _, spawn = r.get_level()
cam = pwnfps_amd.spawn_camera(spawn)
sb, zb = np.empty((2160, 3840), np.uint32), np.empty((2160, 3840), np.float32)
r.host_register(sb)
r.host_register(zb)
w, d = timed(lambda: r.trace_screen_centred(cam, 0.0, sbuf=sb, zbuf=zb), r.stats, calls)
print("%-8s 4K blocking call, registered buffers: %.4f ms per call by the host clock, %.4f ms by the call's events, strips %d" % (
    label, w, d, r.call_strips_state()["strips_last"]), flush=True)
r.host_unregister(sb)
r.host_unregister(zb)
r.close()

r = pwnfps_amd.Renderer(1280, 720)
r.level_load(level)
r.set_objects(sph)
cams, secs = cameras(spawn, 8, 9)
w, d = timed(lambda: r.trace_views(cams, secs), r.stats, calls)
print("%-8s 8 views of 1280x720 (pwn_trace_views):  %.4f ms per call by the host clock, %.4f ms by the call's events" % (label, w, d), flush=True)
r.close()
