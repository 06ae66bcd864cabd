"""The host time Renderer's device forms spend in Python per call: pwnfps_amd/render.py against another render.py of the same
interface (the parent commit's), in one process and in alternation.

render.lib is replaced by a stand-in whose functions return 0, the renderer is a bare object without a context, so no call reaches
the library and no kernel runs; the tensors are real GPU tensors, as the checks want them.  One accepted call per family -- views,
viewports, rays with hide, hits, viewport hits with cell pairs, players, pixel rays of the whole frame -- `--calls` times in a loop,
`--reps` loops per file, the two files taking turns.  Per method: the median and the spread (least ... most) of the other file's
loops in microseconds per call, this file's median, and whether that lies within the other's spread.

    python tools/binding_overhead.py --parent /path/to/parent/render.py [--calls 10000] [--reps 5] [--out profiles/binding_calls/overhead.txt]
"""
import argparse
import ctypes as C
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Quiet:
    """render.lib's stand-in: every function of the ABI table returns 0"""

    def __init__(self, abi):
        for name, _, _ in abi:
            fn = lambda *args: 0
            fn.__name__ = name
            setattr(self, name, fn)


def subject(render):
    """(method name -> a call without arguments) on a bare renderer of `render`, 8 views of 64 x 32 and 4096 rays"""
    import torch
    render.lib = Quiet(render._lib.ABI)
    r = object.__new__(render.Renderer)
    r.w, r.h, r.device, r._ctx = 64, 32, 0, C.c_void_p()
    n, rays_n, W, H = 8, 4096, 256, 64
    lay = render.ViewportsLayout(r, C.c_void_p(0x1000), W, H, n)
    z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device="cuda:0")
    f32, i32 = torch.float32, torch.int32
    cams, secs, hide_v = z(f32, n, 16), z(f32, n), z(i32, n)
    sbuf, zbuf = z(i32, n, r.h, r.w), z(f32, n, r.h, r.w)
    a_sbuf, a_zbuf, a_label, a_cell = z(i32, H, W), z(f32, H, W), z(i32, H, W), z(torch.int16, H, W, 2)
    rays, col, depth, hide_r, hits = z(f32, rays_n, 8), z(i32, rays_n), z(f32, rays_n), z(i32, rays_n), z(i32, rays_n, 12)
    keys, gravity = z(torch.uint8, n), z(f32, n, 4)
    return {
        "trace_views_device": lambda: r.trace_views_device(cams, secs, sbuf, zbuf),
        "trace_viewports_device": lambda: r.trace_viewports_device(lay, cams, secs, a_sbuf, a_zbuf),
        "trace_rays_device(hide)": lambda: r.trace_rays_device(rays, col, depth, hide=hide_r),
        "trace_hits_device": lambda: r.trace_hits_device(rays, hits),
        "trace_viewport_hits_device(cell pairs)": lambda: r.trace_viewport_hits_device(lay, cams, a_label, cell=a_cell),
        "players_step_device": lambda: r.players_step_device(keys, cams, gravity),
        "pixel_rays_device(xy=None)": lambda: r.pixel_rays_device(cams),
    }


def loop_us(call, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the render.py to compare against")
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import pwnfps_amd.render as new
    spec = importlib.util.spec_from_file_location("pwnfps_amd.render_parent", a.parent)
    parent = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent)
    subjects = {"parent": subject(parent), "new": subject(new)}
    lines = ["# host microseconds per call, %d calls a loop, %d loops per file in alternation (parent, new, parent, ...); no call reaches the library"
             % (a.calls, a.reps),
             "%-40s %14s %20s %11s %8s  %s" % ("method", "parent median", "parent least...most", "new median", "new/par", "new within the parent's spread")]
    for name in subjects["new"]:
        for s in subjects.values():
            loop_us(s[name], a.calls // 10)                                       # warm both before the first timed loop
        t = {"parent": [], "new": []}
        for _ in range(a.reps):
            for which in ("parent", "new"):
                t[which].append(loop_us(subjects[which][name], a.calls))
        pm, nm = statistics.median(t["parent"]), statistics.median(t["new"])
        lo, hi = min(t["parent"]), max(t["parent"])
        verdict = "yes" if lo <= nm <= hi else ("faster than all of them" if nm < lo else "NO: slower by %.2f us" % (nm - hi))
        lines.append("%-40s %14.2f %20s %11.2f %8.3f  %s" % (name, pm, "%.2f...%.2f" % (lo, hi), nm, nm / pm, verdict))
        lines.append("%-40s   parent loops: %s   new loops: %s" % ("", " ".join("%.2f" % v for v in t["parent"]), " ".join("%.2f" % v for v in t["new"])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
