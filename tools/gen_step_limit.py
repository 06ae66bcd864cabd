#!/usr/bin/env python3
"""tests/golden/step_limit.npz: one 64 x 16 frame whose rays end around the walk's step limit (trace.h:250, 1000 cell steps).

The scene is a hall of ROWS corridors side by side, each closed on itself by its own portal pair, so that a ray along x walks
until it drifts into a side wall, the floor or the ceiling: 8 walk iterations per 7 units of x.  The camera looks along +x with
a field of view of a few 1e-5: the rows differ in pitch by about one walk iteration each, the columns in yaw.  The pitch and the
yaw are searched on a fixed grid with the oracle's step map (pwno_step_map) and the event chains of tests/hit_chain.py for
the first frame that holds, among the PRIMARY segments,
    an event in iteration 999, an event in iteration 1000, a ray out of steps (1000 iterations, no event),
    a side-wall event and a floor / ceiling event in iteration 1000,
and a segment other than the primary one that runs out of steps (the frame's `exhausted` beyond the primary rays').
Spheres i carry the reflectivity (i + 1) / 32, so that hit_chain reads `object` off them.

    python3 tools/gen_step_limit.py            (CPU only; writes the fixture and prints what the frame holds)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import hit_chain as HC  # noqa: E402
import oracle  # noqa: E402

W, H = 64, 16
ROWS, LEN = 12, 7
SENTINEL = np.uint32(0x7fc12345)          # a NaN pattern no computation makes
ORIGIN = (5.5, 0.5, 1.5)
OUT = os.path.join(ROOT, "tests", "golden", "step_limit.npz")


def level_text():
    rows = ["." * (LEN + 4)]
    for i in range(ROWS):
        body = list(";" * LEN)
        if i == 0:
            body[LEN // 2] = "*"
        rows.append("." + chr(65 + i) + "".join(body) + chr(65 + i) + ".")
    rows.append("." * (LEN + 4))
    return "\n".join(rows) + "\n"


def spheres():
    s = np.zeros(2, oracle.SPHERE_DTYPE)
    s[0] = (0.04, 0.0, 3.5, 0.93, 1.35, 0.2, 0.6, 0.9)
    s[1] = (0.05, 0.0, 6.5, 0.08, 1.9, 0.9, 0.3, 0.2)
    return HC.mark_spheres(s)


def camera(pitch, yaw):
    """rows: pitch +- 0.3 %, columns: yaw +- 1.5 % (screen.h:43-57: ray = z row + x row * (1 - 2 (x + 1) / w) + y row * (h - 2 y) / w)"""
    cam = np.zeros((4, 4), np.float32)
    cam[0] = (0, 0, 0.015 * yaw, 0)
    cam[1] = (0, 0.012 * pitch, 0, 0)
    cam[2] = (1, pitch, yaw, 0)
    cam[3] = (*ORIGIN, 1)
    return cam


def frame(O, cam):
    """colour, depth over the sentinel, stats, step map of the frame"""
    smap = np.zeros((H, W, 3), np.uint16)
    zb = np.full((H, W), SENTINEL, np.uint32).view(np.float32)
    O.L.pwno_step_map.argtypes = [C.c_void_p]
    O.L.pwno_step_map(smap.ctypes.data)
    try:
        sb, zb, st = O.trace_rows(W, H, 0, H, cam, threads=1, zb=zb)
    finally:
        O.L.pwno_step_map(None)
    return sb, zb, st, smap


def kinds(zb, st, smap, ref):
    """what the frame holds: a dict of counts (ref: hit_chain.Ref over every pixel in row order)"""
    none = (zb.view(np.uint32) == SENTINEL).ravel()
    s0 = smap[:, :, 0].ravel()
    face = ref.want["face"]
    side = np.isin(face, (HC.FXP, HC.FZP, HC.FXN, HC.FZN))
    flat = np.isin(face, (HC.FYP, HC.FYN))
    return {"event_999": int(((s0 == 999) & ~none).sum()), "event_1000": int(((s0 == 1000) & ~none).sum()),
            "out_of_steps": int(none.sum()),
            "wall_1000": int(((s0 == 1000) & ~none & side).sum()), "flat_1000": int(((s0 == 1000) & ~none & flat).sum()),
            "later_out_of_steps": int(st.exhausted - none.sum())}


def main():
    O = oracle.Oracle()
    text = level_text()
    O.load_level_text(text)
    sph = spheres()
    O.set_spheres(sph)
    rd = HC.Reader(O)
    xy = HC.all_pixels(W, H)
    found = None
    for pitch in np.arange(5.66e-4, 5.90e-4, 0.01e-4):
        for k in (1.0, 0.99, 1.01, 0.98, 1.02):
            cam = camera(np.float32(pitch), np.float32(-pitch * k))
            sb, zb, st, smap = frame(O, cam)
            none = zb.view(np.uint32) == SENTINEL
            s0 = smap[:, :, 0]
            if not (((s0 == 999) & ~none).any() and ((s0 == 1000) & ~none).sum() >= 2 and none.any() and st.exhausted > none.sum()):
                continue
            ref = rd.pixels(W, H, cam, xy)
            got = kinds(zb, st, smap, ref)
            if "-v" in sys.argv:
                print("pitch %.4e yaw factor %.2f" % (pitch, k), got)
            if all(v > 0 for v in got.values()):
                found = (cam, sb, zb, st, smap, ref, got)
                break
        if found:
            break
    assert found is not None, "no camera on the grid gives every kind"
    cam, sb, zb, st, smap, ref, got = found
    print("pitch %.6e yaw %.6e" % (cam[2, 1], cam[2, 2]), got)
    assert (ref.steps == smap[:, :, 0].ravel()).all()
    np.savez_compressed(OUT, text=np.array(text), cam=cam, sph=sph, sec=np.float32(0.0), wh=np.array([W, H], np.int32),
                        pre=sb, z=zb.view(np.uint32), smap=smap,
                        stats=np.array([st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted], np.int64),
                        hits=ref.want, cmp_dy=ref.cmp_dy)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
