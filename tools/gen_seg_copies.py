#!/usr/bin/env python3
"""tests/golden/seg_copies.npz: 64 x 16 frames (four units across, four rows of units) whose rays end in every copy of the
segment's text (trace_segment.inc) in every way a copy can end a ray, with lanes of ONE unit leaving in each copy.

A ray ends in copy d (d = the number of surfaces it bounced off) because
    steps    it ran out of steps there (trace.h:677),
    refl0    it met a surface of reflectivity 0 there -- only a sphere can be one; walls and the ceiling have 0.25, the floor 0.7 --
    last     d = REFLECT (trace.h:3-7): every other ray.
What a pixel's ray did is read off the oracle's event chain (pwno_debug_pixel: a ` -> ev .. ldir .. fog .. refl ..` line per segment).

Scenes
    sphere      a mirror room with a sphere of reflectivity 0: met by the primary ray, behind a wall mirror, behind the floor
    fog         the same room of fog cells ('$'): fog in the segment that ends a ray of depth 0, 1 and 2, and in the entries of the
                composite stack (depth 1: A; depth 2: B and A)
    corridors   the portal-closed corridors of tools/gen_step_limit.py: rays out of steps in the first, second and third segment
    mixed       corridors of fog cells with a sphere of reflectivity 0 in the camera's: ONE unit whose lanes end on refl0, on steps
                and in the last copy, with fog behind them
The camera of the last two is searched on a fixed grid for the first frame that holds every kind asked for.

    python3 tools/gen_seg_copies.py [-v]          (CPU only; writes the fixture and prints what every frame holds)
"""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import hit_chain as HC  # noqa: E402
import oracle  # noqa: E402

W, H = 64, 16
SENTINEL = np.uint32(0x7fc12345)
OUT = os.path.join(ROOT, "tests", "golden", "seg_copies.npz")
_RET = re.compile(rb"^ -> ev (\d+) ldir (-?\d+) dist \S+ fog (\S+) pos \S+ \S+ \S+ col \S+ \S+ \S+ refl (\S+)")
STEPS, REFL0, LAST = 0, 1, 2


def chains(O, cam):
    """per pixel in row order: [(ev, ldir, fog, refl) per segment]"""
    L = O.L
    L.pwno_debug_pixel.argtypes = [C.c_int, C.c_int]
    camf = np.ascontiguousarray(cam, np.float32).reshape(16)
    sb, zb = np.zeros((H, W), np.uint32), np.zeros((H, W), np.float32)

    def go():
        for y in range(H):
            for x in range(W):
                L.pwno_debug_pixel(x, y)
                assert L.pwno_trace_rows(O.lv, W, H, y, y + 1, camf.ctypes.data, 0.0, 1, sb.ctypes.data, zb.ctypes.data, None) == 0
    try:
        text = HC._stderr_of(go)
    finally:
        L.pwno_debug_pixel(-1, -1)
    # (the chain's `pixel` line closes a pixel's lines: tests/hit_chain.py)
    out, cur = [], []
    for ln in text.split(b"\n"):
        if ln.startswith(b"pixel "):
            out.append(cur)
            cur = []
        elif ln.startswith(b" -> "):
            m = _RET.match(ln)
            assert m is not None, ln
            cur.append((int(m.group(1)), int(m.group(2)), float.fromhex(m.group(3).decode()), float.fromhex(m.group(4).decode())))
    assert len(out) == W * H and all(out), len(out)
    return out


def classify(ch):
    """(h, w) arrays: depth, kind (STEPS / REFL0 / LAST), the face of segment 0's surface, fog of the ending segment != 0,
    fog of entry A != 0, fog of entry B != 0"""
    depth = np.zeros(W * H, np.int8); kind = np.zeros(W * H, np.int8); face0 = np.full(W * H, -2, np.int8)
    fog_end = np.zeros(W * H, bool); fog_a = np.zeros(W * H, bool); fog_b = np.zeros(W * H, bool)
    for i, segs in enumerate(ch):
        d = len(segs) - 1
        ev, ldir, fog, refl = segs[-1]
        depth[i] = d
        kind[i] = STEPS if ev == 0 else (LAST if d == 2 else REFL0)
        if ev != 0 and d < 2:
            assert refl == 0.0, (i, segs)
        face0[i] = segs[0][1] if segs[0][0] == 1 else (-1 if segs[0][0] == 2 else -2)
        fog_end[i] = fog != 0.0
        fog_a[i] = d >= 1 and segs[0][2] != 0.0
        fog_b[i] = d >= 2 and segs[1][2] != 0.0
    r = lambda a: a.reshape(H, W)
    return r(depth), r(kind), r(face0), r(fog_end), r(fog_a), r(fog_b)


def units(a):
    """(h, w) -> (n_units, 64)"""
    return a.reshape(H // 4, 4, W // 16, 16).transpose(0, 2, 1, 3).reshape(-1, 64)


def holds(cls):
    """what the frame holds: counts of pixels, and of units that mix"""
    depth, kind, face0, fog_end, fog_a, fog_b = cls
    side = np.isin(face0, (HC.FXP, HC.FZP, HC.FXN, HC.FZN))
    g = {}
    for d in range(3):
        g["steps_%d" % d] = int(((kind == STEPS) & (depth == d)).sum())
        g["fog_end_%d" % d] = int((fog_end & (depth == d)).sum())
    g["refl0_0"] = int(((kind == REFL0) & (depth == 0)).sum())
    g["refl0_1_wall"] = int(((kind == REFL0) & (depth == 1) & side).sum())
    g["refl0_1_floor"] = int(((kind == REFL0) & (depth == 1) & (face0 == HC.FYN)).sum())
    g["last"] = int((kind == LAST).sum())
    g["fog_a_1"] = int((fog_a & (depth == 1)).sum()); g["fog_a_2"] = int((fog_a & (depth == 2)).sum()); g["fog_b_2"] = int(fog_b.sum())
    ud, uk = units(depth), units(kind)
    g["units_all_depths"] = int(sum(1 for u in ud if set(u.tolist()) >= {0, 1, 2}))
    g["units_all_kinds"] = int(sum(1 for d_, k_, f_ in zip(ud, uk, units(fog_a | fog_end))
                                   if set(k_.tolist()) >= {STEPS, REFL0, LAST} and f_.any()))
    return g


def room_text(cell):
    rows = ["." * 8] + ["." + cell * 6 + "." for _ in range(6)] + ["." * 8]
    return "\n".join(rows) + "\n"


def corridor_text(cell, rows=12, length=7):
    out = ["." * (length + 4)]
    for i in range(rows):
        out.append("." + chr(65 + i) + cell * length + chr(65 + i) + ".")
    out.append("." * (length + 4))
    return "\n".join(out) + "\n"


def room_scene(cell):
    sph = np.zeros(2, oracle.SPHERE_DTYPE)
    sph[0] = (0.45, 0.0, 4.5, 0.5, 1.9, 0.9, 0.6, 0.2)          # reflectivity 0: ends a ray; beside the wall z = 1, which mirrors it
    sph[1] = (0.25, 0.5, 2.6, 0.3, 5.2, 0.2, 0.9, 0.4)
    cam = np.zeros((4, 4), np.float32)
    cam[0] = (0, 0, 1.6, 0); cam[1] = (0, 1.6, 0, 0); cam[2] = (1, -0.25, 0.45, 0); cam[3] = (1.6, 0.6, 3.4, 1)
    return room_text(cell), sph, cam


def corridor_cam(pitch, yaw):
    cam = np.zeros((4, 4), np.float32)
    cam[0] = (0, 0, 0.015 * yaw, 0); cam[1] = (0, 0.012 * pitch, 0, 0); cam[2] = (1, pitch, yaw, 0); cam[3] = (5.5, 0.5, 1.5, 1)
    return cam


def frame(O, cam, sec):
    zb = np.full((H, W), SENTINEL, np.uint32).view(np.float32)
    sb, zb, st = O.trace_rows(W, H, 0, H, cam, sec=sec, threads=1, zb=zb)
    return sb, zb.view(np.uint32), np.array([st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted], np.int64)


def main():
    verbose = "-v" in sys.argv
    O = oracle.Oracle()
    scenes = {}

    def take(name, text, sph, cam, need):
        O.load_level_text(text)
        O.set_spheres(sph)
        g = holds(classify(chains(O, cam)))
        if verbose:
            print(name, {k: v for k, v in g.items() if v})
        if not all(g[k] > 0 for k in need):
            return None
        return g

    for name, cell, need in (("sphere", ";", ("refl0_0", "refl0_1_wall", "refl0_1_floor", "last", "units_all_depths")),
                             ("fog", "$", ("fog_end_0", "fog_end_1", "fog_end_2", "fog_a_1", "fog_a_2", "fog_b_2", "units_all_depths"))):
        text, sph, cam = room_scene(cell)
        g = take(name, text, sph, cam, need)
        assert g is not None, (name, "the room does not hold every kind")
        scenes[name] = (text, sph, cam, g)

    sphc = np.zeros(2, oracle.SPHERE_DTYPE)
    sphc[0] = (0.04, 0.35, 3.5, 0.93, 1.35, 0.2, 0.6, 0.9)
    sphc[1] = (0.05, 0.5, 6.5, 0.08, 1.9, 0.9, 0.3, 0.2)
    found = None
    for pitch in np.arange(5.50e-4, 6.10e-4, 0.02e-4):
        for k in (1.0, 0.99, 1.01, 0.98, 1.02, 0.9, 1.1):
            cam = corridor_cam(np.float32(pitch), np.float32(-pitch * k))
            g = take("corridors", corridor_text(";"), sphc, cam, ("steps_0", "steps_1", "steps_2", "last"))
            if g is not None:
                found = (cam, g)
                break
        if found:
            break
    assert found is not None, "corridors: no camera on the grid gives every kind"
    scenes["corridors"] = (corridor_text(";"), sphc, found[0], found[1])

    # mixed: the sphere of reflectivity 0 touches the middle of the beam at the corridor's far end, so that the frame's left part
    # meets it (behind the end wall's mirror) and its right part walks on to the step limit
    pitch = np.float32(5.7e-4)
    yaw = np.float32(-pitch)
    sphm = sphc.copy()
    sphm[0] = (0.2, 0.0, 9.5, 0.5 + 4 * float(pitch), 1.5 + 4 * float(yaw) + 0.2, 0.2, 0.6, 0.9)
    g = take("mixed", corridor_text("$"), sphm, corridor_cam(pitch, yaw), ("units_all_kinds", "units_all_depths", "steps_0", "fog_a_1", "fog_b_2"))
    assert g is not None, "mixed: the frame does not hold every kind"
    scenes["mixed"] = (corridor_text("$"), sphm, corridor_cam(pitch, yaw), g)

    save = {"wh": np.array([W, H], np.int32), "names": np.array(list(scenes))}
    for name, (text, sph, cam, g) in scenes.items():
        O.load_level_text(text)
        O.set_spheres(sph)
        sec = np.float32(0.0)          # (the chains above were read at this time: the floor ripples with it)
        sb, z, stats = frame(O, cam, float(sec))
        print(name, g, "stats", stats.tolist())
        save.update({name + "_text": np.array(text), name + "_sph": sph, name + "_cam": cam, name + "_sec": sec,
                     name + "_pre": sb, name + "_z": z, name + "_stats": stats,
                     name + "_holds": np.array(sorted(g.items()), dtype="U32")})
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
