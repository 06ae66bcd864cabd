"""The reference for pwn_trace_hits: first-hit records read off the oracle's event chain.

pwno_debug_pixel(x, y) makes the oracle print, for that pixel, a ` segment` line per ray segment, a `  step` line per walk step
(after the step's sphere tests: the cell the step begins in, pos, ray, the w's, cdist, aux_dist, ldir) and a ` ->` line with what
the segment returned, all floats as hex.  The reader redirects file descriptor 2 to a temporary file around single-threaded
pwno_trace_rows calls of one row each, flushes C stdio and takes from segment 0:
  kind, face, dist, point   the `->` line's ev (0 = out of steps), ldir, dist and pos;
  object                    the `->` line's refl: spheres are made recognisable by giving sphere i the reflectivity (i + 1) / 32
                            (mark_spheres), which the line prints unchanged;
  portals                   the steps whose cell is 'A'..'Z' and that crossed.  Every letter step either returns or crosses, and only
                            the last step can have returned: it did unless its cell is an endpoint of a paired portal (then the
                            step crossed and trace.h:668 returned the sphere behind the crossing);
  cell                      the last step's cell, moved one along the face when that cell is '#' or '&' and the face is a side face
                            (the one return behind the reference's own cell advance);
  direction                 the last step's ray -- turned as the portal turns it when the last step crossed (see portals); its y is
                            compared only when the last step's cell is not a ramp ('>', '<', ',', '^': the step skews ray.y).
A segment that ran out of steps is PWN_HIT_NONE: face = object = -1, every other field 0.
Caller-made rays go through the trick camera (tests/test_rays_oracle.py) on a 1 x 1 frame.
Floats compare as bits; where the oracle has NaN, NaN is required.
"""
import ctypes as C
import os
import re
import tempfile
from collections import namedtuple

import numpy as np

HIT_DTYPE = np.dtype([("kind", "<i4"), ("face", "<i4"), ("object", "<i4"), ("portals", "<i4"),
                      ("dist", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                      ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("cell_x", "<i2"), ("cell_z", "<i2")])
FXP, FZP, FXN, FZN, FYP, FYN = range(6)
NONE, WALL, SPHERE = 0, 1, 2

_STEP = re.compile(rb"^  step cell '(.)' \((-?\d+),(-?\d+)\) pos (\S+) (\S+) (\S+) ray (\S+) (\S+) (\S+) w ", re.S)
_RET = re.compile(rb"^ -> ev (\d+) ldir (-?\d+) dist (\S+) fog \S+ pos (\S+) (\S+) (\S+) col \S+ \S+ \S+ refl (\S+)")
_libc = C.CDLL(None)
# what the reader gives for n rays: the records, where dy is compared, segment 0's walk steps, the last step's cell character
Ref = namedtuple("Ref", "want cmp_dy steps last_ch")


def mark_spheres(sph):
    """the spheres with sphere i's reflectivity (i + 1) / 32 (exact in fp32 up to i = 2^24)"""
    sph = np.array(sph, copy=True)
    assert len(sph) < 1 << 20
    sph["refl"] = (np.arange(len(sph), dtype=np.float32) + np.float32(1)) / np.float32(32)
    return sph


def _f(tok):
    return np.float32(float.fromhex(tok.decode()))


def _stderr_of(fn):
    """what fn() writes to file descriptor 2, C stdio flushed"""
    _libc.fflush(None)
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        try:
            os.dup2(tmp.fileno(), 2)
            fn()
            _libc.fflush(None)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return tmp.read()


class Reader:
    def __init__(self, O):
        self.O = O
        self.O.L.pwno_debug_pixel.argtypes = [C.c_int, C.c_int]
        _, pmap, _ = O.get_level()
        self.pmap = pmap

    def _crossing(self, ch, cx, cz):
        """None, or the rotation a step in letter cell ch at (cx, cz) crosses with (trace.h:547-560)"""
        x1, z1, x2, z2, rot12 = (int(v) for v in self.pmap[ch - 65][:5])
        if x2 == -1:
            return None
        if (x1, z1) == (cx, cz):
            return (-rot12) & 3
        if (x2, z2) == (cx, cz):
            return rot12 & 3
        return None

    def _record(self, lines):
        """(record, compare dy, steps of segment 0, the last step's cell character) from the lines of one pixel's chain"""
        steps = []
        ret = None
        seg = -1
        for ln in lines:
            if ln.startswith(b" segment "):
                seg += 1
                if seg > 0:
                    break
            elif ln.startswith(b"  step cell "):
                m = _STEP.match(ln)
                assert m is not None, ln
                steps.append(m)
            elif ln.startswith(b" -> "):
                ret = _RET.match(ln)
                assert ret is not None, ln
                break
        assert seg == 0 and ret is not None and steps, lines[:3]
        rec = np.zeros((), HIT_DTYPE)
        ev = int(ret.group(1))
        if ev == NONE:
            rec["face"] = rec["object"] = -1
            return rec, True, len(steps), steps[-1].group(1)[0]
        last = steps[-1]
        ch, cx, cz = last.group(1)[0], int(last.group(2)), int(last.group(3))
        face = int(ret.group(2))
        rec["kind"], rec["face"] = ev, face
        rec["dist"] = _f(ret.group(3))
        rec["x"], rec["y"], rec["z"] = _f(ret.group(4)), _f(ret.group(5)), _f(ret.group(6))
        rec["object"] = -1
        if ev == SPHERE:
            idx = float.fromhex(ret.group(7).decode()) * 32.0 - 1.0
            assert idx == int(idx) and idx >= 0, ("the spheres are not marked (mark_spheres)", idx)
            rec["object"] = int(idx)
        letters = sum(1 for s in steps if 65 <= s.group(1)[0] <= 90)
        dx, dy, dz = _f(last.group(7)), _f(last.group(8)), _f(last.group(9))
        if 65 <= ch <= 90:
            rot = self._crossing(ch, cx, cz)
            if rot is None:
                letters -= 1                    # the step returned in front of the portal
            else:
                assert ev == SPHERE, ch         # (behind a crossing only trace.h:668 returns)
                dx, dz = {0: (dx, dz), 1: (dz, -dx), 2: (-dx, -dz), 3: (-dz, dx)}[rot]
        rec["portals"] = letters
        rec["dx"], rec["dy"], rec["dz"] = dx, dy, dz
        if ch in (35, 38) and face in (FXP, FZP, FXN, FZN):
            cx += {FXP: 1, FXN: -1}.get(face, 0)
            cz += {FZP: 1, FZN: -1}.get(face, 0)
        rec["cell_x"], rec["cell_z"] = cx, cz
        return rec, bytes([ch]) not in (b">", b"<", b",", b"^"), len(steps), ch

    def _run(self, jobs):
        """jobs: (w, h, cam, x, y) each; the chains of all of them from one redirection"""
        L = self.O.L
        bufs = {}

        def go():
            for w, h, cam, x, y in jobs:
                if (w, h) not in bufs:
                    bufs[(w, h)] = (np.zeros((h, w), np.uint32), np.zeros((h, w), np.float32))
                sb, zb = bufs[(w, h)]
                L.pwno_debug_pixel(int(x), int(y))
                assert L.pwno_trace_rows(self.O.lv, w, h, int(y), int(y) + 1, cam.ctypes.data, 0.0, 1,
                                         sb.ctypes.data, zb.ctypes.data, None) == 0
        try:
            text = _stderr_of(go)
        finally:
            L.pwno_debug_pixel(-1, -1)
        chains, cur = [], []
        for ln in text.split(b"\n"):
            if ln.startswith(b"pixel "):
                chains.append(cur)
                cur = []
            elif ln:
                cur.append(ln)
        assert len(chains) == len(jobs), (len(chains), len(jobs))
        want = np.zeros(len(jobs), HIT_DTYPE)
        cmp_dy = np.zeros(len(jobs), bool)
        steps = np.zeros(len(jobs), np.int64)
        last_ch = np.zeros(len(jobs), np.uint8)
        for i, lines in enumerate(chains):
            want[i], cmp_dy[i], steps[i], last_ch[i] = self._record(lines)
        return Ref(want, cmp_dy, steps, last_ch)

    def pixels(self, w, h, cam, xy):
        """Ref of pixels xy (n,2) of camera cam's w x h frame"""
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        return self._run([(w, h, cam, x, y) for x, y in np.asarray(xy)])

    def rays(self, rec):
        """... of ray records (n,8), each through its trick camera: x and y rows zero, z row the direction, w row the origin"""
        jobs = []
        for r in np.ascontiguousarray(rec, np.float32):
            cam = np.zeros(16, np.float32)
            cam[8:12] = r[4:]
            cam[12:16] = r[:4]
            jobs.append((1, 1, cam, 0, 0))
        return self._run(jobs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mismatches(got, want, cmp_dy=None, fields=None):
    """indices where the records differ: ints equal, floats equal as bits or both NaN; dy only where cmp_dy"""
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.zeros(len(want), bool)
    for name in fields or HIT_DTYPE.names:
        g, w = got[name], want[name]
        if HIT_DTYPE[name].kind == "f":
            ne = (_bits(g) != _bits(w)) & ~(np.isnan(w) & np.isnan(g))
            if name == "dy" and cmp_dy is not None:
                ne &= cmp_dy | (want["kind"] == NONE)
        else:
            ne = g != w
        bad |= ne
    return np.flatnonzero(bad)


# ---- the three level.txt frames of the issue: level.txt with spheres_t0 (marked), 32 x 24, the camera at the spawn cell's centre,
# the identity turned about y by 0, 0.8 and 5.6 with pwno_mat4_roty

LEVEL_W, LEVEL_H = 32, 24
LEVEL_YAWS = (0.0, 0.8, 5.6)
_level_cache = {}


def level_frames(oracle_mod):
    """(Oracle, marked spheres, [camera per yaw], [Ref per yaw over every pixel in row order]); computed once"""
    if "v" not in _level_cache:
        from conftest import level_path, load_spheres
        O = oracle_mod.Oracle()
        O.load_level(level_path("pwnfps_level"))
        sph = mark_spheres(load_spheres("t0"))
        O.set_spheres(sph)
        _, _, spawn = O.get_level()
        rd = Reader(O)
        cams, refs = [], []
        for yaw in LEVEL_YAWS:
            cam = np.eye(4, dtype=np.float32)
            O.L.pwno_mat4_roty(cam.ctypes.data, C.c_float(yaw))
            cam[3, :3] = (spawn[0] + 0.5, 0.5, spawn[1] + 0.5)
            cams.append(cam)
            refs.append(rd.pixels(LEVEL_W, LEVEL_H, cam, all_pixels(LEVEL_W, LEVEL_H)))
        _level_cache["v"] = (O, sph, cams, refs)
    return _level_cache["v"]


def all_pixels(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)
