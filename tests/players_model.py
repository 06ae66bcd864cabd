"""The model of pwn_players_step and the corpus its tests walk.

The model is host/player.c itself: compiled here with tests/players_driver.c into a shared object, with host/Makefile's flags
(-ffp-contract=off above all), and called as model_step(data, pmap, keys, tdiff, ticks, cams, gravity, traversals).

The corpus: seeded start states on the shipped level (positions in free cells and within 0.25 of every wall side and corner,
heights 0.4 .. 1.95, headings over the full circle, random gravity and keys, cameras with denormal entries and w lanes, positions
in (-1, 0) and beyond 64), players that walk into every portal endpoint and over every edge of a two-high room, and turn-only
players whose angle takes the sine's general path.  A hand-made level (HAND_LEVEL) has a portal of every rotation, entered from
both endpoints, and an unpaired letter.  classify() names what a tick did from the states before and after it alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from conftest import GOLD, ROOT

F = np.float32
TURN_LEFT, TURN_RIGHT, TURN_UP, TURN_DOWN, FORWARD, BACK, LEFT, RIGHT = (1 << i for i in range(8))
BBOX = F(0.2)

# A level of corridors: first endpoints open towards +x; the second ones towards -x, +x, +z and -z, which makes rot12 0, 2, 3 and 1
# (level.h:194-221); E has one endpoint only; a two-high room with both kinds of low neighbour; the spawn.
HAND_LEVEL = "\r\n".join([
    "..............",
    ".A;;;....;;;A.",
    "..............",
    ".B;;;....B;;;.",
    "..............",
    ".C;;;....C....",
    ".........;....",
    ".........;....",
    "..............",
    ".........;....",
    ".........;....",
    ".D;;;....D....",
    "..............",
    ".E;;;.........",
    "..............",
    ".;;\"##\"&&\";;..",
    "..............",
    ".;*;;.........",
    ""])
HAND_ROT12 = {"A": 0, "B": 2, "C": 3, "D": 1}

_model = None


def _lib():
    global _model
    if _model is None:
        out = os.path.join(tempfile.mkdtemp(prefix="players_model_"), "libplayersmodel.so")
        subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-Wall", "-Wextra", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "host"), "-o", out,
                               os.path.join(ROOT, "host", "player.c"), os.path.join(ROOT, "tests", "players_driver.c"), "-lm"])
        L = C.CDLL(out)
        L.players_model_step.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.players_model_step.restype = None
        _model = L
    return _model


def model_step(data, pmap, keys, tdiff, ticks, cams, gravity, traversals):
    """`ticks` pwn_player_step calls per player; returns new (cams, gravity, traversals) -- traversals None where none was given"""
    data = np.ascontiguousarray(data, np.uint8)
    pmap = np.ascontiguousarray(pmap, np.int32)
    keys = np.ascontiguousarray(keys, np.uint8)
    assert data.size == 4096 and pmap.size == 26 * 7
    c = np.array(cams, np.float32, order="C")
    g = np.array(gravity, np.float32, order="C")
    t = np.array(traversals, np.int32, order="C") if traversals is not None else None
    n = keys.shape[0]
    assert c.size == 16 * n and g.size == 4 * n and (t is None or t.size == n)
    _lib().players_model_step(n, int(ticks), keys.ctypes.data, float(tdiff), data.ctypes.data, pmap.ctypes.data,
                              c.ctypes.data, g.ctypes.data, t.ctypes.data if t is not None else None)
    return c, g, t


def model_step_inplace(data, pmap, keys, tdiff, ticks, cams, gravity, traversals):
    """the driver alone, on the caller's own C-contiguous arrays, stepped in place: nothing is allocated or copied (what a timer wants)"""
    for a, t in ((data, np.uint8), (pmap, np.int32), (keys, np.uint8), (cams, np.float32), (gravity, np.float32), (traversals, np.int32)):
        assert a.dtype == t and a.flags["C_CONTIGUOUS"]
    _lib().players_model_step(keys.shape[0], int(ticks), keys.ctypes.data, float(tdiff), data.ctypes.data, pmap.ctypes.data,
                              cams.ctypes.data, gravity.ctypes.data, traversals.ctypes.data)


# ---- levels -------------------------------------------------------------------------------------

def shipped_level():
    t = np.load(os.path.join(GOLD, "levels", "pwnfps_level_tables.npz"))
    return np.ascontiguousarray(t["data"], np.uint8).reshape(64, 64), np.ascontiguousarray(t["pmap"], np.int32).reshape(26, 7)


def parse_level(text):
    """(data, pmap) of a level text, by the checker's parser (oracle/, level.h:107-228)"""
    import oracle
    o = oracle.Oracle()
    o.load_level_text(text)
    data, pmap, _ = o.get_level()
    return data, pmap


OPEN = b';$"#&><^,'


def cell(data, cx, cz):
    """get_cell (util.h:151-158)"""
    cx = np.where((cx < 0) | (cx >= 64), 0, cx)
    cz = np.where((cz < 0) | (cz >= 64), 0, cz)
    return data.reshape(64, 64)[cz, cx]


# ---- start states ---------------------------------------------------------------------------------

def make_cams(x, y, z, heading):
    """cameras at (x, y, z) looking along `heading` (mat4_iden turned about y, util.h:91-110), w lanes 0, 0, 0, 1"""
    n = len(x)
    s, c = np.sin(heading.astype(F)).astype(F), np.cos(heading.astype(F)).astype(F)
    cams = np.zeros((n, 16), F)
    cams[:, 0], cams[:, 2], cams[:, 5], cams[:, 8], cams[:, 10], cams[:, 15] = c, -s, 1, s, c, 1
    cams[:, 12], cams[:, 13], cams[:, 14] = x, y, z
    return cams


def corpus_states(data, n=4096, seed=20250601):
    """n start states on `data` with one key byte each: (keys, cams, gravity, traversals), seeded"""
    rng = np.random.default_rng(seed)
    d = data.reshape(64, 64)
    free = np.argwhere(np.isin(d, np.frombuffer(OPEN, np.uint8)))          # (z, x) of cells one can stand in
    pick = free[rng.integers(0, len(free), n)]
    cz, cx = pick[:, 0].astype(F), pick[:, 1].astype(F)
    # a third anywhere in the cell; the rest within 0.25 of a side or a corner of it (walls are where the neighbours are solid)
    kind = rng.integers(0, 3, n)
    near = lambda: np.where(rng.integers(0, 2, n) == 0, rng.uniform(0.0, 0.25, n), rng.uniform(0.75, 1.0, n))
    fx = np.where(kind == 0, rng.uniform(0, 1, n), near())
    fz = np.where(kind == 1, rng.uniform(0, 1, n), near())
    fz = np.where(kind == 0, rng.uniform(0, 1, n), fz)
    x, z = (cx + fx).astype(F), (cz + fz).astype(F)
    y = rng.uniform(0.4, 1.95, n).astype(F)
    cams = make_cams(x, y, z, rng.uniform(-np.pi, np.pi, n))
    gravity = np.zeros((n, 4), F)
    gravity[:, 1] = -rng.uniform(0.0, 0.05, n)
    keys = rng.integers(0, 256, n).astype(np.uint8)
    q = n // 16
    # all four lanes of the gravity, and w lanes in the camera: they take part like the others (host/player.c)
    gravity[0:q] = rng.uniform(-0.01, 0.01, (q, 4))
    cams[q:2 * q, 3], cams[q:2 * q, 11] = rng.uniform(-1, 1, q), rng.uniform(-1, 1, q)
    cams[q:2 * q, 15] = rng.uniform(-2, 2, q)
    # denormal entries in the camera's rows and the gravity
    den = (rng.integers(1, 1 << 22, (q, 4)).astype(np.uint32) | (rng.integers(0, 2, (q, 4)).astype(np.uint32) << 31)).view(F)
    cams[2 * q:3 * q, 1], cams[2 * q:3 * q, 9], cams[2 * q:3 * q, 3] = den[:, 0], den[:, 1], den[:, 2]
    gravity[2 * q:3 * q, 0] = den[:, 3]
    # outside the grid: (int) truncates (-1, 0) to cell 0, and get_cell sends everything else outside to row / column 0
    e = q // 4
    o = 3 * q
    cams[o:o + e, 12] = -rng.uniform(0.01, 0.99, e)
    cams[o + e:o + 2 * e, 14] = -rng.uniform(0.01, 0.99, e)
    cams[o + 2 * e:o + 3 * e, 12] = rng.uniform(64.0, 70.0, e)
    cams[o + 3 * e:o + 4 * e, 14] = rng.uniform(64.0, 1000.0, e)
    cams[o + 4 * e:o + 5 * e, 12] = -rng.uniform(1.0, 300.0, e)
    cams[o + 5 * e:o + 6 * e, 14] = -rng.uniform(1.0, 5.0, e)
    # heights on a ceiling exactly (util.h:112-126 compares with >=), at rest for the first tick
    for lo, y in ((o + 6 * e, 1.0), (o + 7 * e, 2.0)):
        cams[lo:lo + e, 13] = y
        gravity[lo:lo + e, 1] = 0
    # rows y of the cameras are the caller's: never read, never written
    cams[:, 4:8] = rng.uniform(-1, 1, (n, 4))
    return keys, cams, gravity, rng.integers(0, 1000, n).astype(np.int32)


DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))


def edge_walkers(data, pmap):
    """players that stand in the middle of an open cell and walk forward into a neighbour: into every paired portal letter from each
    of its open neighbours, and over every edge between a '"' and a '#' / '&' cell, both ways.  An unpaired letter is solid
    (util.h:124): its players stand still and a gravity of 0.6 along the way carries them in, behind the push-back.
    (keys, cams, gravity, traversals)"""
    d = data.reshape(64, 64)
    xs, ys, zs, hs, gs = [], [], [], [], []
    for z in range(64):
        for x in range(64):
            c = int(d[z, x])
            for dx, dz in DIRS:
                nx, nz = x + dx, z + dz
                if not (0 <= nx < 64 and 0 <= nz < 64):
                    continue
                nb = int(d[nz, nx])
                y, g = None, (0.0, 0.0)
                if ord("A") <= nb <= ord("Z") and c in OPEN:
                    y = 1.5 if c in b"#&" else 0.5
                    if pmap[nb - 65, 2] == -1:
                        g = (0.6 * dx, 0.6 * dz)
                elif c == ord('"') and nb in b"#&":
                    y = 0.5
                elif c in b"#&" and nb == ord('"'):
                    y = 1.5
                if y is None:
                    continue
                xs.append(x + 0.5); ys.append(y); zs.append(z + 0.5); hs.append(np.arctan2(dx, dz)); gs.append(g)
    n = len(xs)
    cams = make_cams(np.array(xs, F), np.array(ys, F), np.array(zs, F), np.array(hs, np.float64))
    gravity = np.zeros((n, 4), F)
    gravity[:, 0], gravity[:, 2] = np.array(gs, F)[:, 0], np.array(gs, F)[:, 1]
    keys = np.where((gravity[:, 0] == 0) & (gravity[:, 2] == 0), FORWARD, 0).astype(np.uint8)
    return keys, cams, gravity, np.zeros(n, np.int32)


def turners(n=64, seed=7):
    """turn-only players for tdiff = 1e6: the angle 3e6 is far beyond the sine's middle path (glibc's reduction by 4 / pi words)"""
    rng = np.random.default_rng(seed)
    cams = make_cams(np.full(n, 9.5, F), np.full(n, 0.5, F), np.full(n, 4.5, F), rng.uniform(-np.pi, np.pi, n))
    keys = np.where(np.arange(n) % 2 == 0, TURN_LEFT, TURN_RIGHT).astype(np.uint8)
    return keys, cams, np.zeros((n, 4), F), np.zeros(n, np.int32)


def concat(*sets):
    return tuple(np.concatenate([s[i] for s in sets]) for i in range(4))


# ---- what a tick did, from the states before and after --------------------------------------------

def _solid(pmap, c, old, y):
    """util.h:112-126"""
    if c == ord('"') and old in b"#&":
        return y < 1 or y >= 2
    if c in b"#&":
        return y < 0 or y >= 2
    if c in b';$"><^,':
        return y < 0 or y >= 1
    if ord("A") <= c <= ord("Z"):
        return pmap[c - 65, 2] == -1
    return True


def classify(data, pmap, keys, tdiff, before, after):
    """The set of events the tick from `before` to `after` (each (cams, gravity, traversals)) shows over the batch.  Push-back and
    portal events are read off players that do not turn and whose gravity has no x / z part: their camera rows are the tick's."""
    ev = set()
    cb, gb, tb = before
    ca, ga, ta = after
    td = F(tdiff)
    d = data.reshape(64, 64)
    k = keys.astype(np.int32)
    fwd = (td * F(5)) * (((k >> 4) & 1) - ((k >> 5) & 1)).astype(F)
    side = (td * F(5)) * (((k >> 6) & 1) - ((k >> 7) & 1)).astype(F)
    still = ((k & 3) == 0) | ((k & 3) == 3)
    with np.errstate(all="ignore"):
        vel = cb[:, 8:12] * fwd[:, None] + cb[:, 0:4] * side[:, None]
        p1 = cb[:, 12:16] + vel
        cx1, cz1 = np.trunc(cb[:, 12]).astype(np.int64), np.trunc(cb[:, 14]).astype(np.int64)
        if ((cx1 < 0) | (cx1 >= 64)).any():
            ev.add("clamp x")
        if ((cz1 < 0) | (cz1 >= 64)).any():
            ev.add("clamp z")
        gx = np.where(vel[:, 0] < 0, -1, 1)
        gz = np.where(vel[:, 2] < 0, -1, 1)
        bcx = np.trunc(p1[:, 0] + gx.astype(F) * BBOX).astype(np.int64)
        bcz = np.trunc(p1[:, 2] + gz.astype(F) * BBOX).astype(np.int64)
        backx = cx1.astype(F) + F(0.5) + F(F(0.5) - BBOX) * gx.astype(F)
        backz = cz1.astype(F) + F(0.5) + F(F(0.5) - BBOX) * gz.astype(F)
        plain = still & (gb[:, 0] == 0) & (gb[:, 2] == 0)
        same = ta == tb if ta is not None else np.ones(len(k), bool)
        px = plain & same & (ca[:, 12] == backx) & (p1[:, 0] != backx)
        pz = plain & same & (ca[:, 14] == backz) & (p1[:, 2] != backz)
        diag = (cx1 != bcx) & (cz1 != bcz)
        if (diag & px & pz).any():
            ev.add("push diagonal both")
        if (diag & px & ~pz).any():
            ev.add("push diagonal x")
        for i in np.nonzero(diag & pz & ~px)[0]:
            old = int(cell(d, cx1[i], cz1[i]))
            solz = _solid(pmap, int(cell(d, cx1[i], bcz[i])), old, p1[i, 1])
            ev.add("push diagonal z" if solz else "push diagonal corner")
        if (~diag & (cx1 != bcx) & px).any():
            ev.add("push x arm")
        if (~diag & (cx1 == bcx) & (cz1 != bcz) & pz).any():
            ev.add("push z arm")
        # the floor
        ypre = p1[:, 1] + gb[:, 1]
        if ((ypre < F(0.4)) & (ca[:, 13] == F(0.4)) & (ga[:, 1] == 0)).any():
            ev.add("floor clamp")
        # a new cell: the steps of a two-high room, portals
        cx2, cz2 = np.trunc(ca[:, 12]).astype(np.int64), np.trunc(ca[:, 14]).astype(np.int64)
        c1, c2 = cell(d, cx1, cz1), cell(d, cx2, cz2)
        two = np.isin(c1, [35, 38]), np.isin(c2, [35, 38])
        dy = ca[:, 13] - np.maximum(ypre, F(0.4))
        if (same & two[0] & (c2 == 34) & (np.abs(dy + 1) < 0.01)).any():
            ev.add("step down")
        if (same & (c1 == 34) & two[1] & (np.abs(dy - 1) < 0.01)).any():
            ev.add("step up")
        if ta is not None:
            for i in np.nonzero(plain & (ta == tb + 1))[0]:
                # the cell entered, before the portal moved the player: the position behind the move (no push-back on the way in)
                ex, ez = int(np.trunc(p1[i, 0])), int(np.trunc(p1[i, 2]))
                c = int(cell(d, np.int64(ex), np.int64(ez)))
                if not ord("A") <= c <= ord("Z"):
                    continue
                pm = pmap[c - 65]
                if (pm[0], pm[1]) == (ex, ez):
                    ev.add("portal 1->2 rot %d" % ((-int(pm[4])) & 3))
                elif (pm[2], pm[3]) == (ex, ez):
                    ev.add("portal 2->1 rot %d" % (int(pm[4]) & 3))
        if ta is not None:
            # an unpaired letter moves nobody: the player stands in it afterwards
            letter = (c2 >= 65) & (c2 <= 90) & ((cx1 != cx2) | (cz1 != cz2)) & (ta == tb + 1)
            if (letter & (pmap[np.clip(c2.astype(np.int64) - 65, 0, 25), 2] == -1)).any():
                ev.add("portal unpaired")
    if (np.abs(td * F(3)) >= 120) and (((k & 3) == 1) | ((k & 3) == 2)).any():
        ev.add("sine general path")
    return ev


WANTED = (["push diagonal both", "push diagonal x", "push diagonal z", "push diagonal corner", "push x arm", "push z arm",
           "floor clamp", "step up", "step down", "portal unpaired", "clamp x", "clamp z", "sine general path"] +
          ["portal %s rot %d" % (w, r) for w in ("1->2", "2->1") for r in range(4)])


def walk_events(data, pmap, start, tdiff, ticks):
    """the events of `ticks` single ticks from `start` = (keys, cams, gravity, traversals), and the last state"""
    keys, state = start[0], start[1:]
    ev = set()
    for _ in range(ticks):
        nxt = model_step(data, pmap, keys, tdiff, 1, *state)
        ev |= classify(data, pmap, keys, tdiff, state, nxt)
        state = nxt
    return ev, state
