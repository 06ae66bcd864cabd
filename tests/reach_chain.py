"""The reference for pwn_trace_reach: records read off the oracle's event chain, as tests/hit_chain.py reads pwn_trace_hits'.

The chain of a ray does not depend on its reach, so it is read once (Chains) and the record for any reach is derived from it
(model).  The `  step` lines print pos, ray, cdist and aux_dist at the top of every step (after the step's sphere tests, which
change none of pos, ray and cdist), the ` ->` line what the walk returned.  The definition (include/pwnhip.h):
  the walk stops behind the first step that leaves cdist > reach, or where the unlimited walk returns, whichever comes first;
  D = the returned dist (aux_dist of a sphere, cdist of a wall);
  returned and not D > reach     hit_chain's own record, bit for bit;
  out of steps first             PWN_HIT_NONE;
  otherwise PWN_HIT_FREE read off the step k the walk stopped behind: face = object = -1, portals = the letter steps in front of
  k (every one of them crossed: only a chain's last step can have returned), dist = reach, cell = step k's, dx dy dz = step k's
  ray, x y z = pos_k + (reach - cdist_k) * a in fp32, every operation rounded by itself, a = ray_k with the ramp's skew restated
  from the cell character where step k's cell is a ramp (trace.h:443-505: ray.y -+= 0.5 * (ray.x or ray.z)).
cdist_{k+1} is the next step's printed cdist; behind a chain's last step it is not printed, and not needed where the walk returned
(D decides).  A ray is LEFT OUT only where the chain cannot decide: an out-of-steps chain whose last printed cdist is <= reach
(the last step may or may not have passed it), or a FREE record with a denormal among its inputs and intermediates (the kernel
flushes them, numpy does not).  model() says which rays it left out; every user asserts that they are <= 1 % of its rays.
"""
import re
from collections import namedtuple

import numpy as np

import hit_chain as HC

FREE = 3
F = np.float32
REACHES = (0.0, 0.25, 1.0, 3.7, 20.0, float("inf"))
RAMPS = {ord(">"): (True, True), ord("<"): (True, False), ord(","): (False, True), ord("^"): (False, False)}        # (along x, minus)

_STEP = re.compile(rb"^  step cell '(.)' \((-?\d+),(-?\d+)\) pos (\S+) (\S+) (\S+) ray (\S+) (\S+) (\S+) w \S+ \S+ \S+ cdist (\S+) aux (\S+) ", re.S)

# One ray's chain: per step the cell character, cell, pos, ray and cdist; what the walk returned (ev, D); hit_chain's record for the
# unlimited walk and where its dy is compared; which end of which letter every crossing went in at (0 = the first endpoint)
Chain = namedtuple("Chain", "ch cell pos ray cdist ev dist rec cmp_dy crossings")
# model()'s answer for n rays: the records, where dy is compared, the rays left out, the steps each walk took (-1 where left out), the
# arm each record came out of (a short string, for the corpus test)
Want = namedtuple("Want", "want cmp_dy left_out steps arm")


class Chains:
    """the chains of a batch of rays, read once"""

    def __init__(self, O):
        self.rd = HC.Reader(O)

    def _chain(self, lines):
        rec, cmp_dy, nsteps, _ = self.rd._record(lines)
        steps, ret = [], None
        for ln in lines:
            if ln.startswith(b" segment ") and steps:
                break
            if ln.startswith(b"  step cell "):
                m = _STEP.match(ln)
                assert m is not None, ln
                steps.append(m)
            elif ln.startswith(b" -> "):
                ret = HC._RET.match(ln)
                break
        assert ret is not None and len(steps) == nsteps
        ch = np.array([s.group(1)[0] for s in steps], np.uint8)
        cell = np.array([[int(s.group(2)), int(s.group(3))] for s in steps], np.int32)
        pos = np.array([[HC._f(s.group(i)) for i in (4, 5, 6)] for s in steps], F)
        ray = np.array([[HC._f(s.group(i)) for i in (7, 8, 9)] for s in steps], F)
        cdist = np.array([HC._f(s.group(10)) for s in steps], F)
        crossings = []
        for k in range(len(steps)):
            if 65 <= ch[k] <= 90:
                x1, z1 = (int(v) for v in self.rd.pmap[ch[k] - 65][:2])
                crossings.append((chr(ch[k]), 0 if (x1, z1) == tuple(cell[k]) else 1))
        return Chain(ch, cell, pos, ray, cdist, int(ret.group(1)), HC._f(ret.group(3)), rec, bool(cmp_dy), crossings)

    def _run(self, jobs):
        L = self.rd.O.L
        bufs = {}

        def go():
            for w, h, cam, x, y in jobs:
                if (w, h) not in bufs:
                    bufs[(w, h)] = (np.zeros((h, w), np.uint32), np.zeros((h, w), np.float32))
                sb, zb = bufs[(w, h)]
                L.pwno_debug_pixel(int(x), int(y))
                assert L.pwno_trace_rows(self.rd.O.lv, w, h, int(y), int(y) + 1, cam.ctypes.data, 0.0, 1, sb.ctypes.data, zb.ctypes.data, None) == 0
        try:
            text = HC._stderr_of(go)
        finally:
            L.pwno_debug_pixel(-1, -1)
        chains, cur = [], []
        for ln in text.split(b"\n"):
            if ln.startswith(b"pixel "):
                chains.append(self._chain(cur))
                cur = []
            elif ln:
                cur.append(ln)
        assert len(chains) == len(jobs), (len(chains), len(jobs))
        return chains

    def pixels(self, w, h, cam, xy):
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        return self._run([(w, h, cam, x, y) for x, y in np.asarray(xy)])

    def rays(self, rec):
        """ray records (n,8), each through hit_chain's trick camera"""
        jobs = []
        for r in np.ascontiguousarray(rec, np.float32):
            cam = np.zeros(16, np.float32)
            cam[8:12] = r[4:]
            cam[12:16] = r[:4]
            jobs.append((1, 1, cam, 0, 0))
        return self._run(jobs)


def _denormal(*vals):
    for v in vals:
        v = np.abs(np.asarray(v, F))
        if ((v > 0) & (v < F(2.0 ** -126))).any():
            return True
    return False


def _free(c, k, reach):
    """(record, decidable) of a walk of chain c that stopped behind step k"""
    rec = np.zeros((), HC.HIT_DTYPE)
    rec["kind"], rec["face"], rec["object"] = FREE, -1, -1
    rec["portals"] = int(((c.ch[:k] >= 65) & (c.ch[:k] <= 90)).sum())
    rec["dist"] = reach
    rec["cell_x"], rec["cell_z"] = c.cell[k]
    rx, ry, rz = c.ray[k]
    rec["dx"], rec["dy"], rec["dz"] = rx, ry, rz
    ay = ry
    skew = F(0)
    if int(c.ch[k]) in RAMPS:
        alongx, minus = RAMPS[int(c.ch[k])]
        skew = F(F(0.5) * (rx if alongx else rz))
        ay = F(ry - skew) if minus else F(ry + skew)
    with np.errstate(all="ignore"):
        rem = F(F(reach) - c.cdist[k])
        prod = [F(rem * a) for a in (rx, ay, rz)]
        pt = [F(p + q) for p, q in zip(c.pos[k], prod)]
    rec["x"], rec["y"], rec["z"] = pt
    return rec, not _denormal(reach, c.cdist[k], c.pos[k], c.ray[k], skew, ay, rem, prod, pt)


def model_one(c, reach):
    """(record, compare dy, decidable, steps taken, arm) of chain c under `reach`"""
    reach = F(reach)
    K = len(c.cdist)
    with np.errstate(invalid="ignore"):
        over = np.flatnonzero(c.cdist[1:] > reach)           # step k leaves cdist_{k+1} > reach, k < K - 1
        k = int(over[0]) if len(over) else -1
        if k < 0:
            if c.ev == HC.NONE:
                # out of steps: the last step's own cdist is not printed
                if np.isnan(reach) or reach == F(np.inf):
                    return c.rec, True, True, K, "none"
                return c.rec, True, False, -1, "undecided"
            if not (c.dist > reach):
                return c.rec, c.cmp_dy, True, K, "wall" if c.ev == HC.WALL else "sphere"
            k = K - 1
            arm = "free_wall_same_step" if c.ev == HC.WALL else "free_sphere_beyond"
        else:
            arm = "free"
    rec, ok = _free(c, k, reach)
    return rec, True, ok, k + 1 if ok else -1, arm if ok else "denormal"


def model(chains, reach):
    """Want of the chains under reach (one value, or one per ray)"""
    n = len(chains)
    reach = np.broadcast_to(np.asarray(reach, F), (n,))
    want = np.zeros(n, HC.HIT_DTYPE)
    cmp_dy = np.zeros(n, bool)
    left = np.zeros(n, bool)
    steps = np.zeros(n, np.int64)
    arm = []
    for i, c in enumerate(chains):
        want[i], cmp_dy[i], ok, steps[i], a = model_one(c, reach[i])
        left[i] = not ok
        arm.append(a)
    return Want(want, cmp_dy, left, steps, np.array(arm))


def mismatches(got, w):
    """indices, among the rays the model did not leave out, where the records differ (hit_chain.mismatches' rules)"""
    keep = np.flatnonzero(~w.left_out)
    bad = HC.mismatches(got[keep], w.want[keep], w.cmp_dy[keep])
    return keep[bad]


# ---- the corpus: level.txt with its 14 spheres (marked) from three cameras at 40 x 26; a hand-made level with every ramp kind, fog,
# the two-high room's cells, every portal rotation from both ends, an unpaired letter and a corridor closed on itself, from cameras in
# every corridor looking both ways at 12 x 8; 256 seeded pixels each of two hard scenes (tests/hard_scenes.py): random cells of every
# kind around the camera, and a camera inside a sphere.

LEVEL_W, LEVEL_H = 40, 26
LEVEL_YAWS = (0.0, 0.8, 5.6)
HAND_W, HAND_H = 12, 8
# (tests/players_model.py's second level with fog, ramps, the loop F and a sphere in the A corridor: A, B, C, D have rot12 0, 2, 3, 1)
HAND_LEVEL = "\r\n".join([
    "..............",
    ".A;$;....;>;A.",
    "..............",
    ".B;<;....B;,;.",
    "..............",
    ".C;;;....C....",
    ".........;....",
    ".........^....",
    "..............",
    ".........,....",
    ".........;....",
    ".D;;;....D....",
    "..............",
    ".E;$;.........",
    "..............",
    ".;;\"##\"&&\";;..",
    "..............",
    ".;*;;....F;;F.",
    ""])
# x, z, yaw, pitch: in every corridor, looking both ways along it
HAND_CAMS = [(3.5, 1.5, 0.5 * np.pi, 0.0), (3.5, 1.5, 1.5 * np.pi, 0.05), (10.5, 1.5, 0.5 * np.pi, 0.02), (10.5, 1.5, 1.5 * np.pi, 0.0),
             (3.5, 3.5, 0.5 * np.pi, 0.0), (3.5, 3.5, 1.5 * np.pi, -0.03), (11.5, 3.5, 0.5 * np.pi, 0.0), (11.5, 3.5, 1.5 * np.pi, 0.04),
             (2.5, 5.5, 0.5 * np.pi, 0.0), (3.5, 5.5, 1.5 * np.pi, 0.0), (9.5, 7.5, 0.0, 0.0), (9.5, 7.5, np.pi, 0.03),
             (9.5, 10.5, 0.0, 0.0), (9.5, 10.5, np.pi, 0.0), (3.5, 11.5, 0.5 * np.pi, 0.0), (3.5, 11.5, 1.5 * np.pi, 0.0),
             (3.5, 13.5, 0.5 * np.pi, 0.0), (3.5, 13.5, 1.5 * np.pi, 0.0),
             (1.5, 15.5, 0.5 * np.pi, 0.1), (11.5, 15.5, 1.5 * np.pi, 0.1), (5.5, 15.5, 0.5 * np.pi, -0.2), (7.5, 15.5, 1.5 * np.pi, 0.3),
             (10.5, 17.5, 0.5 * np.pi, 0.0), (10.5, 17.5, 1.5 * np.pi, 0.01), (2.5, 17.5, 0.5 * np.pi, 0.0), (2.5, 17.5, 1.5 * np.pi, 0.0)]
# rays along +x or -x whose steps and walls lie at a reach of the list exactly (cdist == reach is not exceeded, D == reach is within
# reach), and one that starts in a portal's cell (under a negative reach it stops behind the crossing step and is read off in front of
# it); six of each in a row, so that every one meets every value of the hostile batch
HAND_AXIS = [((2.75, 0.5, 1.5), (1, 0, 0)), ((3.0, 0.5, 1.5), (1, 0, 0)), ((4.75, 0.5, 13.5), (1, 0, 0)), ((4.0, 0.5, 13.5), (1, 0, 0)),
             ((1.5, 0.5, 1.5), (-1, 0, 0))]
HARD = ("open_inside", "sphere_cam_inside")
HARD_PIXELS = 256

Part = namedtuple("Part", "name level spheres rays chains")
_corpus = {}


def hand_spheres(sphere_dtype):
    s = np.zeros(3, sphere_dtype)
    s[0] = (0.2, 0.5, 10.5, 0.5, 1.5, 1.0, 0.5, 0.2)         # in the A corridor's far half
    s[1] = (0.15, 0.5, 3.5, 0.4, 13.5, 0.2, 1.0, 0.2)        # in the E corridor, around its camera's neighbourhood
    s[2] = (0.25, 0.5, 6.5, 1.2, 15.5, 0.2, 0.5, 1.0)        # in the upper half of the two-high room
    return s


def corpus(oracle_mod):
    """[Part]: per part the level (a path or a text), its marked spheres, the ray records (n,8) and their chains; computed once"""
    if "v" in _corpus:
        return _corpus["v"]
    import pwnfps_amd
    import edge_scenes
    import hard_scenes as HS
    from conftest import level_path, load_spheres
    parts = []
    # level.txt
    O = oracle_mod.Oracle()
    O.load_level(level_path("pwnfps_level"))
    sph = HC.mark_spheres(load_spheres("t0"))
    O.set_spheres(sph)
    _, _, spawn = O.get_level()
    ch = Chains(O)
    rays, chains = [], []
    xy = HC.all_pixels(LEVEL_W, LEVEL_H)
    for yaw in LEVEL_YAWS:
        cam = edge_scenes._cam(spawn[0] + 0.5, 0.5, spawn[1] + 0.5, yaw)
        rays.append(pwnfps_amd.pixel_rays(LEVEL_W, LEVEL_H, cam, xy)[0])
        chains += ch.pixels(LEVEL_W, LEVEL_H, cam, xy)
    parts.append(Part("level", level_path("pwnfps_level"), sph, np.concatenate(rays), chains))
    # the hand-made level
    O = oracle_mod.Oracle()
    O.load_level_text(HAND_LEVEL)
    sph = HC.mark_spheres(hand_spheres(oracle_mod.SPHERE_DTYPE))
    O.set_spheres(sph)
    ch = Chains(O)
    rays, chains = [], []
    xy = HC.all_pixels(HAND_W, HAND_H)
    for x, z, yaw, pitch in HAND_CAMS:
        cam = edge_scenes._cam(x, 0.5, z, yaw, pitch)
        rays.append(pwnfps_amd.pixel_rays(HAND_W, HAND_H, cam, xy)[0])
        chains += ch.pixels(HAND_W, HAND_H, cam, xy)
    axis = np.zeros((6 * len(HAND_AXIS), 8), np.float32)
    axis[:, 3] = 1.0
    for i, (o, d) in enumerate(HAND_AXIS):
        axis[6 * i:6 * i + 6, :3], axis[6 * i:6 * i + 6, 4:7] = o, d
    rays.append(axis)
    chains += ch.rays(axis)
    parts.append(Part("hand", HAND_LEVEL, sph, np.concatenate(rays), chains))
    # two hard scenes
    for sc in HS.scenes(oracle_mod.SPHERE_DTYPE):
        if sc.name not in HARD:
            continue
        sc = sc._replace(spheres=HC.mark_spheres(sc.spheres))
        O = oracle_mod.Oracle()
        HS.load_oracle(O, sc)
        rng = np.random.default_rng(2100 + len(sc.name))
        pick = rng.choice(sc.w * sc.h, HARD_PIXELS, replace=False)
        xy = np.stack([pick % sc.w, pick // sc.w], 1).astype(np.int32)
        parts.append(Part(sc.name, sc.level, sc.spheres, pwnfps_amd.pixel_rays(sc.w, sc.h, sc.cam, xy)[0], Chains(O).pixels(sc.w, sc.h, sc.cam, xy)))
    _corpus["v"] = parts
    return parts


HOSTILE = (-1.0, float("nan"), 0.0, float("inf"), -0.25, -0.0)


def reaches(part_index, part):
    """the nine batches of a part: REACHES, one value for every ray each; one seeded random reach per ray; the hostile values in turn;
    and reaches that lie EXACTLY on a distance of the ray's own chain -- the D it returns, or the cdist a step of it ends on (== is not
    exceeded, D == reach is within reach)"""
    n = len(part.rays)
    rng = np.random.default_rng(77 + part_index)
    rnd = (rng.uniform(0.0, 1.0, n) ** 2 * 12.0).astype(F)
    exact = np.zeros(n, F)
    for i, c in enumerate(part.chains):
        K = len(c.cdist)
        if i % 2 == 0 and c.ev != HC.NONE:
            exact[i] = c.dist
        elif K > 1:
            exact[i] = c.cdist[1 + (i // 2) % min(3, K - 1)]
    return [np.full(n, r, F) for r in REACHES] + [rnd, np.resize(np.array(HOSTILE, F), n), exact]


def load_renderer(r, part):
    import hard_scenes as HS
    (r.level_load if HS.is_path(part.level) else r.level_load_text)(part.level)
    r.set_objects(part.spheres)
