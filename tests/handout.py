"""What the hand-out tests share (tests/test_gpu_handout.py, tests/test_handout_walk.py): a camera that never stands still, poison
for planes of the caller's, and the oracle's frames of both, computed once.

A launch that skips a 16 x 4 unit leaves in the planes what was there before.  Two things make that visible:

  poison   where the caller owns the planes, every launch gets planes filled with POISON_S / POISON_Z; the oracle traces the same
           rows with the poison as entry depth, so a ray that runs out of steps keeps it on both sides;
  the walk where the library owns the planes, frame k of a sequence has its own camera and time (walk()), chosen so that no unit of
           a frame keeps the colour AND the depth bits of the frame its planes held before: hidden_units(prev, cur) == 0, which
           every test asserts from the oracle's frames alone before it looks at the GPU's.

The judge is always the oracle (tests/oracle.py), never the library.
"""
import numpy as np

from conftest import level_path, load_spheres

POISON_S, POISON_Z = 0x5a5a5a5a, 0x7fc12345
LEVELS = {"pwnfps_level": "t0", "synth64": "synth64", "synth256": "synth256"}
FRAMES = 8          # launches per sequence: more than the 6 ticket sets (PWN_TICKET_SETS) and than the 2R = 4 in use at R = 2

_scenes = {}
_rows = {}
_chains = {}


def scene(level="pwnfps_level"):
    """(oracle, level file, spheres, spawn cell) of a level with its own spheres, loaded once"""
    if level not in _scenes:
        import oracle
        oracle.build()
        O = oracle.Oracle()
        path = level_path(level)
        sph = load_spheres(LEVELS[level])
        O.load_level(path)
        O.set_spheres(sph)
        _, _, spawn = O.get_level()
        _scenes[level] = (O, path, sph, spawn)
    return _scenes[level]


def walk(level, k):
    """(camera, time) of frame k of a sequence: the spawn cell's centre, turned further and pitched differently every frame"""
    import pwnfps_amd
    spawn = scene(level)[3]
    return pwnfps_amd.spawn_camera(spawn, ang_y=0.6 + 0.37 * k, ang_x=-0.25 + 0.05 * (k % 3)), 1.25 + 0.5 * k


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def units_of(h, w):
    return ((w + 15) // 16) * ((h + 3) // 4)


def hidden_units(prev, cur):
    """16 x 4 units (counted from the planes' corner) all of whose pixels have the same colour AND the same depth bits in prev and
    cur, each a pair (colour, depth) of equal shape: the units a launch could skip without a pixel test seeing it"""
    same = (bits(prev[0]) == bits(cur[0])) & (bits(prev[1]) == bits(cur[1]))
    h, w = same.shape
    pad = np.ones(((h + 3) // 4 * 4, (w + 15) // 16 * 16), bool)
    pad[:h, :w] = same
    return int(pad.reshape(pad.shape[0] // 4, 4, pad.shape[1] // 16, 16).all(axis=(1, 3)).sum())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def poisoned_rows(level, w, h, k, y0, y1):
    """the oracle's rows [y0, y1) of the walk's frame k on planes that held the poison: (colour rows, depth rows as uint32, the five
    counters).  Asserts that no colour of those rows is the poison word, so a row that kept it was not traced."""
    import hard_scenes as HS
    key = (level, w, h, k, y0, y1)
    if key not in _rows:
        O = scene(level)[0]
        cam, sec = walk(level, k)
        zb = np.full((h, w), POISON_Z, np.uint32).view(np.float32)
        sb = np.full((h, w), POISON_S, np.uint32)
        sb, zb, st = O.trace_rows(w, h, y0, y1, cam, sec=np.float32(sec), sb=sb, zb=zb)
        zu = bits(zb)
        assert (sb[:y0] == POISON_S).all() and (sb[y1:] == POISON_S).all() and (zu[:y0] == POISON_Z).all() and (zu[y1:] == POISON_Z).all()
        assert not (sb[y0:y1] == POISON_S).any(), key
        _rows[key] = _frozen(sb[y0:y1].copy(), zu[y0:y1].copy()) + (HS.stats5(st),)
    return _rows[key]


def chain(level, w, h, ks):
    """the oracle's frames of ONE persistent depth plane of w x h that starts from zero and is shown the walk's frames ks in that
    order (hard_scenes.Plane: a ray that runs out of steps keeps the depth of the frame before).  A list of (pre-blur colour,
    depth as float32, blurred colour or None where w % 4 != 0); prefixes are shared."""
    ks = tuple(ks)
    key = (level, w, h)
    have = _chains.setdefault(key, {})
    if ks not in have:
        O = scene(level)[0]
        before = chain(level, w, h, ks[:-1]) if len(ks) > 1 else []
        z = before[-1][1].copy() if before else np.zeros((h, w), np.float32)
        cam, sec = walk(level, ks[-1])
        sb, z, _ = O.trace_rows(w, h, 0, h, cam, sec=np.float32(sec), zb=z)
        post = O.blur_rows(0, h, sb, z) if w % 4 == 0 else None
        have[ks] = before + [_frozen(sb, z) + (None if post is None else _frozen(post)[0],)]
    return have[ks]


def assert_walk_hides_nothing(level, w, h, ks):
    """the precondition of every test that relies on the walk: on a plane that is shown frames ks, from zero, no unit of any frame
    keeps the colour and the depth of the frame before (the first frame's before: the zeros of a fresh plane)"""
    frames = chain(level, w, h, ks)
    prev = (np.zeros((h, w), np.uint32), np.zeros((h, w), np.float32))
    for k, fr in zip(ks, frames):
        n = hidden_units(prev, fr[:2])
        assert n == 0, (level, w, h, ks, k, n)
        prev = fr[:2]
    return frames


class Shown:
    """The oracle's side of one persistent depth plane that is shown cameras of the caller's choosing, the walk's among them
    (hard_scenes.Plane, with the walk's precondition): show() asserts that no unit of the new frame keeps colour and depth of the
    frame the plane held, unless the caller says that it is the same frame again."""

    def __init__(self, O, w, h):
        self.O, self.w, self.h = O, w, h
        self.held = (np.zeros((h, w), np.uint32), np.zeros((h, w), np.float32))

    def show(self, cam, sec, blur, again=False):
        """(colour -- blurred where blur is set --, depth) of the next frame on this plane"""
        sb, z, _ = self.O.trace_rows(self.w, self.h, 0, self.h, cam, sec=np.float32(sec), zb=self.held[1].copy())
        n = hidden_units(self.held, (sb, z))
        assert again or n == 0, (self.w, self.h, float(sec), n)
        self.held = (sb, z)
        return (self.O.blur_rows(0, self.h, sb, z) if blur else sb), z


def same(what, sb, zb, want_sb, want_z):
    bad = bits(sb) != bits(want_sb)
    assert not bad.any(), (what, "colour", int(bad.sum()), np.argwhere(bad)[:4].tolist())
    bad = bits(zb) != bits(want_z)
    assert not bad.any(), (what, "depth", int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- the planes the library owns: which frames of the walk each persistent depth plane is shown, test by test ----
# (tests/test_gpu_handout.py renders them, tests/test_handout_walk.py asserts the precondition on the CPU alone)

LEVEL = "pwnfps_level"
# (every shape has more units than the 1 024 waves of one workgroup per CU, so that with that grid tickets are drawn, not only the
# waves' static first ones: a launch with fewer items than resident waves hands every item out as a static ticket)
BLOCKING = (1000, 260)         # the blocking call in one launch per pass, and the group of three
STRIPPED = (1000, 520)         # the blocking call in four strips of 160, 160, 160 and 40 rows
IN_FLIGHT = (2080, 36)         # three slots on two streams: 1 170 units, enough for an order to be sorted
VIEWS = (336, 208)             # three view slots, 1 092 units each
# layout L1 of tests/test_gpu_viewports.py
VIEWPORTS = (336, 208, [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
                        (100, 138, 36, 70), (140, 100, 196, 108)])
MIXED_CYCLE = 6                # launches of one cycle of the mixed sequence, which runs twice


def library_planes():
    """{test: [(level, w, h, frames of the walk the plane is shown, in order)]}"""
    W, Hh, rects = VIEWPORTS
    return {
        "blocking": [(LEVEL,) + BLOCKING + (tuple(range(FRAMES)),)],
        "stripped": [(LEVEL,) + STRIPPED + (tuple(range(FRAMES)),)],
        "in_flight": [(LEVEL,) + IN_FLIGHT + (tuple(range(s, FRAMES, 3)),) for s in range(3)],
        "views": [(LEVEL,) + VIEWS + (tuple(range(s, s + FRAMES)),) for s in range(3)],
        "viewports": [(LEVEL, w, h, tuple(range(i, i + FRAMES))) for i, (_, _, w, h) in enumerate(rects)],
        # one context of W x Hh; launch n of the sequence is shown frame n of the walk (a view slot or a rectangle i: frame n + i)
        "mixed": [(LEVEL, W, Hh, (0, MIXED_CYCLE))] + [(LEVEL, W, Hh, (1 + s, 1 + s + MIXED_CYCLE)) for s in range(3)] +
                 [(LEVEL, w, h, (4 + i, 4 + i + MIXED_CYCLE)) for i, (_, _, w, h) in enumerate(rects)],
    }
