"""What tests/test_baked_cells.py (CPU) and tests/test_gpu_baked_cells.py share: a literal Python restatement of the
tests the reference makes on a cell that holds a portal letter (trace.h:404-413, 508-559), random levels with the
hostile cases among them, and a dozen hand-made levels around a 2-high hall whose walls are portal letters.

A level here is (data, pmap): data (64, 64) uint8 as lv->data[z][x], pmap (26, 7) int32 rows x1 z1 x2 z2 rot12 c1 c2
(defs.h:87-94) -- what pwn_upload_level, the oracle's and the reference harness's set_level take.  The portal tables
are made by hand, not by a loader, so that they can say what no level file says.
"""
from collections import namedtuple

import numpy as np

LT2, LTDQ = 1, 2                      # cell_bake.h: PWN_C_LT2, PWN_C_LTDQ
PST_WALL, PST_MAGENTA, PST_REC0 = 0, 1, 2


# ---- the reference's tests, literally ----------------------------------------------------------------------------

def get_cell(data, cx, cz):
    """util.h:151-158: a coordinate outside [0, 64) reads index 0 on that axis"""
    if cx < 0 or cx >= 64:
        cx = 0
    if cz < 0 or cz >= 64:
        cz = 0
    return int(data[cz, cx])


def look_through(data, pmap, cx, cz):
    """trace.h:404-413: what a ray that leaves a 2-high room sees in cell (cx, cz): (carries on, is a '"'-cell)"""
    xcell = get_cell(data, cx, cz)
    if ord('A') <= xcell <= ord('Z'):
        x1, z1, x2, z2, rot12, c1, c2 = (int(v) for v in pmap[xcell - ord('A')])
        if x1 == cx and z1 == cz:
            xcell = c2
        elif x2 == cx and z2 == cz:
            xcell = c1
    return (xcell == ord('#') or xcell == ord('&')), xcell == ord('"')


def portal_step(data, pmap, cx, cz):
    """trace.h:508-559 for a ray standing in the letter cell (cx, cz): "wall", "magenta", or
    ("go", destination x, z, what is added to pos.x, to pos.z, rot)"""
    cell = get_cell(data, cx, cz)
    x1, z1, x2, z2, rot12, c1, c2 = (int(v) for v in pmap[cell - ord('A')])
    if x2 == -1:
        return "wall"
    if x1 == cx and z1 == cz:
        return ("go", x2, z2, np.float32(x2 - x1), np.float32(z2 - z1), (-rot12) & 3)
    if x2 == cx and z2 == cz:
        return ("go", x1, z1, -np.float32(x2 - x1), -np.float32(z2 - z1), rot12 & 3)
    return "magenta"


# Row / column 64 of the table stand for every coordinate outside the grid on that axis: -1 among them, the one outside
# coordinate that a portal table can hold (its "no endpoint").  The reference compares it with the ray's cell like any other.
OUTSIDE = (-1, 64, 65, 1000, 16383, -2, -37, -16384)


def table_is_taken(data, pmap):
    """Which tables pwn_upload_level has to take, derived from the reference's tests and not from the library's rule: the
    coordinates lie in -1 .. 63 (the API's range), and every entry of row / column 64 has ONE answer whichever cell
    outside the grid reads it -- then a table entry can hold it.  (Cells further out than -1 match no endpoint, so
    that one answer is the non-endpoint's, which the bake writes.)"""
    if not ((pmap[:, :4] >= -1) & (pmap[:, :4] <= 63)).all():
        return False
    for u in range(65):
        for ux, uz in ((64, u), (u, 64)):
            try:
                expected_cell(data, pmap, ux, uz)
            except AssertionError:
                return False
    return True


def expected_cell(data, pmap, ux, uz):
    """the (look-through bits, portal step or None) the reference's tests allow for table entry (ux, uz):
    ONE answer, asserted to be the same for all coordinates that read the entry"""
    answers = set()
    for cx in ([ux] if ux < 64 else OUTSIDE):
        for cz in ([uz] if uz < 64 else OUTSIDE):
            on, dq = look_through(data, pmap, cx, cz)
            low = (LT2 if on else 0) | (LTDQ if dq else 0)
            cell = get_cell(data, cx, cz)
            step = portal_step(data, pmap, cx, cz) if ord('A') <= cell <= ord('Z') else None
            answers.add((low, step))
    assert len(answers) == 1, (ux, uz, answers)
    return answers.pop()


# ---- levels ------------------------------------------------------------------------------------------------------

PLAIN = list(';;;;;;$$##&&""<>,^....')


def empty_pmap():
    pm = np.zeros((26, 7), np.int32)
    pm[:, :4] = -1
    pm[:, 5:] = ord(';')
    return pm


def as_level_load_leaves_it(pmap, stale=None):
    """level_new sets x1, x2, c1 and c2 only (level.h:94-99): the z of an endpoint never seen is 0 in a fresh process, or
    what the level loaded before left there (`stale`: 26 x 2 values)"""
    pm = pmap.copy()
    for i in range(26):
        if pm[i, 0] == -1:
            pm[i, 1] = 0 if stale is None else stale[i][0]
        if pm[i, 2] == -1:
            pm[i, 3] = 0 if stale is None else stale[i][1]
            pm[i, 4] = 0 if stale is None else stale[i][0] & 3        # (rot12 is not set either)
    return pm


def random_level(rng, kind):
    """a random grid with letters and a hand-made portal table; `kind` cycles through the hostile cases.  Every fourth
    level has -1 in the table where no loader puts it, and letters in row 0 / column 0 for it to matter: most of those
    pwn_check_portals refuses"""
    data = np.array([[ord(rng.choice(PLAIN)) for _ in range(64)] for _ in range(64)], np.uint8)
    pm = empty_pmap()
    far = [ord(c) for c in '#&";$.>A']
    nlet = int(rng.integers(3, 27))
    for li in rng.permutation(26)[:nlet]:
        ch = ord('A') + int(li)
        lo = 0 if kind % 3 == 0 else 1                       # endpoints in row 0 and column 0 as well
        x1, z1, x2, z2 = (int(v) for v in rng.integers(lo, 64, 4))
        if kind % 5 == 1 and rng.random() < 0.5:
            x1 = 0
        if kind % 5 == 2 and rng.random() < 0.5:
            z2 = 0
        mode = int(rng.integers(0, 6))
        data[z1, x1] = ch
        if mode == 0:                                        # unpaired, the far side set all the same
            x2 = z2 = -1
        elif mode == 1:                                      # both endpoints in one cell
            x2, z2 = x1, z1
        else:
            data[z2, x2] = ch
        if mode == 2:                                        # the letter in a third (and fourth) cell
            for _ in range(2):
                data[int(rng.integers(0, 64)), int(rng.integers(0, 64))] = ch
        if mode == 3:                                        # an endpoint whose cell holds something else
            data[z1, x1] = ord(rng.choice(PLAIN))
        if kind % 4 == 3 and rng.random() < 0.3:
            # -1 in one half of an endpoint, an absent endpoint 1 in front of a present endpoint 2, a letter in cell (0, 0) whose
            # absent endpoint has something behind it: with the letter in the cell that the clamp reads for that coordinate
            what = int(rng.integers(0, 4))
            if what == 0:
                x1 = -1; data[z1, 0] = ch
            elif what == 1:
                z2 = -1; data[0, max(x2, 0)] = ch
            elif what == 2:
                x1 = z1 = -1; data[0, 0] = ch
            else:
                x2 = z2 = -1; data[0, 0] = ch
        if x2 == -1 and kind % 2 == 1:
            z2 = int(rng.integers(0, 64)) if rng.random() < 0.7 else 0      # as level_load leaves it: 0 or stale
            if rng.random() < 0.3:
                data[z2, 0] = ch                                          # ... with the letter in the cell that (-1, z2) reads
        pm[li] = (x1, z1, x2, z2, int(rng.integers(-3, 8)), int(rng.choice(far)), int(rng.choice(far)))
    if kind % 2 == 1:
        pm[pm[:, 0] == -1, 1] = int(rng.integers(0, 64))                  # letters never seen: (-1, z, -1, z)
        pm[(pm[:, 0] == -1), 3] = int(rng.integers(0, 64))
    # 2-high rooms next to letters
    for z in range(64):
        for x in range(63):
            if ord('A') <= data[z, x] <= ord('Z') and not ord('A') <= data[z, x + 1] <= ord('Z') and rng.random() < 0.5:
                data[z, x + 1] = ord(rng.choice(list('#&')))
    # a later letter may have overwritten an earlier one's cell: that is one more hostile case, kept
    return data, pm


Scene = namedtuple("Scene", "name data pmap cam sec spheres")
W, H = 128, 64


def _cam(x, y, z, ang_y=0.0, ang_x=0.0):
    cy, sy, cx, sx = np.cos(ang_y), np.sin(ang_y), np.cos(ang_x), np.sin(ang_x)
    cam = np.eye(4, dtype=np.float32)
    cam[:3, :3] = (np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])).astype(np.float32)
    cam[3, :3] = (x, y, z)
    return cam


def _grid(rows, x0=0, z0=0):
    data = np.full((64, 64), ord('.'), np.uint8)
    for z, row in enumerate(rows):
        for x, c in enumerate(row):
            data[z0 + z, x0 + x] = ord(c)
    return data


# A 2-high hall (columns 2..13, rows 2..11; its lower rows are fogged '&').  Its east wall, column 14, is made of
# letters: first endpoints.  The second endpoints stand in column 20 and open to the east onto rooms of every kind.
_HALL = [
    "................................",
    "................................",
    "..############A.....A######.....",
    "..############B.....B&&&&&&.....",
    "..############C.....C\"\"\"\"\"\".....",
    "..############D.....D;;;;;;.....",
    "..############E.....E$$$$$$.....",
    "..&&&&&&&&&&&&F.....F>>;;;;.....",
    "..&&&&&&&&&&&&G.....G...........",
    "..&&&&&&&&&&&&H.................",
    "..&&&&&&&&&&&&A.................",
    "..&&&&&&&&&&&&C.................",
    "................................",
]


def _hall():
    data = _grid(_HALL)
    pm = empty_pmap()
    far = '#&";$>.'
    for i, ch in enumerate("ABCDEFG"):
        # endpoint 1 opens west onto the hall, endpoint 2 east: rot12 = (d2 - d1 + 2) & 3 = 0 (level.h:194-221)
        pm[ord(ch) - 65] = (14, 2 + i, 20, 2 + i, 0, data[2 + i, 13], ord(far[i]))
    pm[ord('H') - 65] = (14, 9, -1, -1, 0, ord(';'), ord(';'))
    return data, pm


def scenes(sphere_dtype):
    """the hand-made levels: name, level, camera, spheres"""
    rng = np.random.default_rng(2718)

    def spheres(n, x, z):
        s = np.zeros(n, sphere_dtype)
        for i in range(n):
            s[i] = (rng.uniform(0.05, 0.3), rng.choice([0.0, 0.5]), x + rng.uniform(-2, 2), rng.uniform(0.2, 1.8),
                    z + rng.uniform(-2, 2), *rng.uniform(0, 1, 3))
        return s

    east_hi = _cam(8.4, 1.45, 6.6, np.pi / 2, 0.05)
    east_lo = _cam(9.3, 0.5, 7.4, np.pi / 2 - 0.2, 0.45)
    out = []
    data, pm = _hall()
    out.append(Scene("hall_upper", data, pm, east_hi, 0.5, spheres(6, 10, 6)))
    out.append(Scene("hall_lower_looking_up", data, pm, east_lo, 1.5, spheres(0, 0, 0)))
    # from the far side back into the hall: endpoint 2 looks through at c1
    out.append(Scene("far_side_back", data, pm, _cam(24.5, 1.3, 3.4, -np.pi / 2, 0.1), 0.0, spheres(3, 23, 3)))
    # every rotation, also values outside 0..3
    for rots in ((1, 2, 3, 5, -1, -2, 7), (3, 3, 2, 2, 1, 1, 6)):
        p2 = pm.copy()
        p2[:7, 4] = rots
        out.append(Scene("rotations_%d" % rots[0], data, p2, east_hi, 0.25, spheres(4, 10, 6)))
    # both endpoints in one cell (endpoint 1 wins), with a quarter turn and a half turn
    p2 = pm.copy()
    for li, rot in ((0, 1), (1, 2), (5, 3), (6, 0)):
        p2[li, 2:4] = p2[li, 0:2]
        p2[li, 4] = rot
    out.append(Scene("both_endpoints_one_cell", data, p2, east_hi, 0.0, spheres(2, 10, 6)))
    # an unpaired letter whose table says what is behind it: looked through all the same, then a wall
    for c2 in '#"':
        p2 = pm.copy()
        p2[7, 6] = ord(c2)
        p2[7, 5] = ord('&')
        for li in (2, 4):
            p2[li, 2:4] = -1
            p2[li, 6] = ord(c2)
        out.append(Scene("unpaired_far_%s" % ("hash" if c2 == '#' else "dq"), data, p2, east_lo, 0.75, spheres(3, 10, 8)))
    # far sides swapped around by hand: '"' behind the fogged rows, solid and a letter behind the plain ones
    p2 = pm.copy()
    p2[:7, 6] = [ord(c) for c in '"&#.Q"#']
    p2[:7, 5] = [ord(c) for c in '";.&#;"']
    out.append(Scene("far_sides_by_hand", data, p2, east_hi, 2.0, spheres(5, 10, 6)))
    # endpoints in row 0 and column 0 of a level without walls at the border: the rays that leave the grid read
    # the copies of those cells and must meet a magenta wall there, not a portal
    rows = [list("#" * 64) for _ in range(64)]
    for z in range(64):
        for x in range(64):
            if (x * 7 + z * 3) % 11 == 0:
                rows[z][x] = '&'
            if 20 <= x < 30 and 20 <= z < 30:
                rows[z][x] = ';"$'[(x + z) % 3]
    for (x, z), ch in (((0, 5), 'A'), ((9, 0), 'A'), ((0, 0), 'B'), ((40, 40), 'B'), ((0, 33), 'C'), ((63, 12), 'D'), ((12, 63), 'D'),
                       ((0, 50), 'E')):
        rows[z][x] = ch
    data2 = _grid(["".join(r) for r in rows])
    p3 = empty_pmap()
    p3[0] = (0, 5, 9, 0, 1, ord('#'), ord('&'))
    p3[1] = (0, 0, 40, 40, 2, ord('"'), ord('#'))
    p3[2] = (0, 33, -1, -1, 0, ord('#'), ord('#'))
    p3[3] = (63, 12, 12, 63, 3, ord('&'), ord('"'))
    p3[4] = (0, 50, 0, 50, 1, ord('#'), ord('#'))
    out.append(Scene("border_from_outside", data2, p3, _cam(-4.5, 1.4, 70.25, 2.4, 0.02), 0.5, spheres(0, 0, 0)))
    out.append(Scene("border_from_inside", data2, p3, _cam(2.5, 1.5, 3.5, 4.0, 0.0), 0.5, spheres(4, 3, 3)))
    out.append(Scene("border_far_outside", data2, p3, _cam(80.5, 0.6, -9.5, -0.8, 0.1), 1.0, spheres(0, 0, 0)))
    # cell (-1, -1) reads cell (0, 0) and matches an absent endpoint: an unpaired letter there, seen from outside that corner.
    # On its endpoint 1, cell (0, 0), the reference looks through at c2; from (-1, -1) through the absent endpoint 2 at c1
    rows3 = [list(r) for r in rows]
    rows3[0][0] = 'F'
    data3 = _grid(["".join(r) for r in rows3])
    p4 = p3.copy()
    p4[5] = (0, 0, -1, -1, 2, ord(';'), ord('#'))
    out.append(Scene("corner_minus_one", data3, p4, _cam(-3.5, 1.45, -3.25, 0.7, 0.03), 0.5, spheres(0, 0, 0)))
    out.append(Scene("corner_minus_one_from_inside", data3, p4, _cam(1.5, 1.5, 1.5, 0.7 + np.pi, 0.0), 0.5, spheres(2, 2, 2)))
    assert len(out) >= 12
    return out


def refused_tables():
    """portal tables that pwn_upload_level refuses (pwn_check_portals): on each of them some cell outside the grid, at
    coordinate -1, IS an endpoint for the reference -- name, data, pmap"""
    out = []
    data = _grid(["#" * 64] * 64)
    data[5, 0] = data[10, 10] = ord('A')
    pm = empty_pmap()
    pm[0] = (-1, 5, 10, 10, 1, ord('#'), ord('#'))           # a ray in cell (-1, 5) stands on endpoint 1
    out.append(("endpoint_1_at_x_minus_one", data, pm))
    data = _grid(["#" * 64] * 64)
    data[7, 7] = data[0, 9] = ord('B')
    pm = empty_pmap()
    pm[1] = (7, 7, 9, -1, 0, ord('#'), ord('#'))             # ... in cell (9, -1) on endpoint 2
    out.append(("endpoint_2_at_z_minus_one", data, pm))
    data = _grid(["#" * 64] * 64)
    data[0, 0] = data[20, 20] = ord('C')
    pm = empty_pmap()
    pm[2] = (-1, -1, 20, 20, 3, ord('#'), ord('#'))          # endpoint 1 absent, endpoint 2 present: cell (-1, -1) goes to (20, 20)
    out.append(("absent_endpoint_1_of_a_pair", data, pm))
    data = _grid(["#" * 64] * 64)
    data[0, 0] = ord('D')
    pm = empty_pmap()
    pm[3] = (0, 0, -1, -1, 0, ord('&'), ord(';'))            # unpaired letter in cell (0, 0): from (-1, -1) looked through at c1
    out.append(("far_side_behind_an_absent_endpoint_2", data, pm))
    pm = empty_pmap()
    pm[3] = (-1, -1, -1, -1, 0, ord(';'), ord('"'))          # ... and through an absent endpoint 1 at c2
    out.append(("far_side_behind_an_absent_endpoint_1", data, pm))
    data = _grid(["#" * 64] * 64)
    data[3, 3] = data[7, 0] = ord('E')
    pm = empty_pmap()
    pm[4] = (3, 3, -1, 7, 0, ord('#'), ord(';'))             # no endpoint 2, a z left beside it: from (-1, 7) looked through at c1
    out.append(("far_side_behind_an_absent_endpoint_with_a_z", data, pm))
    pm = empty_pmap()
    pm[25] = (3, 3, 64, 2, 0, ord(';'), ord(';'))
    out.append(("coordinate_out_of_range", data, pm))
    return out
