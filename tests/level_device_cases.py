"""What the tests of pwn_upload_level_device share: the corpus of levels (tests/baked_scenes.py's hostile random levels and refused
tables, the shipped levels, the hand-made level of tests/players_model.py), hand-made grids for the derived table, the hostile
coordinates and bytes, and level_host.c's pwn_parse_level restated in Python for the shipped levels' cells.

A level is (name, data, pmap): data (64, 64) uint8 as lv->data[z][x], pmap (26, 7) int32 or None (the table is derived)."""
import os

import numpy as np

import baked_scenes as bs
from conftest import GOLD

SEED, NKINDS = 20261021, 48
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def parse_level(text):
    """pwn_parse_level (level_host.c; level.h:107-228): (data, pmap) of a level text"""
    if isinstance(text, str):
        text = text.encode("latin-1")
    data = np.full((64, 64), ord('.'), np.uint8)
    pm = bs.empty_pmap()
    flat = data.reshape(-1)

    def endpoint(i, x, z):
        if pm[i, 0] == -1:
            pm[i, 0:2] = (x, z)
        elif pm[i, 2] == -1:
            pm[i, 2:4] = (x, z)
    x = z = 0
    for c in text:
        if z >= 64:
            break
        if c in (13, 10):
            if x != 0:
                x, z = 0, z + 1
            continue
        if c == ord('*'):
            c = ord(';')
        if ord('a') <= c < ord('z'):
            endpoint(c - ord('a'), x, z)
            c = c - ord('a') + ord('A') + 1
        if ord('A') <= c <= ord('Z'):
            endpoint(c - ord('A'), x, z)
        data[z, x] = c
        x += 1
        if x == 64:
            x, z = 0, z + 1
    opens = set(b';$"#&><^,')
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))

    def cell(x, z):
        i = z * 64 + x
        return int(flat[i]) if 0 <= i < 4096 else ord('.')

    def open_dir(x, z):
        for d, (dx, dz) in enumerate(dirs):
            if cell(x + dx, z + dz) in opens:
                return d
        return 0
    for i in range(26):
        x1, z1, x2, z2 = (int(v) for v in pm[i, :4])
        if x2 == -1:
            continue
        d1, d2 = open_dir(x1, z1), open_dir(x2, z2)
        pm[i, 4] = (d2 - d1 + 2) & 3
        pm[i, 5] = cell(x1 + dirs[d1][0], z1 + dirs[d1][1])
        pm[i, 6] = cell(x2 + dirs[d2][0], z2 + dirs[d2][1])
    return data, pm


def shipped_levels():
    """the three shipped levels and players_model's hand-made one, parsed: (name, data, pmap)"""
    from players_model import HAND_LEVEL
    out = []
    for name in ("pwnfps_level", "synth64", "synth256"):
        with open(os.path.join(GOLD, "levels", name + ".txt"), "rb") as f:
            out.append((name,) + parse_level(f.read()))
    out.append(("players_hand_level",) + parse_level(HAND_LEVEL))
    return out


def random_levels():
    """the 48 hostile random levels: (name, data, pmap, taken) -- 37 taken and 11 refused tables"""
    rng = np.random.default_rng(SEED)
    out = []
    for kind in range(NKINDS):
        data, pm = bs.random_level(rng, kind)
        out.append(("random_%02d" % kind, data, pm, bs.table_is_taken(data, pm)))
    return out


def both_kinds_occur(levels):
    """neither side of the corpus can go untested"""
    taken = sum(1 for lv in levels if lv[3])
    assert taken >= 24 and len(levels) - taken >= 8, (taken, len(levels))


def refused_tables():
    return [(name, data, pm) for name, data, pm in bs.refused_tables()]


def _grid(fill='.'):
    return np.full((64, 64), ord(fill), np.uint8)


def derived_grids():
    """hand-made grids for the derived table: (name, data)"""
    g = _grid()
    # the aliasing neighbour read: a letter in column 63 and in column 0 of the next row -- each is the other's +x / -x neighbour;
    # B in column 63 whose only open neighbour is column 0 of the next row
    g[5, 63] = g[6, 0] = ord('A')
    g[10, 63] = g[20, 20] = ord('B')
    g[11, 0] = ord(';')
    g[21, 20] = ord('$')
    # a letter in cell 4095: its +x and +z neighbours lie outside the array
    g[63, 63] = g[30, 30] = ord('C')
    g[63, 62] = ord('#')
    g[30, 29] = ord('"')
    # three and four sightings of one letter
    for x, z in ((3, 40), (9, 40), (3, 44)):
        g[z, x] = ord('D')
        g[z + 1, x] = ord('&')
    for x, z in ((40, 3), (44, 3), (40, 9), (44, 9)):
        g[z, x] = ord('E')
        g[z, x - 1] = ord('>')
    # a letter with no open neighbour, and one seen once
    g[50, 50] = g[55, 55] = ord('F')
    g[58, 8] = ord('G')
    g[58, 9] = ord(';')
    out = [("aliasing_4095_sightings", g)]
    h = _grid()
    # cell 0: its -x and -z neighbours lie in front of the array; Z and the neighbours of every kind
    h[0, 0] = h[0, 2] = ord('H')
    h[1, 0] = ord(',')
    h[0, 3] = ord('^')
    h[33, 33] = h[33, 35] = ord('Z')
    h[33, 34] = ord('<')
    h[20, 10] = h[20, 11] = ord('Q')          # each other's neighbour, nothing open
    h[21, 10] = ord(';')                       # ... but +z of the first
    out.append(("cell_0_and_pairs", h))
    return out


def hostile_coordinate_tables():
    """tables with a coordinate far out of range: (name, data, pmap), all verdict 1"""
    out = []
    for name, v in (("int_min", INT_MIN), ("int_max", INT_MAX), ("sixty_four", 64), ("minus_two", -2)):
        for col in range(4):
            data = _grid('#')
            data[7, 7] = data[9, 9] = ord('K')
            pm = bs.empty_pmap()
            pm[10] = (7, 7, 9, 9, 1, ord('#'), ord(';'))
            pm[10, col] = v
            out.append(("%s_in_column_%d" % (name, col), data, pm))
    # every coordinate of every letter hostile at once, differences that overflow
    data = _grid(';')
    data[0, :26] = np.arange(26) + ord('A')
    pm = bs.empty_pmap()
    pm[:, 0], pm[:, 1], pm[:, 2], pm[:, 3] = INT_MIN, INT_MAX, INT_MAX, INT_MIN
    pm[:, 4] = INT_MIN
    pm[:, 5:] = INT_MAX
    out.append(("all_hostile", data, pm))
    return out


def all_bytes_grid():
    """a grid of all 256 byte values, each sixteen times, letters and line ends among them"""
    return (np.arange(4096, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(64, 64)


def derive_table(data):
    """the table pwn_upload_level_device derives from the cells as stored: the parser's rules on upper-case letters alone"""
    flat = np.ascontiguousarray(data, np.uint8).reshape(-1)
    pm = bs.empty_pmap()
    for i in np.flatnonzero((flat >= ord('A')) & (flat <= ord('Z'))):
        row = pm[int(flat[i]) - ord('A')]
        if row[0] == -1:
            row[0:2] = (i & 63, i >> 6)
        elif row[2] == -1:
            row[2:4] = (i & 63, i >> 6)
    opens = set(b';$"#&><^,')
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))

    def cell(x, z):
        i = z * 64 + x
        return int(flat[i]) if 0 <= i < 4096 else ord('.')
    for row in pm:
        if row[2] == -1:
            continue
        d = []
        for x, z in ((int(row[0]), int(row[1])), (int(row[2]), int(row[3]))):
            d.append(next((k for k, (dx, dz) in enumerate(dirs) if cell(x + dx, z + dz) in opens), 0))
        row[4] = (d[1] - d[0] + 2) & 3
        row[5] = cell(int(row[0]) + dirs[d[0]][0], int(row[1]) + dirs[d[0]][1])
        row[6] = cell(int(row[2]) + dirs[d[1]][0], int(row[3]) + dirs[d[1]][1])
    return pm


def expected_verdict(data, pmap):
    """(verdict, letter) of pwn_level_device_state for a given table: level_host.c's pwn_check_portals with the lowest offending
    letter of the rule that decides -- 1: a coordinate outside -1 .. 63; 2: a cell outside the grid at coordinate -1 that is an endpoint
    for the reference and sees or does something there; (0, 26): taken"""
    pm = np.asarray(pmap, np.int64)
    bad = np.flatnonzero(((pm[:, :4] < -1) | (pm[:, :4] > 63)).any(axis=1))
    if len(bad):
        return 1, int(bad[0])

    def look(c):
        return (c & 0xff) in (ord('#'), ord('&'), ord('"'))
    letters = []
    for t in range(-1, 64):
        for cx, cz in ((-1, t), (t, -1)):
            c = int(data[max(cz, 0), max(cx, 0)])
            if not ord('A') <= c <= ord('Z'):
                continue
            x1, z1, x2, z2, _, c1, c2 = (int(v) for v in pm[c - ord('A')])
            at1, at2 = (x1, z1) == (cx, cz), (x2, z2) == (cx, cz)
            differs = look(c2) if at1 else (look(c1) if at2 else False)
            if differs or (x2 != -1 and (at1 or at2)):
                letters.append(c - ord('A'))
    return (2, min(letters)) if letters else (0, 26)
