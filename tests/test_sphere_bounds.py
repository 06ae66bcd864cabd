"""The bounding balls of the longest per-cell sphere lists (pwnfps_amd/csrc/sphere_bound.h, pwn_sphere_bounds_build in
level_host.c), on the CPU: which lists pwn_sphere_bounds_plan gives a ball, that a ball holds its members with the inflation
the header derives, that the tables' sizes do not move -- and that the predicate the kernels compile never lets a wave skip a
list of which the exact test (trace.h:256-270, restated here in float32 in the reference's operation order) accepts a member:
over a million samples, zero violations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_spheres
from oracle import SPHERE_DTYPE

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
T0_CELL = 5 * 64 + 9


@pytest.fixture(scope="module")
def hip():
    lib = C.CDLL(os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so"))
    lib.pwn_sphere_bounds_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pwn_sphere_tables_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pwn_bin_spheres.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lib


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    """sphere_bound.h compiled for the CPU the way the library is: no contraction of a product and a sum"""
    so = str(tmp_path_factory.mktemp("sb") / "libsbdrv.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=gnu11", "-ffp-contract=off", "-I" + CSRC,
                           "-o", so, os.path.join(ROOT, "tests", "sphere_bound_driver.c")])
    lib = C.CDLL(so)
    lib.sb_pass_many.argtypes = [C.c_int, C.c_long] + [C.c_void_p] * 5
    lib.sb_normalise_many.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    lib.sb_const.restype = C.c_double
    lib.sb_const.argtypes = [C.c_int]
    return lib


def _consts(drv):
    return {k: drv.sb_const(i) for i, k in enumerate(("eps", "eta", "dmax", "rlimit", "minrec", "kmax", "coord"))}


def _plan(hip, s):
    s = np.ascontiguousarray(s, SPHERE_DTYPE)
    buf = s if len(s) else np.zeros(1, SPHERE_DTYPE)
    out = np.full((4, 8), -1.0)
    n = hip.pwn_sphere_bounds_plan(buf.ctypes.data, len(s), out.ctypes.data)
    assert 0 <= n <= 4, n
    assert (out[n:] == 0.0).all()
    return [dict(cell=int(o[0]), records=int(o[1]), id=int(o[2]), c=o[3:6].copy(), r_eff=float(o[6]), rr=float(o[7])) for o in out[:n]]


def _tables(hip, s):
    s = np.ascontiguousarray(s, SPHERE_DTYPE)
    buf = s if len(s) else np.zeros(1, SPHERE_DTYPE)
    out = (C.c_uint64 * 6)()
    rc = hip.pwn_sphere_tables_plan(buf.ctypes.data, len(s), out)
    return (rc,) + tuple(int(v) for v in out)


def _bins(hip, s):
    s = np.ascontiguousarray(s, SPHERE_DTYPE)
    off = np.zeros(4097, np.int32)
    n = hip.pwn_bin_spheres(s.ctypes.data, len(s), off.ctypes.data, None, 0)
    idx = np.zeros(max(n, 1), np.int32)
    assert hip.pwn_bin_spheres(s.ctypes.data, len(s), off.ctypes.data, idx.ctypes.data, n) == n
    return off, idx


def _members(hip, s, cell):
    off, idx = _bins(hip, s)
    return np.ascontiguousarray(s, SPHERE_DTYPE)[idx[off[cell]:off[cell + 1]]]


def _holds(b, m, k):
    """in float64: every member lies in the ball with the inflation of sphere_bound.h to spare; rr is the radius squared, upwards"""
    c = np.float64(b["c"])
    for q in m:
        rho = np.sqrt((q["x"] - c[0]) ** 2 + (q["y"] - c[1]) ** 2 + (q["z"] - c[2]) ** 2)
        r = abs(float(q["r"]))
        infl = np.sqrt(r * r + k["eps"] * (k["dmax"] + rho) ** 2 + k["eta"]) - r
        assert infl > 0.0 and rho + r <= b["r_eff"] - infl, (b, q, rho, infl)
    assert b["rr"] >= b["r_eff"] ** 2 and b["rr"] <= b["r_eff"] ** 2 * (1 + 1e-6)
    assert b["rr"] == np.float32(b["rr"]) and b["r_eff"] == np.float32(b["r_eff"])


def _cluster(cx, cz, n, r=0.1, spread=0.2, y=0.4, seed=0):
    """n spheres inside cell (cx, cz), none reaching into a neighbour"""
    g = np.random.default_rng(seed)
    s = np.zeros(n, SPHERE_DTYPE)
    s["x"] = cx + 0.5 + g.uniform(-spread, spread, n)
    s["z"] = cz + 0.5 + g.uniform(-spread, spread, n)
    s["y"] = y + g.uniform(-0.1, 0.1, n)
    s["r"] = r
    s["refl"] = 0.3
    s["cb"] = s["cg"] = s["cr"] = 0.7
    return s


def test_t0_one_ball(hip, drv):
    k = _consts(drv)
    s = load_spheres("t0")
    before = _tables(hip, s)
    b = _plan(hip, s)
    assert len(b) == 1 and b[0]["cell"] == T0_CELL and b[0]["records"] == 14 and b[0]["id"] == 0
    m = _members(hip, s, T0_CELL)
    assert len(m) == 14
    _holds(b[0], m, k)
    # (the tight ball has radius 0.401 here; sphere_bound.h states what the guards and fp32 cost on top)
    tight = max(np.sqrt((q["x"] - b[0]["c"][0]) ** 2 + (q["y"] - b[0]["c"][1]) ** 2 + (q["z"] - b[0]["c"][2]) ** 2) + q["r"] for q in m)
    assert tight < b[0]["r_eff"] < tight + 0.03
    assert _tables(hip, s) == before
    import pwnfps_amd
    w = pwnfps_amd.sphere_bounds_plan(s)
    assert len(w) == 1 and w[0]["cell"] == T0_CELL and w[0]["records"] == 14 and w[0]["r_eff"] == b[0]["r_eff"]


@pytest.mark.parametrize("key", ["synth64", "synth256", "none"])
def test_short_lists_get_none(hip, key):
    s = load_spheres(key)
    before = _tables(hip, s)
    assert _plan(hip, s) == []
    assert _tables(hip, s) == before


def test_ids_follow_the_form(hip, drv, monkeypatch):
    """the id is what the cell word carries: entries before the list (with end marks), records before it, non-empty cells before it"""
    s = np.concatenate([_cluster(3, 2, 2, seed=1), _cluster(7, 2, 6, seed=2), _cluster(1, 9, 5, seed=3)])
    want = {"indexed": {2 * 64 + 7: 3, 9 * 64 + 1: 10}, "inline": {2 * 64 + 7: 2, 9 * 64 + 1: 8}, "global": {2 * 64 + 7: 1, 9 * 64 + 1: 2}}
    for form, ids in want.items():
        monkeypatch.setenv("PWN_SPHERE_LISTS", form)
        assert _tables(hip, s)[1] == {"indexed": 0, "inline": 1, "global": 2}[form]
        b = _plan(hip, s)
        assert [(x["cell"], x["records"]) for x in b] == [(2 * 64 + 7, 6), (9 * 64 + 1, 5)]
        assert {x["cell"]: x["id"] for x in b} == ids, form
        for x in b:
            _holds(x, _members(hip, s, x["cell"]), _consts(drv))


def test_the_four_longest_by_the_tie_rule(hip, drv):
    cells = [(20, 3, 5), (4, 3, 7), (9, 9, 5), (30, 1, 9), (2, 40, 6), (5, 5, 5)]       # x, z, records
    s = np.concatenate([_cluster(x, z, n, seed=10 + i) for i, (x, z, n) in enumerate(cells)])
    before = _tables(hip, s)
    b = _plan(hip, s)
    # 9, 7, 6, then of the three lists of 5 the lowest cell (z * 64 + x): (20, 3)
    assert [(x["cell"], x["records"]) for x in b] == [(1 * 64 + 30, 9), (3 * 64 + 4, 7), (40 * 64 + 2, 6), (3 * 64 + 20, 5)]
    for x in b:
        _holds(x, _members(hip, s, x["cell"]), _consts(drv))
    assert _tables(hip, s) == before


@pytest.mark.parametrize("what", ["nan_x", "inf_y", "nan_y", "nan_r", "inf_r", "huge_r", "far_member", "far_out", "short"])
def test_lists_that_get_no_ball(hip, drv, what):
    k = _consts(drv)
    good = _cluster(12, 12, 6, seed=5)
    bad = _cluster(40, 20, 8, seed=6)
    if what == "nan_x":
        bad["x"][3] = np.nan           # (binned to no cell at all, level.h:27-31: the other seven make a list that may have a ball)
    elif what == "inf_y":
        bad["y"][2] = np.inf           # (y takes no part in the binning: this one is a member)
    elif what == "nan_y":
        bad["y"][5] = np.nan
    elif what == "nan_r":
        bad["r"][1] = np.nan           # (x - r is NaN: binned to no cell either)
    elif what == "inf_r":
        bad["r"][1] = np.inf           # (the same: the conversion of an infinity gives INT_MIN on both sides)
    elif what == "huge_r":
        bad["r"][0] = 1.45             # centre distance + radius beyond the limit (and it is binned to many cells)
        bad["x"][0] += 0.2
    elif what == "far_member":
        bad["y"][0] = 2.5              # in the cell's column, far above the others
    elif what == "far_out":
        bad["y"] += 2000.0
    elif what == "short":
        bad = bad[:int(k["minrec"]) - 1]
    s = np.concatenate([good, bad])
    before = _tables(hip, s)
    b = _plan(hip, s)
    off, idx = _bins(hip, s)
    for x in b:
        m = np.ascontiguousarray(s, SPHERE_DTYPE)[idx[off[x["cell"]]:off[x["cell"] + 1]]]
        assert len(m) == x["records"] >= k["minrec"]
        assert np.isfinite([m["x"], m["y"], m["z"], m["r"]]).all()
        _holds(x, m, k)
        assert x["r_eff"] < 1.75
    assert 12 * 64 + 12 in [x["cell"] for x in b]
    # (nan_x, nan_r, inf_r: the bad sphere is binned to no cell, so it is no member and the other seven may have their ball.
    # huge_r IS a member of its own cell's list, with seven small ones: rho + r is about 1.65 there, over PWN_SB_R_LIMIT)
    if what not in ("nan_x", "nan_r", "inf_r"):
        assert 20 * 64 + 40 not in [x["cell"] for x in b], what
    if what == "huge_r":
        m = _members(hip, s, 20 * 64 + 40)
        c = np.array([np.float64(m[n]).mean() for n in ("x", "y", "z")])
        reach = max(np.sqrt((q["x"] - c[0]) ** 2 + (q["y"] - c[1]) ** 2 + (q["z"] - c[2]) ** 2) + abs(float(q["r"])) for q in m)
        # the case is about the limit and nothing else: all members finite, eight of them, and the list's reach between the limit
        # and the 1.75 that the loop above lets a ball have
        assert len(m) == 8 and np.isfinite([m["x"], m["y"], m["z"], m["r"]]).all() and k["rlimit"] < reach < 1.7, reach
    assert _tables(hip, s) == before


# ---- the predicate never skips a list the exact test accepts from

def _normalise(drv, v):
    v = np.ascontiguousarray(v, np.float32)
    drv.sb_normalise_many(C.cast(oracle.lib().pwno_normalise, C.c_void_p), len(v), v.ctypes.data)
    return v


def _exact_any(has_w, pos, ray, mem):
    """trace.h:256-270 in float32, the reference build's operation order (x*x + z*z) + (y*y + w*w); r*r one fp32 product, flushed"""
    f = np.float32
    acc = np.zeros(len(pos), bool)
    with np.errstate(all="ignore"):
        for q in mem:
            r2 = f(q["r"]) * f(q["r"])
            if r2 < f(1.17549435e-38):
                r2 = f(0.0)
            rx, ry, rz = f(q["x"]) - pos[:, 0], f(q["y"]) - pos[:, 1], f(q["z"]) - pos[:, 2]
            if has_w:
                rw = f(1.0) - pos[:, 3]
                d2 = (rx * rx + rz * rz) + (ry * ry + rw * rw)
                dt = (rx * ray[:, 0] + rz * ray[:, 2]) + (ry * ray[:, 1] + rw * ray[:, 3])
            else:
                d2 = (rx * rx + rz * rz) + ry * ry
                dt = (rx * ray[:, 0] + rz * ray[:, 2]) + ry * ray[:, 1]
            assert d2.dtype == np.float32 and dt.dtype == np.float32
            acc |= (dt > 0) & (d2 - dt * dt < r2)
    return acc


def _samples(drv, g, b, mem, has_w, n):
    """(pos, ray) around one list: float32 (n', 4) each"""
    c = np.float64(b["c"])
    cx, cz = b["cell"] % 64, b["cell"] // 64
    P, R = [], []

    def rays_from(d, table=True):
        d = np.float32(d)
        return _normalise(drv, d) if table else np.float32(d / np.linalg.norm(np.float64(d), axis=1, keepdims=True))

    def vec4(xyz, w):
        v = np.zeros((len(xyz), 4))
        v[:, :3] = xyz
        v[:, 3] = w
        return v

    def w_pos(m):
        return np.where(g.random(m) < 0.5, 1.0, 1.0 + g.normal(0, 0.3, m)) if has_w else np.ones(m)

    def w_ray(m):
        return g.normal(0, 0.3, m) * (g.random(m) < 0.7) if has_w else np.zeros(m)

    # random positions in and around the cell, random directions
    m = n
    P.append(vec4(c + g.uniform(-1.4, 1.4, (m, 3)), w_pos(m)))
    R.append(rays_from(vec4(g.normal(0, 1, (m, 3)), w_ray(m))))
    # on the cell's faces (where a ray enters it), floor and ceiling included, aimed roughly at the cluster
    m = n // 2
    p = np.stack([cx + g.random(m), g.random(m) * 2.0, cz + g.random(m)], 1)
    face = g.integers(0, 6, m)
    p[face == 0, 0] = cx
    p[face == 1, 0] = cx + 1
    p[face == 2, 2] = cz
    p[face == 3, 2] = cz + 1
    p[face == 4, 1] = 0.0
    p[face == 5, 1] = 1.0
    P.append(vec4(p, w_pos(m)))
    R.append(rays_from(vec4((c - p) + g.normal(0, 0.5, (m, 3)), w_ray(m))))
    # inside the spheres
    m = n // 4
    j = g.integers(0, len(mem), m)
    ctr = np.stack([np.float64(mem["x"][j]), np.float64(mem["y"][j]), np.float64(mem["z"][j])], 1)
    u = g.normal(0, 1, (m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    P.append(vec4(ctr + u * (np.abs(np.float64(mem["r"][j])) * g.random(m))[:, None], w_pos(m)))
    R.append(rays_from(vec4(g.normal(0, 1, (m, 3)), w_ray(m))))
    # tangent to a member, +- 1e-6 of its radius: through the table normalise and normalised in double
    for table in (True, False):
        m = n // 2
        j = g.integers(0, len(mem), m)
        ctr = np.stack([np.float64(mem["x"][j]), np.float64(mem["y"][j]), np.float64(mem["z"][j])], 1)
        rad = np.abs(np.float64(mem["r"][j]))
        u = g.normal(0, 1, (m, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        dist = rad + g.uniform(0.01, 1.5, m)
        p = ctr - u * dist[:, None]
        v = np.cross(u, g.normal(0, 1, (m, 3)))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        sn = np.clip(rad * (1.0 + g.choice([-1e-6, 0.0, 1e-6], m)) / dist, 0, 1)
        d = u * np.sqrt(1 - sn * sn)[:, None] + v * sn[:, None]
        P.append(vec4(p, np.ones(m)))
        R.append(rays_from(vec4(d, np.zeros(m)), table))
    # the spheres behind the start
    m = n // 4
    p = c + g.uniform(-1.2, 1.2, (m, 3))
    P.append(vec4(p, w_pos(m)))
    R.append(rays_from(vec4((p - c) + g.normal(0, 0.3, (m, 3)), w_ray(m))))
    # rays that are not unit vectors: at the guard's edges and well outside
    m = n // 4
    p = c + g.uniform(-1.2, 1.2, (m, 3))
    d = rays_from(vec4((c - p) + g.normal(0, 0.4, (m, 3)), w_ray(m)), False)
    sc = np.sqrt(1.0 + g.choice([-2.0 ** -10, 2.0 ** -10, -1.1e-3, 1.1e-3, -0.5, 0.5, 3.0], m) * g.choice([1.0, 0.999, 1.001], m))
    P.append(vec4(p, w_pos(m)))
    R.append(np.float32(d * sc[:, None]))
    # zero, denormal, huge, infinite, NaN components in the position or the ray
    m = n // 2
    p = vec4(c + g.uniform(-1.2, 1.2, (m, 3)), w_pos(m))
    d = np.float64(rays_from(vec4((c - p[:, :3]) + g.normal(0, 0.4, (m, 3)), w_ray(m))))
    odd = np.array([0.0, -0.0, 1e-45, -1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan])
    lanes = 4 if has_w else 3
    for arr in (p, d):
        hit = g.random(m) < 0.6
        arr[hit, g.integers(0, lanes, m)[hit]] = g.choice(odd, m)[hit]
    P.append(p)
    R.append(np.float32(d))
    # positions 1e13 away (a far start clamps the cell index into the grid: the list is still visited)
    m = n // 8
    far = g.choice([-1e13, 1e13], (m, 3)) * (g.random((m, 3)) < 0.5)
    p = c + g.uniform(-1, 1, (m, 3)) + far
    P.append(vec4(p, w_pos(m)))
    R.append(rays_from(vec4(c - p + g.normal(0, 0.3, (m, 3)), w_ray(m))))
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.concatenate(P), np.float32), np.ascontiguousarray(np.concatenate(R), np.float32)


def _lists(hip):
    """sphere sets and, per set, the balls pwn_sphere_bounds_plan makes"""
    g = np.random.default_rng(77)
    sets = [load_spheres("t0")]
    for i, (r, spread, n) in enumerate([(1e-4, 0.3, 5), (0.0, 0.05, 4), (0.45, 0.02, 6), (0.02, 0.45, 12), (0.3, 0.15, 4), (1e-20, 0.2, 7)]):
        s = _cluster(5 + 6 * i, 3 + 5 * i, n, r=r, spread=spread, y=0.5, seed=100 + i)
        s["r"] = r * g.uniform(0.5, 1.0, n)
        sets.append(s)
    # spheres of one list that reach into the neighbours, mixed radii, far out in the grid and up a 2-high room
    s = _cluster(60, 61, 9, r=0.2, spread=0.4, y=1.2, seed=200)
    s["r"] = g.uniform(0.01, 0.6, 9)
    sets.append(s)
    out = []
    for s in sets:
        for b in _plan(hip, s):
            out.append((b, _members(hip, s, b["cell"])))
    return out


def test_predicate_is_conservative(hip, drv):
    lists = _lists(hip)
    assert len(lists) >= 8
    g = np.random.default_rng(2026)
    total = skipped = accepted = skipped_in_reach = 0
    per = 15000
    for has_w in (0, 1):
        for b, mem in lists:
            pos, ray = _samples(drv, g, b, mem, has_w, per)
            ball = np.array([b["c"][0], b["c"][1], b["c"][2], b["rr"], -b["r_eff"]], np.float32)
            which = np.zeros(len(pos), np.int32)
            out = np.zeros(len(pos), np.uint8)
            drv.sb_pass_many(has_w, len(pos), pos.ctypes.data, ray.ctypes.data, ball.ctypes.data, which.ctypes.data, out.ctypes.data)
            acc = _exact_any(has_w, pos, ray, mem)
            bad = acc & (out == 0)
            assert not bad.any(), (has_w, b, pos[bad][:4], ray[bad][:4], int(bad.sum()))
            total += len(pos)
            skipped += int((out == 0).sum())
            accepted += int(acc.sum())
            skipped_in_reach += int((out[:per] == 0).sum())
            # a sample with anything not finite in it passes
            nf = ~(np.isfinite(pos[:, :4 if has_w else 3]).all(1) & np.isfinite(ray[:, :4 if has_w else 3]).all(1))
            assert (out[nf] == 1).all()
    assert total >= 1000000, total
    # the test is not vacuous: many samples are accepted by a member, many are skipped, and of the plain random ones around a cell a good part
    assert accepted > total // 20 and skipped > total // 10, (total, accepted, skipped)
    assert skipped_in_reach > (2 * len(lists) * per) // 5, skipped_in_reach
