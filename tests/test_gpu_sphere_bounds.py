"""The walk skips a cell's sphere list for a wave none of whose rays can meet the list's bounding ball (trace_walk.inc,
sphere_bound.h): frames with the balls in the launch's arguments and without them (PWN_SPHERE_BOUNDS=0), bit for bit against the
oracle -- colour, depth and the five counters, the sphere tests among them: a skip counts the tests it did not make.

Scenes: the level's own cluster from its room's far end, from inside its cell, from inside its big sphere and looking away from
it; in a hall of 2-high cells a small cluster seen from far (most waves skip it), three clusters in cells that touch (the lanes
of one wave stand on different lists in the same step: the path that does not ask the ball) and six clusters (more lists than
balls).  Every scene with a camera without and with w components, the three forms of the lists, both schedulers; one case each
through views, rays and hits.  All frames are 128 x 64 or smaller; the oracle renders each (scene, camera) once."""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
from conftest import level_path, load_spheres
from oracle import SPHERE_DTYPE

pytestmark = pytest.mark.gpu

W, H = 128, 64
HALL = "\n".join(["." * 64] + ["." + "#" * 12 + "." * 51] * 20 + ["." * 64]) + "\n"
RG_SPHTEST, RG_SPHBOUND, RG_SPHSKIP = 14, 24, 25         # trace_common.h


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cam(x, y, z, ang_y=0.0, ang_x=0.0):
    cy, sy, cx, sx = np.cos(ang_y), np.sin(ang_y), np.cos(ang_x), np.sin(ang_x)
    cam = np.eye(4, dtype=np.float32)
    cam[:3, :3] = (np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])).astype(np.float32)
    cam[3, :3] = (x, y, z)
    return cam


def _with_w(cam):
    """the same camera with w components: the kernels' 4-lane variants, relw = 1 - pos.w in every sphere test"""
    c = cam.copy()
    c[:, 3] = (0.05, -0.03, 0.2, 0.9)
    return c


def _cluster(cx, cz, n, seed, r=(0.02, 0.06), spread=0.1, y=0.6):
    g = np.random.default_rng(seed)
    s = np.zeros(n, SPHERE_DTYPE)
    s["x"] = cx + 0.5 + g.uniform(-spread, spread, n)
    s["z"] = cz + 0.5 + g.uniform(-spread, spread, n)
    s["y"] = y + g.uniform(-spread, spread, n)
    s["r"] = g.uniform(r[0], r[1], n)
    s["refl"] = g.choice([0.0, 0.5], n)
    s["cb"], s["cg"], s["cr"] = g.uniform(0.2, 1, n), g.uniform(0.2, 1, n), g.uniform(0.2, 1, n)
    return s


def _scenes():
    t0 = load_spheres("t0")
    lvl = level_path("pwnfps_level")
    three = np.concatenate([_cluster(6, 12, 9, 1), _cluster(7, 12, 8, 2), _cluster(6, 11, 7, 3)])
    six = np.concatenate([_cluster(4 + 2 * (i % 3), 10 + 2 * (i // 3), 5 + i, 10 + i) for i in range(6)])
    #        name            level  spheres              camera                             sec   bounded lists
    return [("t0_far",       lvl,   t0,                  _cam(11.7, 0.6, 5.5, np.pi / 2) ,   0.0,  1),
            ("t0_in_cell",   lvl,   t0,                  _cam(9.15, 1.2, 5.2, 0.6, 0.5),    1.25, 1),
            ("t0_in_sphere", lvl,   t0,                  _cam(9.55, 0.25, 5.45, 2.0, 0.1),  0.5,  1),
            ("t0_away",      lvl,   t0,                  _cam(9.5, 0.5, 4.5, np.pi, 0.0),   0.0,  1),
            ("hall_far",     HALL,  _cluster(6, 12, 14, 7), _cam(6.4, 0.5, 5.5, 0.0, -0.05), 0.75, 1),
            ("hall_three",   HALL,  three,               _cam(7.02, 0.7, 7.5, 0.03, 0.0),   0.25, 3),
            ("hall_six",     HALL,  six,                 _cam(6.5, 0.8, 4.5, 0.1, -0.1),    2.0,  4)]


SCENES = _scenes()
IDS = [s[0] for s in SCENES]
_refs = {}


def _ref(oracle_lib, sc, hasw):
    """the oracle's pre-blur frame, depth and counters of (scene, camera): rendered once, shared, never written to"""
    key = (sc[0], hasw)
    if key not in _refs:
        name, level, sph, cam, sec, _ = sc
        O = oracle_lib.Oracle()
        (O.load_level if HS.is_path(level) else O.load_level_text)(level)
        O.set_spheres(sph)
        cam = _with_w(cam) if hasw else cam
        sb, z, st = HS.fresh(O, W, H, cam, sec, 0)
        sb.setflags(write=False)
        z.setflags(write=False)
        # (no ray of these frames runs out of steps: every pixel's depth is written, a context's earlier frames leave nothing behind)
        assert st.exhausted == 0 and st.sphere_tests > 0, (key, HS.stats5(st))
        _refs[key] = (cam, sb, z, HS.stats5(st))
    return _refs[key]


def _renderer(sc, lists, bounds, w=W, h=H):
    import pwnfps_amd
    env = {"PWN_SPHERE_BOUNDS": "1" if bounds else "0"}
    if lists != "default":
        env["PWN_SPHERE_LISTS"] = lists
    with _env(**env):
        r = pwnfps_amd.Renderer(w, h)
    (r.level_load if HS.is_path(sc[1]) else r.level_load_text)(sc[1])
    r.set_objects(sc[2])
    r.set_blur_passes(0)
    return r


def test_scenes_have_the_balls_they_are_about():
    import pwnfps_amd
    for sc in SCENES:
        b = pwnfps_amd.sphere_bounds_plan(sc[2])
        assert len(b) == sc[5], (sc[0], b)
    assert pwnfps_amd.sphere_tables_plan(SCENES[-1][2])["cells"] == 6


@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "nobounds"])
@pytest.mark.parametrize("lists", ["indexed", "inline", "global"])
@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_frames(oracle_lib, sc, lists, bounds):
    """colour, depth and the five counters of every scene: camera without and with w, both schedulers"""
    r = _renderer(sc, lists, bounds)
    r.set_counters(True)
    for sched in ("units", "refill"):
        r.set_scheduler(sched)
        want_form = {"indexed": 0, "inline": 1 if sched == "units" else 0, "global": 2}[lists]
        assert r.sphere_tables()["form"] == want_form, (sc[0], lists, sched, r.sphere_tables())
        for hasw in (False, True):
            cam, sb, z, st = _ref(oracle_lib, sc, hasw)
            got, gz = r.trace_screen_centred(cam, sc[4])
            what = (sc[0], lists, bounds, sched, hasw)
            bad = got != sb
            assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert (HS.bits(gz) == HS.bits(z)).all(), (what, "depth")
            assert HS.stats5(r.stats()) == st, (what, HS.stats5(r.stats()), st)
    r.close()


@pytest.mark.parametrize("lists", ["indexed", "inline", "global"])
@pytest.mark.parametrize("name", ["t0_far", "hall_far"])
def test_the_skip_runs(oracle_lib, name, lists):
    """the counting variant's region counters on the two far views -- the level's own cluster from its room's far end and the small
    cluster down the hall -- in each form of the lists (the id a ball carries is the form's own: a wrong one would switch the skip
    off and leave every frame right): with the balls the view makes fewer than 0.6 of the wave-level sphere tests it makes without
    (14 per visit of the list then), every visit asks the ball, and the sphere-test COUNTER is the same"""
    sc = SCENES[IDS.index(name)]
    cam, sb, z, st = _ref(oracle_lib, sc, False)
    seen = {}
    for bounds in (True, False):
        r = _renderer(sc, lists, bounds)
        assert r.sphere_tables()["form"] == {"indexed": 0, "inline": 1, "global": 2}[lists]
        r.set_counters(True)
        got, gz = r.trace_screen_centred(cam, sc[4])
        s = r.stats()
        r.close()
        assert (got == sb).all() and HS.stats5(s) == st
        seen[bounds] = (s["regions"][RG_SPHTEST], s["regions"][RG_SPHBOUND], s["regions"][RG_SPHSKIP], s["wave_paths"][0])
    print("sphere bounds, %s, %s: (w_sphtest, w_sphbound, skips, w_sphlist) on %s, off %s" % (name, lists, seen[True], seen[False]))
    on, off = seen[True], seen[False]
    assert off[1] == 0 and off[2] == 0 and off[0] == 14 * off[3] and off[3] > 50
    assert on[3] == off[3] and on[1] == on[3] and on[2] > 0
    assert on[0] == 14 * (on[3] - on[2])
    assert on[0] < 0.6 * off[0], (on, off)


def test_lanes_on_different_lists_run_them(oracle_lib):
    """hall_three: some waves visit lists without asking a ball although every list has one -- their lanes stand on two lists"""
    sc = SCENES[IDS.index("hall_three")]
    cam, sb, z, st = _ref(oracle_lib, sc, False)
    r = _renderer(sc, "default", True)
    r.set_counters(True)
    got, _ = r.trace_screen_centred(cam, sc[4])
    s = r.stats()
    r.close()
    assert (got == sb).all() and HS.stats5(s) == st
    print("sphere bounds, hall_three: w_sphlist %d, w_sphbound %d, skips %d" % (s["wave_paths"][0], s["regions"][RG_SPHBOUND], s["regions"][RG_SPHSKIP]))
    assert 0 < s["regions"][RG_SPHBOUND] < s["wave_paths"][0]
    assert s["regions"][RG_SPHSKIP] > 0


def test_lists_without_a_ball_are_run(oracle_lib):
    """hall_six: four lists have balls, the two shortest are visited without"""
    sc = SCENES[IDS.index("hall_six")]
    cam, sb, z, st = _ref(oracle_lib, sc, False)
    r = _renderer(sc, "default", True)
    r.set_counters(True)
    got, _ = r.trace_screen_centred(cam, sc[4])
    s = r.stats()
    r.close()
    assert (got == sb).all() and HS.stats5(s) == st
    assert 0 < s["regions"][RG_SPHBOUND] < s["wave_paths"][0] and s["regions"][RG_SPHSKIP] > 0


@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "nobounds"])
def test_views_rays_hits(oracle_lib, bounds):
    """one case each through pwn_trace_views, pwn_trace_rays and pwn_trace_hits (the three-cluster hall, camera with w components
    among the views)"""
    import pwnfps_amd
    sc = SCENES[IDS.index("hall_three")]
    cam0, sb0, z0, st0 = _ref(oracle_lib, sc, False)
    cam1, sb1, z1, st1 = _ref(oracle_lib, sc, True)
    r = _renderer(sc, "default", bounds)
    r.set_counters(True)
    a, za = r.trace_views(np.stack([cam0, cam1]), np.array([sc[4], sc[4]], np.float32))
    assert (a[0] == sb0).all() and (a[1] == sb1).all(), "views"
    assert (HS.bits(za[0]) == HS.bits(z0)).all() and (HS.bits(za[1]) == HS.bits(z1)).all(), "views depth"
    assert HS.stats5(r.stats()) == tuple(x + y for x, y in zip(st0, st1))
    # every pixel of the frame as a ray of the caller's
    rays, seeds, xy = pwnfps_amd.pixel_rays(W, H, cam0)
    col, zz = r.trace_rays(rays, seeds, sc[4])
    assert (col == sb0[xy[:, 1], xy[:, 0]]).all(), "rays"
    assert (HS.bits(zz) == HS.bits(z0)[xy[:, 1], xy[:, 0]]).all(), "rays depth"
    assert HS.stats5(r.stats()) == st0
    # first hits: a record's dist is the frame's depth; no ray of this hall runs out of steps
    hits = r.trace_hits(rays)
    assert (hits["kind"] != 0).all() and (hits["kind"] == 2).any()
    assert (HS.bits(hits["dist"]) == HS.bits(z0)[xy[:, 1], xy[:, 0]]).all(), "hits"
    r.close()
