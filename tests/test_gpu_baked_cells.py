"""The walk's portal arms read what pwn_bake_cells decided per level (cell_bake.h): small frames of the hand-made
levels of tests/baked_scenes.py -- a 2-high hall walled with portal letters whose far sides are of every kind,
unpaired letters, letters off their endpoints, both endpoints in one cell, every rotation, endpoints in row 0 and
column 0 seen from outside the grid -- through the C ABI against the oracle: colour, depth and the path counters,
both schedulers, the 3-lane and the general 4-lane kernels, with and without the counting variants.  The oracle
equals the compiled reference on the same scenes: tests/test_baked_cells.py."""
import numpy as np
import pytest

import baked_scenes as bs

pytestmark = pytest.mark.gpu


def test_hand_made_levels_vs_oracle(oracle_lib, monkeypatch):
    import pwnfps_amd
    portals = 0
    for sc in bs.scenes(oracle_lib.SPHERE_DTYPE):
        O = oracle_lib.Oracle()
        O.set_level(sc.data, sc.pmap)
        O.set_spheres(sc.spheres)
        b, zb, ost = O.render(bs.W, bs.H, sc.cam, sec=sc.sec, blur=0, stats=True)
        b1, _ = O.render(bs.W, bs.H, sc.cam, sec=sc.sec, blur=1)
        want = (ost.rays, ost.steps, ost.portals, ost.sphere_tests, ost.exhausted)
        portals += ost.portals
        for hasw in (False, True):
            # (read when a context is created: the general kernels for a camera without w components)
            if hasw:
                monkeypatch.setenv("PWN_DBG_FORCE_HASW", "1")
            else:
                monkeypatch.delenv("PWN_DBG_FORCE_HASW", raising=False)
            for sched in ("units", "refill"):
                for counters in (False, True):
                    tag = (sc.name, sched, hasw, counters)
                    r = pwnfps_amd.Renderer(bs.W, bs.H)
                    r.upload_level(sc.data, sc.pmap)
                    r.set_objects(sc.spheres)
                    r.set_scheduler(sched)
                    r.set_counters(counters)
                    r.set_blur_passes(0)
                    a, za = r.trace_screen_centred(sc.cam, sc.sec)
                    assert (a == b).all(), (tag, int((a != b).sum()))
                    assert (za.view(np.uint32) == zb.view(np.uint32)).all(), tag
                    if counters:
                        st = r.stats()
                        assert (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"]) == want, tag
                    else:
                        r.set_blur_passes(1)
                        a1, _ = r.trace_screen_centred(sc.cam, sc.sec)
                        assert (a1 == b1).all(), (tag, int((a1 != b1).sum()))
                    r.close()
    assert portals > 10000      # the scenes do walk through portals


def test_a_new_portal_table_for_the_same_grid_is_baked_again(oracle_lib):
    """pwn_upload_level with the grid unchanged and another portal table: the baked words and records follow"""
    import pwnfps_amd
    sc = {s.name: s for s in bs.scenes(oracle_lib.SPHERE_DTYPE)}
    first, second = sc["hall_upper"], sc["both_endpoints_one_cell"]
    assert (first.data == second.data).all() and not (first.pmap == second.pmap).all()
    r = pwnfps_amd.Renderer(bs.W, bs.H)
    r.set_blur_passes(0)
    O = oracle_lib.Oracle()
    # where a ray runs out of steps the depth plane keeps what the context's last frame left (trace.h:677): the oracle
    # traces into the planes of its last frame as the context does
    sb = zb = None
    for s in (first, second, first):
        r.upload_level(s.data, s.pmap)
        r.set_objects(first.spheres)
        O.set_level(s.data, s.pmap)
        O.set_spheres(first.spheres)
        a, za = r.trace_screen_centred(first.cam, 0.5)
        sb, zb, _ = O.trace_rows(bs.W, bs.H, 0, bs.H, first.cam, sec=0.5, sb=sb, zb=zb)
        assert (a == sb).all(), (s.name, int((a != sb).sum()))
        assert (za.view(np.uint32) == zb.view(np.uint32)).all(), s.name
    r.close()


def test_tables_with_an_endpoint_outside_the_grid_are_refused(oracle_lib):
    """pwn_upload_level: PWN_EINVAL for the tables of baked_scenes.refused_tables (on them a cell at coordinate -1 is an
    endpoint for the reference; tests/test_baked_cells.py), and the level the context had still renders"""
    import pwnfps_amd
    from pwnfps_amd import PwnError
    sc = next(s for s in bs.scenes(oracle_lib.SPHERE_DTYPE) if s.name == "corner_minus_one")
    O = oracle_lib.Oracle()
    O.set_level(sc.data, sc.pmap)
    O.set_spheres(sc.spheres)
    b, zb = O.render(bs.W, bs.H, sc.cam, sec=sc.sec, blur=0)
    r = pwnfps_amd.Renderer(bs.W, bs.H)
    r.set_blur_passes(0)
    r.upload_level(sc.data, sc.pmap)
    r.set_objects(sc.spheres)
    for name, data, pmap in bs.refused_tables():
        with pytest.raises(PwnError) as e:
            r.upload_level(data, pmap)
        assert e.value.code == -1, name
    d, p, _ = r.get_level()
    assert (d == sc.data).all() and (p == sc.pmap).all()
    a, za = r.trace_screen_centred(sc.cam, sc.sec)
    assert (a == b).all() and (za.view(np.uint32) == zb.view(np.uint32)).all()
    r.close()


def test_the_table_as_level_load_leaves_it(oracle_lib):
    """A host that keeps the reference's level_load hands over its table as it is: level_new sets x1, x2, c1 and c2 only
    (level.h:94-99), so an endpoint never seen has x == -1 beside a z of 0, or of the level loaded before.  level.txt
    (21 pairs of 26 letters) with such tables through pwn_upload_level, against the oracle with the same table."""
    import pwnfps_amd
    from conftest import level_path, load_spheres
    sph = load_spheres("t0")
    r = pwnfps_amd.Renderer(320, 200)
    r.level_load(level_path("pwnfps_level"))
    data, pmap, spawn = r.get_level()
    r.close()
    cam = pwnfps_amd.spawn_camera(spawn, ang_y=0.4)
    rng = np.random.default_rng(5)
    for stale in (None, rng.integers(0, 64, (26, 2)), np.zeros((26, 2), np.int64) + 4):
        pm = bs.as_level_load_leaves_it(pmap, stale)
        assert not (pm == pmap).all()
        O = oracle_lib.Oracle()
        O.set_level(data, pm)
        O.set_spheres(sph)
        b, zb, ost = O.render(320, 200, cam, sec=1.0, blur=0, stats=True)
        for sched in ("units", "refill"):
            r = pwnfps_amd.Renderer(320, 200)
            r.upload_level(data, pm)
            r.set_objects(sph)
            r.set_scheduler(sched)
            r.set_counters(True)
            r.set_blur_passes(0)
            a, za = r.trace_screen_centred(cam, 1.0)
            st = r.stats()
            assert (a == b).all() and (za.view(np.uint32) == zb.view(np.uint32)).all(), sched
            assert (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"]) == \
                (ost.rays, ost.steps, ost.portals, ost.sphere_tests, ost.exhausted), sched
            r.close()
