"""PWN_OPT_UNIT_ORDER (an option, off by default): the trace kernel hands its units out by what they cost in the last launch of the same rows (every
unit's cost written by the launch, sorted per queue behind the frame's last kernel).  Any order of the units gives the same
frame: every frame of a sequence is the golden frame and has the golden counters, whichever order it was traced in; and the
sorted order really is used (pwn_unit_order_state).  A launch that follows a sort must not find its frame in the planes already
(a permutation that dropped units would leave it there): frames of a camera walk (tests/handout.py) stand between the golden
frames, judged by the oracle, so every ordered launch renders what the planes do not hold.  Replaces the static schedule of
screen.h:63-64."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu


def case(cases, name):
    return [c for c in cases if c["name"] == name][0]


def _oracle_of(c):
    """the oracle on a case's level, which is one of the walk's, with the case's spheres"""
    import handout as H
    assert H.LEVELS[c["level"]] == c["spheres"]
    return H.scene(c["level"])[0]


@pytest.mark.parametrize("name", ["level_spawn_1280x720", "synth64_cam1_1920x1080", "synth256_cam0_1920x1080", "level_spawn_3840x2160"])
def test_every_frame_of_a_sequence_is_the_golden_frame_in_any_order(name, cases, oracle_lib):
    import handout as H
    import pwnfps_amd
    c = case(cases, name)
    w, h = c["w"], c["h"]
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    cam = np.array(c["cam"], np.float32).reshape(4, 4)
    plane = H.Shown(_oracle_of(c), w, h)
    # (a ray that runs out of steps keeps the depth it finds: where the golden frame has such rays it is the golden frame only on
    # its own depth, and the walk's frames cannot stand between the golden ones -- they follow at the end)
    between = c["exhausted"] == 0
    assert r.unit_order_state()["option"] == 0          # off by default: measured a loss on long launches (profiles/r4/unit_order_ab.txt)
    r.set_unit_order(True)
    for k in range(5):
        if k == 3:
            r.set_counters(True)
        sb, z = r.trace_screen_centred(cam, c["sec"])
        assert oracle_lib.fnv64(sb) == c["post"] and oracle_lib.fnv64(z) == c["z"], (name, k)
        if k == 3:
            st = r.stats()
            assert (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"]) == (
                c["rays"], c["steps"], c["portals"], c["sphere_tests"], c["exhausted"])
            r.set_counters(False)
        # the oracle's side of the plane: the golden frame is what the planes hold now, no unit of the walk's frame keeps it ...
        want = plane.show(cam, c["sec"], 1, again=k > 0 and not between)
        assert oracle_lib.fnv64(want[0]) == c["post"] and oracle_lib.fnv64(want[1]) == c["z"], (name, k)
        if between and k < 4:
            # ... and the walk's frame k, in the order sorted from the golden frame's costs; the next golden frame follows in its order
            wcam, wsec = H.walk(c["level"], k)
            want = plane.show(wcam, wsec, 1)
            sb, z = r.trace_screen_centred(wcam, wsec)
            H.same((name, "walk", k), sb, z, *want)
    st = r.unit_order_state()
    assert st["sorts"] == (9 if between else 5) and st["launches_in_sorted_order"] == (8 if between else 4), st
    assert st["units_ordered"] == ((w + 15) // 16) * ((h + 3) // 4), st
    # ... and switched off: arithmetic order again, same frame
    r.set_unit_order(False)
    sb, z = r.trace_screen_centred(cam, c["sec"])
    assert oracle_lib.fnv64(sb) == c["post"]
    assert r.unit_order_state()["launches_in_sorted_order"] == (8 if between else 4)
    if not between:
        # switched on again (which forgets the orders): the golden frame in arithmetic order, then two frames of the walk, each in
        # the order sorted from the launch before it
        plane.show(cam, c["sec"], 1, again=True)
        r.set_unit_order(True)
        sb, z = r.trace_screen_centred(cam, c["sec"])
        assert oracle_lib.fnv64(sb) == c["post"] and oracle_lib.fnv64(z) == c["z"], name
        H.same((name, "golden again"), sb, z, *plane.show(cam, c["sec"], 1, again=True))
        for k in range(2):
            wcam, wsec = H.walk(c["level"], k)
            want = plane.show(wcam, wsec, 1)
            sb, z = r.trace_screen_centred(wcam, wsec)
            H.same((name, "walk", k), sb, z, *want)
        st = r.unit_order_state()
        assert st["sorts"] == 8 and st["launches_in_sorted_order"] == 6, st
    r.close()


def test_order_follows_the_rows_it_was_made_for(cases, oracle_lib):
    """A strip launch (pwn_trace_rows_device) and frames of another camera in between: an order is only used for the rows it was
    sorted from; frames in flight on two streams each keep their stream's own.  Every second submit is a frame of the camera
    walk, so each slot is shown the golden frame and a frame of the walk in turn and no launch finds its frame in its slot."""
    import handout as H
    import pwnfps_amd
    c = case(cases, "level_spawn_1280x720")
    w, h = c["w"], c["h"]
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    cam = np.array(c["cam"], np.float32).reshape(4, 4)
    r.set_unit_order(True)
    r.frames_config(3, sbuf=True, zbuf=True)
    planes = [H.Shown(_oracle_of(c), w, h) for _ in range(3)]
    want = {}

    def delivered(k):
        # (k: the submit that is waited for)
        f = r.wait_frame(k % 3)
        if k % 2 == 0:
            assert oracle_lib.fnv64(f["sbuf"]) == c["post"], k
        H.same(("in flight", k), f["sbuf"], f["zbuf"], *want.pop(k))
    for k in range(9):
        if k >= 3:
            delivered(k - 3)
        fcam, fsec = (cam, c["sec"]) if k % 2 == 0 else H.walk(c["level"], k)
        want[k] = planes[k % 3].show(fcam, fsec, 1)
        r.submit_frame(fcam, fsec, k % 3)
    for k in range(9, 12):
        delivered(k - 3)
    st = r.unit_order_state()
    assert st["sorts"] == 9 and st["launches_in_sorted_order"] == 7, st          # each stream's first frame runs in arithmetic order
    r.frames_config(0)
    sb, _ = r.trace_screen_centred(cam, c["sec"])
    assert oracle_lib.fnv64(sb) == c["post"]
    r.close()


@pytest.mark.parametrize("units", [64, 65, 4 * 64 + 3, 14400, 129600, 518400, 2073600])
def test_the_sort_hands_out_every_unit_once_dearest_first(units):
    """pwn_order_kernel by itself: for random costs (with many ties, zeros and saturated entries) every queue's row is a
    permutation of exactly that queue's units, in order of falling cost -- whatever the costs, every unit is handed out once."""
    import pwnfps_amd
    rng = np.random.default_rng(units)
    cost = rng.integers(0, 40, units).astype(np.uint16) * rng.integers(0, 3, units).astype(np.uint16) * 300
    cost[rng.integers(0, units, max(1, units // 50))] = 65535
    r = pwnfps_amd.Renderer(320, 240)
    perm = r.unit_order_probe(cost)
    r.close()
    cap = (units + 63) // 64
    assert perm.shape == (64, cap)
    seen = np.zeros(units, np.int32)
    for q in range(64):
        n = (units + 63 - q) // 64
        row = perm[q, :n].astype(np.int64)
        assert (perm[q, n:] == 0xffffffff).all()
        assert ((row % 64) == q).all() and (row < units).all()
        np.add.at(seen, row, 1)
        c = np.minimum(cost[row].astype(np.int64) >> 3, 255)          # the sort's cost classes (0.32 us each; order inside one is free)
        assert (np.diff(c) <= 0).all(), q
    assert (seen == 1).all()
