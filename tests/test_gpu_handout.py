"""The hand-out: every trace launch of a sequence traces each of its 16 x 4 units, and the counting kernels trace each exactly once.

A launch that skips a unit writes no wrong pixel: it leaves what the planes held.  So no launch here finds the right answer
already in its planes (tests/handout.py): planes of the caller's are poisoned afresh for every launch, planes of the library's are
shown a camera walk of which no unit keeps colour and depth from one frame to the next, asserted from the oracle's frames before
the GPU's are looked at.  Every sequence is 8 launches through one context or more: more than the six ticket sets there are and
than the four in use at R = 2, so every set is drawn from after a launch of the same context cleared it.  The judge is the oracle.

  1. sequences of device rows -- whole frame and strip in turn, so the item count changes from launch to launch -- through every
     way the units are handed out: tile pairs off / by rule / forced, a sorted order, the refill scheduler, the 4-lane kernels,
     the sphere lists' forms; on the machine's grid, on one workgroup per CU and on that less a reserve of 100;
  2. the same with the counters on: the five counters are the oracle's and every unit is entered once (regions[13]), every right
     half made once (regions[17] + regions[26]), on every launch.  This holds the COUNTING instantiations only: a unit traced
     twice by a kernel that does not count cannot be seen from outside, tracing is idempotent;
  3. planes the library owns: the blocking call in one piece and in strips, frames in flight, view slots, viewports, a group;
  4. one context through twelve launches of six kinds, two of them on a stream that is not the context's.
"""
import contextlib
import os

import numpy as np
import pytest

import handout as H

pytestmark = pytest.mark.gpu

LEVEL = H.LEVEL
# how the units are handed out: environment of the context, and what is set on it
CONTEXTS = {
    "pairs0": {"env": {"PWN_TILE_PAIRS": 0}},
    "pairs1": {"env": {"PWN_TILE_PAIRS": 1}},
    "pairs2": {"env": {"PWN_TILE_PAIRS": 2}},
    "order": {"order": True},
    "refill1": {"refill": 1},
    "refill200": {"refill": 200},
    "force_hasw": {"env": {"PWN_DBG_FORCE_HASW": 1}},
    "indexed": {"env": {"PWN_SPHERE_LISTS": "indexed"}},
    "global": {"env": {"PWN_SPHERE_LISTS": "global"}},
}
# the grid: environment, PWN_OPT_TRACE_ROOM (the reserve shrinks the grid: QBASE and the threshold of draw_n move with it)
GRIDS = {"own": ({}, None), "one_per_cu": ({"PWN_DBG_BLOCKS_PER_CU": 1}, None), "one_per_cu_room100": ({"PWN_DBG_BLOCKS_PER_CU": 1}, 100)}
# shape -> its strips: rows that are no multiples of 4 and that do not hold the frame's middle row
SMALL = {
    (40, 5): [(3, 5)],                  # 6 units, fewer than waves: static tickets past the queue's end go straight to the help path
    (56, 64): [(5, 19), (37, 63)],      # odd units per row, the last tile's right half partial, 64 units = one per queue
}
LARGE = {
    (1000, 260): [(5, 119)],            # one workgroup per CU: static tickets, drawn tickets and the help path
    (4080, 262): [(3, 125)],            # 16 830 units >= 16 x 4 x 256: tickets two at a time, queues of 263 and 262; by rule, single rows first
}
LARGE_CONTEXTS = ("pairs0", "pairs1", "pairs2", "order")


@contextlib.contextmanager
def _env(kv):
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


def _renderer(w, h, env=None, level=LEVEL, **kw):
    """(the environment is read when a context is created)"""
    import pwnfps_amd
    _, path, sph, _ = H.scene(level)
    with _env(env or {}):
        r = pwnfps_amd.Renderer(w, h, **kw)
    r.level_load(path)
    r.set_objects(sph)
    return r


def _context(name, grid, w, h):
    c = CONTEXTS[name]
    genv, room = GRIDS[grid]
    r = _renderer(w, h, dict(c.get("env", {}), **genv))
    if name == "global":
        assert r.sphere_tables()["form"] == 2, r.sphere_tables()
    if name == "indexed":
        assert r.sphere_tables()["form"] == 0, r.sphere_tables()
    if "refill" in c:
        r.set_scheduler("refill")
        r.set_refill_limit(c["refill"])
    if c.get("order"):
        r.set_unit_order(True)
    if room is not None:
        r.set_trace_room(room)
        assert r.trace_room_state()["room_now"] == room
    return r


def _sequence(name, strips):
    """the 8 launches of a sequence of device rows as (y0, y1) or None for the whole frame: frame and strip in turn -- an order is
    only valid for the rows it was sorted from, so a context with an order runs each kind twice running, and its second launch
    of a kind is the one that is handed out in sorted order"""
    kinds = "FFSSFFSS" if CONTEXTS[name].get("order") else "FSFSFSFS"
    out, blocks = [], -1
    for n, kind in enumerate(kinds):
        if kind == "S" and (n == 0 or kinds[n - 1] != "S"):
            blocks += 1
        out.append(strips[blocks % len(strips)] if kind == "S" else None)
    assert len(out) == H.FRAMES
    return out


def _poisoned(torch, w, h):
    return (torch.full((h, w), H.POISON_S, dtype=torch.int32, device="cuda"), torch.full((h, w), H.POISON_Z, dtype=torch.int32, device="cuda"))


def _rows_launch(r, torch, w, h, k, y0, y1, what, stream=0, blur_behind=None):
    """one launch of rows [y0, y1) of the walk's frame k into freshly poisoned planes: those rows are the oracle's, in colour and in
    depth bits, and every other row is still poison.  Returns the oracle's five counters of the rows."""
    want_sb, want_z, st5 = H.poisoned_rows(LEVEL, w, h, k, y0, y1)
    d_sb, d_zb = _poisoned(torch, w, h)
    torch.cuda.synchronize()
    cam, sec = H.walk(LEVEL, k)
    r.trace_rows_device(cam, sec, y0, y1, d_sb.data_ptr(), d_zb.data_ptr(), stream)
    if blur_behind is not None:
        # (a strip's trace and blur on one stream: behind the blur the launch's unit costs are sorted into the stream's next order)
        r.blur_rows_device(y0, y1, d_sb.data_ptr(), d_zb.data_ptr(), blur_behind.data_ptr(), stream)
    torch.cuda.synchronize()
    sb = d_sb.cpu().numpy().view(np.uint32)
    zb = d_zb.cpu().numpy().view(np.uint32)
    H.same((what, k, y0, y1), sb[y0:y1], zb[y0:y1], want_sb, want_z)
    out = np.ones(h, bool)
    out[y0:y1] = False
    assert (sb[out] == H.POISON_S).all() and (zb[out] == H.POISON_Z).all(), (what, k, y0, y1, "rows outside the launch")
    return st5


def _pairs_in_force(name, grid, units, cus):
    """does a frame's launch of `units` units hand out tiles (launch_plan.h): True, False, or None where this test cannot know the
    grid.  By rule (PWN_TILE_PAIRS=1, the default): where tickets would go out in pairs, 16 units or more per wave of the grid."""
    c = CONTEXTS[name]
    if c.get("order") or "refill" in c:
        return False
    setting = int(c.get("env", {}).get("PWN_TILE_PAIRS", 1))
    if setting != 1:
        return setting == 2
    if grid == "own":
        return False if units < 64 * cus else None          # (at least one workgroup per CU)
    g = cus - 100 if (grid == "one_per_cu_room100" and cus > 200) else cus
    return units >= 64 * g


def _exactly_once(name, grid, st, st5, w, rows, cus, what):
    import hard_scenes as HS
    assert HS.stats5(st) == st5, (what, HS.stats5(st), st5)
    if "refill" in CONTEXTS[name]:
        return          # (the refill kernel has no region counts; a unit traced twice shows in its rays)
    ux, uy = (w + 15) // 16, (rows + 3) // 4
    rg = st["regions"]
    assert rg[13] == ux * uy, (what, rg[13], ux * uy)
    right = (ux // 2) * uy
    assert rg[17] + rg[26] == right, (what, rg[17], rg[26], right)
    pairs = _pairs_in_force(name, grid, ux * uy, cus)
    if pairs is False:
        assert rg[26] == 0, (what, rg[17], rg[26])
    elif pairs is True and int(CONTEXTS[name]["env"]["PWN_TILE_PAIRS"]) == 2:
        assert rg[17] == 0, (what, rg[17], rg[26])
    elif pairs is True and right > 0:
        assert 0 < rg[26] < right, (what, rg[17], rg[26], right)          # the launch starts on rows of single units


def _device_rows(name, grid, w, h, strips, counters):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seq = _sequence(name, strips)
    for k, rows in enumerate(seq):                  # (the oracle's rows first: a failure there is not the library's)
        H.poisoned_rows(LEVEL, w, h, k, *(rows or (0, h)))
    r = _context(name, grid, w, h)
    order = bool(CONTEXTS[name].get("order"))
    d_out = torch.zeros((h, w), dtype=torch.int32, device="cuda") if order else None
    if counters:
        r.set_counters(True)
    for k, rows in enumerate(seq):
        y0, y1 = rows or (0, h)
        what = (name, grid, w, h, "counters" if counters else "plain")
        st5 = _rows_launch(r, torch, w, h, k, y0, y1, what, blur_behind=d_out)
        if counters:
            _exactly_once(name, grid, r.stats(), st5, w, y1 - y0, cus, what + (k, y0, y1))
    if order:
        st = r.unit_order_state()
        # every launch's costs are sorted where it has 4 x 64 units or more; the second launch of each pair runs in that order
        sortable = [H.units_of((rows or (0, h))[1] - (rows or (0, h))[0], w) >= 256 for rows in seq]
        assert st["option"] == 1 and st["sorts"] == sum(sortable), (st, sortable)
        assert st["launches_in_sorted_order"] == sum(sortable[n - 1] and seq[n] == seq[n - 1] for n in range(1, len(seq))), st
        if (w, h) in LARGE:
            assert st["launches_in_sorted_order"] >= 2, st
    r.close()


def _ids(shapes):
    return ["%dx%d" % s for s in shapes]


@pytest.mark.parametrize("counters", [False, True], ids=["plain", "counters"])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("name", list(CONTEXTS))
@pytest.mark.parametrize("shape", list(SMALL), ids=_ids(SMALL))
def test_every_launch_of_device_rows_small(shape, name, grid, counters):
    _device_rows(name, grid, shape[0], shape[1], SMALL[shape], counters)


@pytest.mark.parametrize("counters", [False, True], ids=["plain", "counters"])
@pytest.mark.parametrize("name", LARGE_CONTEXTS)
@pytest.mark.parametrize("shape", list(LARGE), ids=_ids(LARGE))
def test_every_launch_of_device_rows_large(shape, name, counters):
    """one workgroup per CU: more items than waves"""
    _device_rows(name, "one_per_cu", shape[0], shape[1], LARGE[shape], counters)


def test_tile_pairs_by_rule_start_on_single_rows():
    """(what the 4080 x 262 case above relies on: with 256 CUs or fewer its whole frame is long enough for the rule)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _pairs_in_force("pairs1", "one_per_cu", H.units_of(262, 4080), cus) == (cus <= 262)
    assert _pairs_in_force("pairs1", "one_per_cu", H.units_of(122, 4080), cus) is False


# ---------------------------------------------------------------- planes the library owns ----

def _planes(test):
    """the oracle's frames of a test's planes, the walk's precondition asserted on each of them first"""
    return [H.assert_walk_hides_nothing(*p) for p in H.library_planes()[test]]


LIB_GRIDS = {"own": {}, "one_per_cu": {"PWN_DBG_BLOCKS_PER_CU": 1}}
lib_grids = pytest.mark.parametrize("grid", list(LIB_GRIDS))


def _blocking(r, frames, what):
    for k, (pre, z, post) in enumerate(frames):
        cam, sec = H.walk(LEVEL, k)
        sb, zb = r.trace_screen_centred(cam, sec)
        H.same((what, k), sb, zb, post, z)


@lib_grids
def test_blocking_call_in_one_launch_per_pass(grid):
    (frames,) = _planes("blocking")
    r = _renderer(*H.BLOCKING, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    r.set_call_strips(0)
    _blocking(r, frames, "blocking")
    assert r.call_strips_state()["strips_last"] == 1
    r.close()


@lib_grids
def test_blocking_call_in_strips(grid):
    (frames,) = _planes("stripped")
    r = _renderer(*H.STRIPPED, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    r.set_call_strips(4)
    _blocking(r, frames, "stripped")
    st = r.call_strips_state()
    assert st["strips_last"] == 4 and st["calls_in_strips"] == H.FRAMES, st
    r.close()


@lib_grids
def test_group_of_three_on_one_device(grid):
    (frames,) = _planes("blocking")
    r = _renderer(*H.BLOCKING, env=LIB_GRIDS[grid], devices=[0, 0, 0])
    assert r.group_info()["members"] == 3
    r.set_blur_passes(1)
    _blocking(r, frames, "group of three")
    r.close()


@lib_grids
@pytest.mark.parametrize("order", [False, True], ids=["arithmetic", "sorted"])
def test_frames_in_flight_on_three_slots(order, grid):
    """two streams, three slots: each slot's camera is the walk's at its submit, each slot's depth plane its own"""
    slots = _planes("in_flight")
    w, h = H.IN_FLIGHT
    r = _renderer(w, h, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    r.set_unit_order(order)
    r.frames_config(3, sbuf=True, zbuf=True)

    def check(j):
        fr = r.wait_frame(j % 3)
        pre, z, post = slots[j % 3][j // 3]
        H.same(("in flight", order, j), fr["sbuf"], fr["zbuf"], post, z)
    for j in range(H.FRAMES):
        if j >= 3:
            check(j - 3)
        cam, sec = H.walk(LEVEL, j)
        r.submit_frame(cam, sec, j % 3)
    for j in range(H.FRAMES - 3, H.FRAMES):
        check(j)
    st = r.unit_order_state()
    if order:
        # each stream's first frame runs in arithmetic order
        assert st["sorts"] == H.FRAMES and st["launches_in_sorted_order"] == H.FRAMES - 2 and st["units_ordered"] == H.units_of(h, w), st
    else:
        assert st["launches_in_sorted_order"] == 0, st
    r.frames_config(0)
    r.close()


@lib_grids
def test_view_slots(grid):
    """three views per call; call j shows slot s the walk's frame j + s, so the cameras move through the slots one per call and no
    slot sees a camera twice running"""
    slots = _planes("views")
    r = _renderer(*H.VIEWS, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    for j in range(H.FRAMES):
        cs = [H.walk(LEVEL, j + s) for s in range(3)]
        sb, zb = r.trace_views(np.stack([c for c, _ in cs]), np.array([t for _, t in cs], np.float32))
        for s in range(3):
            pre, z, post = slots[s][j]
            H.same(("views", j, s), sb[s], zb[s], post, z)
    r.close()


def _viewports(r, rects, planes, j, first, what):
    """one viewport call: rectangle i is shown the walk's frame first + i, the j-th frame of its plane"""
    cs = [H.walk(LEVEL, first + i) for i in range(len(rects))]
    sb, zb = r.trace_viewports(rects, np.stack([c for c, _ in cs]), np.array([t for _, t in cs], np.float32))
    for i, (x, y, w, h) in enumerate(rects):
        pre, z, post = planes[i][j]
        H.same((what, j, i), sb[y:y + h, x:x + w], zb[y:y + h, x:x + w], post, z)


@lib_grids
def test_viewports(grid):
    W, Hh, rects = H.VIEWPORTS
    planes = _planes("viewports")
    r = _renderer(W, Hh, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    for j in range(H.FRAMES):
        _viewports(r, rects, planes, j, j, "viewports")
    r.close()


# ---------------------------------------------------------------- one sequence of mixed kinds ----

@lib_grids
def test_twelve_launches_of_six_kinds_share_the_rotation(grid):
    """a frame, a batch of 3 views, 1000 rays on a foreign stream, 65 hits, a viewport call, a device strip on the foreign stream --
    twice, the walk going on: launch n is shown the walk's frame n.  The launches on the foreign stream leave the rotation over
    the context's streams, so the launcher has to order them (launch_order_waits)."""
    import torch
    import pwnfps_amd
    W, Hh, rects = H.VIEWPORTS
    planes = _planes("mixed")
    frame, slots, vps = planes[0], planes[1:4], planes[4:]
    strip = (5, 99)
    assert strip[0] % 4 and strip[1] % 4 and not strip[0] <= Hh // 2 < strip[1]
    rng = np.random.default_rng(20261019)
    r = _renderer(W, Hh, env=LIB_GRIDS[grid])
    r.set_blur_passes(1)
    r.set_call_strips(0)
    foreign = torch.cuda.Stream()
    assert r.launch_order_waits() == 0
    n = 0
    for cycle in range(2):
        # a frame
        assert n == H.MIXED_CYCLE * cycle
        cam, sec = H.walk(LEVEL, n)
        sb, zb = r.trace_screen_centred(cam, sec)
        H.same(("mixed frame", n), sb, zb, frame[cycle][2], frame[cycle][1])
        n += 1
        # a batch of 3 views
        cs = [H.walk(LEVEL, n + s) for s in range(3)]
        sb, zb = r.trace_views(np.stack([c for c, _ in cs]), np.array([t for _, t in cs], np.float32))
        for s in range(3):
            H.same(("mixed views", n, s), sb[s], zb[s], slots[s][cycle][2], slots[s][cycle][1])
        n += 1
        # 1000 rays of the walk's frame on a stream that is not the context's, into poisoned planes
        cam, sec = H.walk(LEVEL, n)
        want_sb, want_z, _ = H.poisoned_rows(LEVEL, W, Hh, n, 0, Hh)
        pick = rng.choice(W * Hh, 1000, replace=False)
        xy = np.stack([pick % W, pick // W], 1).astype(np.int32)
        rays, seeds, _ = pwnfps_amd.pixel_rays(W, Hh, cam, xy)
        t_rays = torch.from_numpy(rays).cuda()
        t_seeds = torch.from_numpy(seeds.view(np.int32)).cuda()
        t_col = torch.full((1000,), H.POISON_S, dtype=torch.int32, device="cuda")
        t_z = torch.full((1000,), H.POISON_Z, dtype=torch.int32, device="cuda").view(torch.float32)
        torch.cuda.synchronize()
        r.trace_rays_device(t_rays, t_col, t_z, t_seeds, sec, stream=foreign)
        torch.cuda.synchronize()
        H.same(("mixed rays", n), t_col.cpu().numpy(), t_z.cpu().numpy(), want_sb[xy[:, 1], xy[:, 0]], want_z[xy[:, 1], xy[:, 0]])
        n += 1
        # 65 hits: none exactly where the oracle's depth keeps the poison, elsewhere the oracle's distance
        cam, sec = H.walk(LEVEL, n)
        _, want_z, _ = H.poisoned_rows(LEVEL, W, Hh, n, 0, Hh)
        pick = rng.choice(W * Hh, 65, replace=False)
        xy = np.stack([pick % W, pick // W], 1).astype(np.int32)
        rays, _, _ = pwnfps_amd.pixel_rays(W, Hh, cam, xy)
        hits = r.trace_hits(rays)
        wz = want_z[xy[:, 1], xy[:, 0]]
        assert ((hits["kind"] == 0) == (wz == H.POISON_Z)).all(), ("mixed hits", n)
        assert (H.bits(hits["dist"])[hits["kind"] != 0] == wz[hits["kind"] != 0]).all(), ("mixed hits", n)
        assert (hits["kind"] != 0).any()
        n += 1
        # a viewport call
        _viewports(r, rects, vps, cycle, n, "mixed viewports")
        n += 1
        # a strip of device rows on the foreign stream
        _rows_launch(r, torch, W, Hh, n, strip[0], strip[1], "mixed strip", stream=foreign.cuda_stream)
        n += 1
    assert n == 12
    assert r.launch_order_waits() > 0, r.launch_order_waits()
    r.close()
