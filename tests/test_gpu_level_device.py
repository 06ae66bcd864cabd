"""pwn_upload_level_device on the GPU.  Two contexts of 40 x 26: `a`, the ruler, is fed by pwn_upload_level or pwn_level_load_mem plus
pwn_upload_spheres; `b`, the subject, by pwn_upload_level_device plus pwn_upload_spheres_device.  Given tables, derived tables,
refused tables, hostile bytes in guarded allocations, the loop on one stream and the ordering across streams, the C entries'
refusals, the Python wrapper's rules.  The smallest sizes that still cross a wave and a workgroup boundary: 4 cameras, 257 rays,
256 players x 20 ticks."""
import ctypes as C

import numpy as np
import pytest

import baked_scenes as bs
import hard_scenes
import level_device_cases as lc
from conftest import level_path

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
W, H = 40, 26
F = np.float32
NRAYS, NPLAYERS, NTICKS = 257, 256, 20


def _dev():
    import torch
    return torch.device("cuda", 0)


def _dtype():
    import pwnfps_amd
    return pwnfps_amd.SPHERE_DTYPE


def _same(got, want, what):
    g, w = (np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in (got, want))
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d bytes differ, first at %d" % (what, len(bad), int(bad[0][0]))


_state = {}


def _pair():
    """the ruler and the subject, kept for the module; both start on the shipped level"""
    import pwnfps_amd
    if "pair" not in _state:
        rs = []
        for _ in range(2):
            r = pwnfps_amd.Renderer(W, H)
            r.level_load(level_path("pwnfps_level"))
            rs.append(r)
        _state["pair"] = tuple(rs)
    for r in _state["pair"]:
        r.set_blur_passes(1)
        r.set_counters(False)
        r.set_scheduler("units")
    return _state["pair"]


@pytest.fixture(scope="module", autouse=True)
def _close_pair():
    yield
    for r in _state.pop("pair", ()):
        r.close()
    _state.clear()


def _random_levels():
    if "random" not in _state:
        _state["random"] = lc.random_levels()
        lc.both_kinds_occur(_state["random"])
    return _state["random"]


def _grid_t(data):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(data, np.uint8).copy()).to(_dev())
    assert t.data_ptr() % 16 == 0
    return t


def _pmap_t(pmap):
    import torch
    if pmap is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(pmap, np.int32).copy()).to(_dev())
    assert t.data_ptr() % 16 == 0
    return t


def _spheres_t(spheres):
    import torch
    s = np.ascontiguousarray(spheres, _dtype())
    return torch.from_numpy(s.view(np.int32).reshape(len(s), 8).copy()).to(_dev()).view(torch.float32)


def _feed(a, b, data, pmap, spheres, derive=False):
    """the same level and spheres into both: the ruler through the host, the subject through the device"""
    s = np.ascontiguousarray(spheres, _dtype())
    if derive:
        a.level_load_text(np.ascontiguousarray(data, np.uint8).tobytes())
    else:
        a.upload_level(data, pmap)
    a.set_objects(s)
    b.upload_level_device(_grid_t(data), None if derive else _pmap_t(pmap))
    b.upload_spheres_device(_spheres_t(s), 64 * len(s) + 16)
    assert b.spheres_device_state()["reason"] == 0


def _no_spheres():
    return np.zeros(0, _dtype())


def _cams():
    """four cameras: in the grid's middle, near two corners, and outside the grid looking in"""
    return np.stack([bs._cam(32.4, 0.5, 32.6, 0.3, 0.0), bs._cam(3.5, 1.4, 2.5, 2.2, 0.1), bs._cam(60.5, 0.6, 61.5, 4.0, -0.1),
                     bs._cam(-2.5, 1.45, 70.25, 2.4, 0.02)]).reshape(4, 16).astype(F)


def _players():
    if "players" not in _state:
        rng = np.random.default_rng(77)
        cams = np.zeros((NPLAYERS, 16), F)
        cams[:, 0] = cams[:, 5] = cams[:, 10] = cams[:, 15] = 1.0
        cams[:, 12] = rng.uniform(0.5, 63.5, NPLAYERS)
        cams[:, 13] = rng.uniform(0.4, 1.9, NPLAYERS)
        cams[:, 14] = rng.uniform(0.5, 63.5, NPLAYERS)
        _state["players"] = (rng.integers(0, 256, NPLAYERS).astype(np.uint8), cams, np.zeros((NPLAYERS, 4), F), np.zeros(NPLAYERS, np.int32))
    return _state["players"]


def _compare_all(a, b, what, cams=None, sec=0.5):
    """every call family on both contexts, the subject's words against the ruler's"""
    import pwnfps_amd
    cams = _cams() if cams is None else cams
    cams4 = cams.copy()
    cams4[:, 3] = 0.125          # w components: the 4-lane kernels
    for cc, lanes in ((cams, 3), (cams4, 4)):
        for x, y, nm in zip(a.trace_view_hits(cc), b.trace_view_hits(cc), ("label", "cell", "dist")):
            _same(y, x, "%s: view hits %s, %d-lane" % (what, nm, lanes))
    secs = np.array([sec + 0.25 * i for i in range(len(cams))], F)
    for blur in (0, 1):
        a.set_blur_passes(blur)
        b.set_blur_passes(blur)
        for x, y, nm in zip(a.trace_views(cams, secs), b.trace_views(cams, secs), ("colour", "depth")):
            _same(y, x, "%s: views %s, blur %d" % (what, nm, blur))
    rays = np.concatenate([pwnfps_amd.pixel_rays(W, H, cams[i])[0][i::4] for i in range(len(cams))])[:NRAYS]
    assert len(rays) == NRAYS
    _same(b.trace_hits(rays), a.trace_hits(rays), what + ": hit records")
    reach = np.random.default_rng(5).uniform(0.3, 40.0, NRAYS).astype(F)
    _same(b.trace_reach(rays, reach), a.trace_reach(rays, reach), what + ": reach records")
    for x, y, nm in zip(a.trace_screen_centred(cams[0], sec), b.trace_screen_centred(cams[0], sec), ("colour", "depth")):
        _same(y, x, "%s: blocking frame %s" % (what, nm))
    keys, pc, pg, pt = _players()
    for x, y, nm in zip(a.players_step(keys, pc, pg, pt, ticks=NTICKS), b.players_step(keys, pc, pg, pt, ticks=NTICKS), ("cameras", "gravity", "traversals")):
        _same(y, x, "%s: players' %s" % (what, nm))
    st = []
    for r in (a, b):
        r.set_counters(True)
        r.trace_screen_centred(cams[1], sec)
        st.append(hard_scenes.stats5(r.stats()))
        r.set_counters(False)
    assert st[0] == st[1], "%s: counters %s / %s" % (what, st[0], st[1])


def _nrec(data, pmap):
    """endpoint records of a taken table: letter cells at an endpoint of their paired letter"""
    n = 0
    for z, x in np.argwhere((data >= ord('A')) & (data <= ord('Z'))):
        x1, z1, x2, z2 = (int(v) for v in pmap[int(data[z, x]) - ord('A'), :4])
        n += x2 != -1 and ((x1, z1) == (x, z) or (x2, z2) == (x, z))
    return n


# ---------------------------------------------------------------- 1: given tables ----

@pytest.mark.parametrize("kind", range(lc.NKINDS))
def test_table_of_a_random_level_taken_or_refused(kind):
    """the 48 hostile levels of the corpus, 37 taken and 11 refused: which is which is the corpus' own rule"""
    name, data, pm, taken = _random_levels()[kind]
    assert taken == (lc.expected_verdict(data, pm)[0] == 0)
    if not taken:
        _refused(name, data, pm, kind)
        return
    a, b = _pair()
    rng = np.random.default_rng(kind)
    s = np.zeros(5, _dtype())
    for i in range(5):
        s[i] = (rng.uniform(0.05, 0.3), rng.choice([0.0, 0.5]), 32 + rng.uniform(-3, 3), rng.uniform(0.2, 1.8), 32 + rng.uniform(-3, 3), *rng.uniform(0, 1, 3))
    before = b.level_device_state()["uploads"]
    _feed(a, b, data, pm, s)
    st = b.level_device_state()
    assert st == dict(in_force=1, uploads=before + 1, verdict=0, letter=26, records=_nrec(data, pm), paired=int(((pm[:, 0] != -1) & (pm[:, 2] != -1)).sum()), derived=0), (name, st)
    got = b.get_level_device()
    _same(got[0], data, name + ": the cells back")
    _same(got[1], pm, name + ": the table back")
    _compare_all(a, b, name)


def _scenes():
    if "scenes" not in _state:
        _state["scenes"] = bs.scenes(_dtype())
    return _state["scenes"]


@pytest.mark.parametrize("i", range(14))
def test_given_table_of_a_hand_made_scene(i):
    scs = _scenes()
    assert len(scs) == 14
    sc = scs[i]
    a, b = _pair()
    _feed(a, b, sc.data, sc.pmap, sc.spheres)
    assert b.level_device_state()["verdict"] == 0
    got = b.get_level_device()
    _same(got[0], sc.data, sc.name + ": the cells back")
    _same(got[1], sc.pmap, sc.name + ": the table back")
    # the scene's own camera among the four, at the scene's own time
    cams = _cams()
    cams[0] = sc.cam.reshape(16)
    _compare_all(a, b, sc.name, cams, float(sc.sec))


# ---------------------------------------------------------------- 2: derived tables ----

def _derived_cases():
    return ["pwnfps_level", "synth64", "synth256"] + [n for n, _ in lc.derived_grids()]


@pytest.mark.parametrize("name", _derived_cases())
def test_derived_table(name):
    import pwnfps_amd
    a, b = _pair()
    grids = dict(lc.derived_grids())
    if name in grids:
        data = grids[name]
    else:
        # the shipped level's grid as the library stores it
        r = pwnfps_amd.Renderer(W, H)
        r.level_load(level_path(name))
        data = r.get_level()[0]
        r.close()
    _feed(a, b, data, None, _no_spheres(), derive=True)
    want = a.get_level()
    _same(want[0], data, name + ": full rows need no line end")
    st = b.level_device_state()
    assert st["verdict"] == 0 and st["derived"] == 1 and st["in_force"] == 1 and st["letter"] == 26, (name, st)
    assert st["paired"] == int(((want[1][:, 0] != -1) & (want[1][:, 2] != -1)).sum()) and st["records"] == _nrec(data, want[1])
    got = b.get_level_device()
    _same(got[0], data, name + ": the cells back")
    _same(got[1], want[1], name + ": all 26 x 7 words of the table")
    _same(got[1], lc.derive_table(data), name + ": the table, restated")
    _compare_all(a, b, name)


# ---------------------------------------------------------------- 3: refused tables ----

@pytest.mark.parametrize("k", range(7))
def test_refused_table_leaves_the_level_in_force(k):
    name, data, pm = lc.refused_tables()[k]
    _refused(name, data, pm, k)


def _refused(name, data, pm, k):
    case = (name, k)
    a, b = _pair()
    # the level in force: the hall, device-built for the even cases and the host's for the odd ones
    hall = _scenes()[0]
    a.upload_level(hall.data, hall.pmap)
    a.set_objects(_no_spheres())
    if case[1] & 1:
        b.upload_level(hall.data, hall.pmap)
        b.set_objects(hall.spheres)
    else:
        b.upload_level_device(_grid_t(hall.data), _pmap_t(hall.pmap))
        b.upload_spheres_device(_spheres_t(hall.spheres), 4096)
    verdict, letter = lc.expected_verdict(data, pm)
    assert verdict != 0
    b.upload_level_device(_grid_t(data), _pmap_t(pm))
    st = b.level_device_state()
    assert (st["verdict"], st["letter"], st["records"], st["derived"]) == (verdict, letter, 0, 0), (name, st)
    assert st["in_force"] == (0 if case[1] & 1 else 1)
    if not case[1] & 1:
        got = b.get_level_device()
        _same(got[0], hall.data, name + ": still the hall's cells")
        _same(got[1], hall.pmap, name + ": still the hall's table")
    assert b.spheres_device_state()["in_force"] == 1 and b.sphere_tables()["form"] == 2
    cams = _cams()
    cams[0] = hall.cam.reshape(16)
    _compare_all(a, b, name + ": the hall without spheres", cams)
    # a taken level afterwards works
    sc = _scenes()[2]
    _feed(a, b, sc.data, sc.pmap, sc.spheres)
    assert b.level_device_state()["verdict"] == 0 and b.level_device_state()["in_force"] == 1
    for x, y, nm in zip(a.trace_view_hits(cams), b.trace_view_hits(cams), ("label", "cell", "dist")):
        _same(y, x, "%s: afterwards, view hits %s" % (name, nm))


# ---------------------------------------------------------------- 4: hostile bytes ----

def _guarded(arr, torch_dtype):
    """the array in the middle of an allocation whose other elements are poison: (view, whole, offset)"""
    import torch
    a = np.ascontiguousarray(arr)
    n = a.size
    pad = 256 // a.itemsize
    whole = torch.full((n + 2 * pad,), 0x5b if a.itemsize == 1 else 0x5b5b5b5b, dtype=torch_dtype, device=_dev())
    whole[pad:pad + n] = torch.from_numpy(a.reshape(-1).copy()).to(_dev())
    view = whole[pad:pad + n].view(a.shape)
    assert view.data_ptr() % 16 == 0
    return view, whole, pad


@pytest.mark.parametrize("what", ["all_bytes_derived", "all_bytes_hostile_table"] + [n for n, _, _ in lc.hostile_coordinate_tables()])
def test_hostile_bytes_in_guarded_allocations(what):
    import torch
    a, b = _pair()
    hall = _scenes()[0]
    a.upload_level(hall.data, hall.pmap)
    a.set_objects(_no_spheres())
    b.upload_level_device(_grid_t(hall.data), _pmap_t(hall.pmap))
    tables = dict((n, (d, p)) for n, d, p in lc.hostile_coordinate_tables())
    if what == "all_bytes_derived":
        data, pm = lc.all_bytes_grid(), None
    elif what == "all_bytes_hostile_table":
        data, pm = lc.all_bytes_grid(), tables["all_hostile"][1]
    else:
        data, pm = tables[what]
    gd, gd_all, dpad = _guarded(data, torch.uint8)
    gp = gp_all = None
    if pm is not None:
        gp, gp_all, ppad = _guarded(pm, torch.int32)
    b.upload_level_device(gd, gp)
    st = b.level_device_state()
    torch.cuda.synchronize()
    # the guards and the inputs themselves as they were
    whole = gd_all.cpu().numpy()
    assert (whole[:dpad] == 0x5b).all() and (whole[-dpad:] == 0x5b).all() and (whole[dpad:-dpad] == data.reshape(-1)).all()
    if pm is not None:
        whole = gp_all.cpu().numpy()
        assert (whole[:ppad] == 0x5b5b5b5b).all() and (whole[-ppad:] == 0x5b5b5b5b).all() and (whole[ppad:-ppad] == pm.reshape(-1)).all()
    cams = _cams()
    cams[0] = hall.cam.reshape(16)
    if pm is None:
        # every byte value is a cell like any other: the ruler takes the same cells with the table the rules derive from them
        assert (st["verdict"], st["letter"], st["derived"], st["in_force"]) == (0, 26, 1, 1), st
        want = lc.derive_table(data)
        _same(b.get_level_device()[1], want, what + ": the derived table")
        a.upload_level(data, want)
        _compare_all(a, b, what)
    else:
        assert (st["verdict"], st["letter"]) == lc.expected_verdict(data, pm) and st["verdict"] == 1 and st["in_force"] == 1, st
        _same(b.get_level_device()[1], hall.pmap, what + ": still the hall's table")
        _compare_all(a, b, what + ": the hall still", cams)


# ---------------------------------------------------------------- 5: the loop and the ordering ----

def _observe_device(r, cams_t, stream):
    import torch
    n = cams_t.shape[0]
    label = torch.zeros((n, H, W), dtype=torch.int32, device=_dev())
    cell = torch.zeros((n, H, W), dtype=torch.int32, device=_dev())
    dist = torch.zeros((n, H, W), dtype=torch.float32, device=_dev())
    r.trace_view_hits_device(cams_t, label, cell, dist, stream=stream)
    return label, cell, dist


def test_the_loop_on_one_stream_equals_the_host_driven_sequence():
    import torch
    a, b = _pair()
    scs = _scenes()
    A, B = scs[0], scs[9]
    assert not (A.data == B.data).all()
    keys, pc, pg, pt = _players()
    s = torch.cuda.Stream(_dev())
    # everything the subject needs, up before the loop starts
    dev = [(_grid_t(x.data), _pmap_t(x.pmap), _spheres_t(x.spheres)) for x in (A, B)]
    k_t = torch.from_numpy(keys.copy()).to(_dev())
    c_t, g_t, t_t = (torch.from_numpy(x.copy()).to(_dev()) for x in (pc, pg, pt))
    torch.cuda.synchronize()
    seen = []
    with torch.cuda.stream(s):
        for d, p, sp in dev:
            b.upload_level_device(d, p, stream=s)
            b.upload_spheres_device(sp, 4096, stream=s)
            b.players_step_device(k_t, c_t, g_t, t_t, ticks=NTICKS, stream=s)
            seen.append(_observe_device(b, c_t[:4].clone(), s) + (c_t.clone(), g_t.clone(), t_t.clone()))
    s.synchronize()          # the first host wait
    cams, grav, trav = pc, pg, pt
    for x, got in zip((A, B), seen):
        a.upload_level(x.data, x.pmap)
        a.set_objects(x.spheres)
        cams, grav, trav = a.players_step(keys, cams, grav, trav, ticks=NTICKS)
        want = a.trace_view_hits(cams[:4])
        for w_, g_, nm in zip(want + (cams, grav, trav), got, ("label", "cell", "dist", "cameras", "gravity", "traversals")):
            _same(g_.cpu().numpy(), w_, "%s: %s" % (x.name, nm))
    assert b.level_device_state()["uploads"] >= 2


def test_a_launch_queued_before_level_changes_keeps_its_level():
    import torch
    a, b = _pair()
    scs = _scenes()
    A, others = scs[0], [scs[9], scs[2], scs[12], scs[9]]
    _feed(a, b, A.data, A.pmap, A.spheres)
    n = 256
    cams = np.tile(_cams(), (n // 4, 1))
    cams[:, 12] += np.linspace(0, 1, n, dtype=F)
    want = a.trace_view_hits(cams)
    dev = [(_grid_t(x.data), _pmap_t(x.pmap)) for x in others]
    cams_t = torch.from_numpy(cams).to(_dev())
    s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    torch.cuda.synchronize()
    planes = []
    for _ in range(3):          # a queue of launches that read copy k of the tables ...
        label = torch.zeros((n, H, W), dtype=torch.int32, device=_dev())
        cell = torch.zeros((n, H, W), dtype=torch.int32, device=_dev())
        dist = torch.zeros((n, H, W), dtype=torch.float32, device=_dev())
        b.trace_view_hits_device(cams_t, label, cell, dist, stream=s1)
        planes.append((label, cell, dist))
    for d, p in dev:            # ... while four level uploads on another stream go round to that copy
        b.upload_level_device(d, p, stream=s2)
    torch.cuda.synchronize()
    for got in planes:
        for w_, g_, nm in zip(want, got, ("label", "cell", "dist")):
            _same(g_.cpu().numpy(), w_, "queued before the level changes: " + nm)
    # and what is launched now reads the last level
    a.upload_level(others[-1].data, others[-1].pmap)
    a.set_objects(_no_spheres())
    for x, y, nm in zip(a.trace_view_hits(cams[:4]), b.trace_view_hits(cams[:4]), ("label", "cell", "dist")):
        _same(y, x, "after the level changes: " + nm)


def test_a_step_on_a_second_stream_is_held_back_across_a_level_change():
    import torch
    a, b = _pair()
    scs = _scenes()
    A, B = scs[0], scs[9]
    _feed(a, b, A.data, A.pmap, _no_spheres())
    keys, pc, pg, pt = _players()
    k_t = torch.from_numpy(keys.copy()).to(_dev())
    c_t, g_t, t_t = (torch.from_numpy(x.copy()).to(_dev()) for x in (pc, pg, pt))
    d, p = _grid_t(B.data), _pmap_t(B.pmap)
    s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
    torch.cuda.synchronize()
    b.players_step_device(k_t, c_t, g_t, t_t, ticks=NTICKS, stream=s2)          # level A
    s2.synchronize()
    b.upload_level_device(d, p, stream=s1)
    b.players_step_device(k_t, c_t, g_t, t_t, ticks=NTICKS, stream=s2)          # level B, though nothing has waited for s1
    torch.cuda.synchronize()
    cams, grav, trav = a.players_step(keys, pc, pg, pt, ticks=NTICKS)
    a.upload_level(B.data, B.pmap)
    cams, grav, trav = a.players_step(keys, cams, grav, trav, ticks=NTICKS)
    for w_, g_, nm in zip((cams, grav, trav), (c_t, g_t, t_t), ("cameras", "gravity", "traversals")):
        _same(g_.cpu().numpy(), w_, "a step on a second stream: " + nm)


def test_a_host_upload_puts_the_hosts_level_back():
    a, b = _pair()
    scs = _scenes()
    A, B = scs[0], scs[9]
    a.upload_level(A.data, A.pmap)
    b.upload_level(A.data, A.pmap)
    for r in (a, b):
        r.set_objects(A.spheres)
    host = b.get_level()
    b.upload_level_device(_grid_t(B.data), _pmap_t(B.pmap))
    b.upload_spheres_device(_spheres_t(B.spheres), 4096)
    assert b.level_device_state()["in_force"] == 1
    for x, y in zip(host, b.get_level()):
        _same(y, x, "pwn_get_level goes on describing the host's level")
    b.set_objects(A.spheres)          # pwn_upload_spheres: the host's level and the host's spheres
    assert b.level_device_state()["in_force"] == 0 and b.spheres_device_state()["in_force"] == 0
    with pytest.raises(Exception):
        b.get_level_device()
    for x, y in zip(host, b.get_level()):
        _same(y, x, "pwn_get_level never changed")
    cams = _cams()
    cams[0] = A.cam.reshape(16)
    _compare_all(a, b, "the host's level again", cams)
    # and a device build of spheres after that builds over the HOST's level
    b.upload_spheres_device(_spheres_t(A.spheres), 4096)
    _compare_all(a, b, "device spheres over the host's level", cams)


# ---------------------------------------------------------------- 6: refusals of the C entries ----

def test_refusals_leave_the_level():
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    a, b = _pair()
    sc = _scenes()[0]
    _feed(a, b, sc.data, sc.pmap, sc.spheres)
    d, p = _grid_t(sc.data), _pmap_t(sc.pmap)
    st0, sp0 = b.level_device_state(), b.spheres_device_state()
    dp, pp = d.data_ptr(), p.data_ptr()
    for args in ((None, dp, pp), (b._ctx, None, pp), (b._ctx, None, None), (b._ctx, dp + 4, pp), (b._ctx, dp + 8, None), (b._ctx, dp, pp + 4)):
        assert L.pwn_upload_level_device(*args, None) == PWN_EINVAL, args
    assert L.pwn_level_device_state(None, (C.c_uint64 * 8)()) == PWN_EINVAL and L.pwn_level_device_state(b._ctx, None) == PWN_EINVAL
    bare = pwnfps_amd.Renderer(W, H)
    assert L.pwn_upload_level_device(bare._ctx, dp, pp, None) == PWN_ENOLEVEL and L.pwn_upload_level_device(bare._ctx, dp, None, None) == PWN_ENOLEVEL
    assert bare.level_device_state() == dict.fromkeys(("in_force", "uploads", "verdict", "letter", "records", "paired", "derived"), 0)
    assert L.pwn_get_level_device(bare._ctx, None, None) == PWN_EINVAL
    bare.close()
    g = pwnfps_amd.Renderer(W, H, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert L.pwn_upload_level_device(g._ctx, dp, pp, None) == PWN_ENOTSUP
    assert L.pwn_level_device_state(g._ctx, (C.c_uint64 * 8)()) == PWN_ENOTSUP and L.pwn_get_level_device(g._ctx, None, None) == PWN_ENOTSUP
    g.close()
    r = pwnfps_amd.Renderer(W, H)
    r.level_load(level_path("pwnfps_level"))
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert L.pwn_upload_level_device(r._ctx, dp, pp, None) == PWN_EBUSY
    r.tiled_shutdown()
    r.close()
    assert b.level_device_state() == st0 and b.spheres_device_state() == sp0
    cams = _cams()
    cams[0] = sc.cam.reshape(16)
    _compare_all(a, b, "after the refusals", cams)


# ---------------------------------------------------------------- 7: the Python rules ----

class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


@pytest.mark.parametrize("what", ["dtype", "shape", "flat", "strided", "misaligned", "cpu", "pmap_dtype", "pmap_shape", "pmap_misaligned", "pmap_cpu", "pmap_numpy"])
def test_python_refuses_before_the_library_is_entered(monkeypatch, what):
    import pwnfps_amd
    import torch
    from pwnfps_amd import render
    monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = W, H, 0, C.c_void_p()
    dev = _dev()
    good = torch.zeros((64, 64), dtype=torch.uint8, device=dev)
    cases = {
        "dtype": (torch.zeros((64, 64), dtype=torch.int8, device=dev), None),
        "shape": (torch.zeros((64, 65), dtype=torch.uint8, device=dev), None),
        "flat": (torch.zeros((4096,), dtype=torch.uint8, device=dev), None),
        "strided": (torch.zeros((64, 128), dtype=torch.uint8, device=dev)[:, ::2], None),
        "misaligned": (torch.zeros((4096 + 16,), dtype=torch.uint8, device=dev)[1:4097].view(64, 64), None),
        "cpu": (torch.zeros((64, 64), dtype=torch.uint8), None),
        "pmap_dtype": (good, torch.zeros((26, 7), dtype=torch.int64, device=dev)),
        "pmap_shape": (good, torch.zeros((7, 26), dtype=torch.int32, device=dev)),
        "pmap_misaligned": (good, torch.zeros((26 * 7 + 4,), dtype=torch.int32, device=dev)[1:183].view(26, 7)),
        "pmap_cpu": (good, torch.zeros((26, 7), dtype=torch.int32)),
        "pmap_numpy": (good, np.zeros((26, 7), np.int32)),
    }
    data, pmap = cases[what]
    with pytest.raises(ValueError) as e:
        r.upload_level_device(data, pmap)
    assert str(e.value).startswith("upload_level_device: ")
