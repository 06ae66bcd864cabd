"""pwn_upload_spheres_device on the GPU.  Every case uses two contexts on one level: `a` is fed by pwn_upload_spheres and is the
ruler, `b` by the device call.  The state words against pwn_sphere_tables_plan; every call family bit for bit; the capacity rules;
step -> spheres -> tables -> observation for ten ticks on one stream and on two; launches made before a build keep their tables;
who owns the tables; refusals; the Python wrapper's rules."""
import ctypes as C

import numpy as np
import pytest

import big_scenes
import hard_scenes
from conftest import level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_ETOOBIG, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -7, -8, -9
PWN_LIST_MAX = 4096
W, H = 64, 32
F = np.float32


def _dev():
    import torch
    return torch.device("cuda", 0)


def _dtype():
    import pwnfps_amd
    return pwnfps_amd.SPHERE_DTYPE


def _bits(a):
    """the array's bytes, whatever its dtype and shape (an int16 pair and an int32 word of a cell plane compare as what they are)"""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d bytes differ, first at %d" % (what, len(bad), int(bad[0][0]))


def _tensor(spheres):
    """the records as an (n,8) float32 GPU tensor, bit for bit"""
    import torch
    s = np.ascontiguousarray(spheres, _dtype())
    t = torch.from_numpy(s.view(np.int32).reshape(len(s), 8).copy()).to(_dev()).view(torch.float32)
    assert len(s) == 0 or t.data_ptr() % 16 == 0
    return t


def _plan(spheres):
    """(pairs, cells, longest) of pwn_sphere_tables_plan, also for tables it would refuse"""
    from pwnfps_amd import _lib
    s = np.ascontiguousarray(spheres, _dtype())
    out = (C.c_uint64 * 6)()
    buf = s if len(s) else np.zeros(1, _dtype())
    rc = _lib.lib.pwn_sphere_tables_plan(buf.ctypes.data, len(s), out)
    assert rc in (0, PWN_ETOOBIG)
    return int(out[3]), int(out[4]), int(out[5])


_pairs = {}


def _pair(level="pwnfps_level", w=W, h=H):
    """the two contexts of a level (a path's stem or a level's text), kept for the module"""
    import pwnfps_amd
    key = (level, w, h)
    if key not in _pairs:
        rs = []
        for _ in range(2):
            r = pwnfps_amd.Renderer(w, h)
            if "\n" in level:
                r.level_load_text(level)
            else:
                r.level_load(level if level.endswith(".txt") else level_path(level))
            rs.append(r)
        _pairs[key] = tuple(rs)
    a, b = _pairs[key]
    for r in (a, b):
        r.set_blur_passes(1)
        r.set_counters(False)
        r.set_scheduler("units")
    return a, b


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for a, b in _pairs.values():
        a.close()
        b.close()
    _pairs.clear()


def _spawn_xz(r):
    sp = r.get_level()[2]
    return float(sp[0]) + 0.5, float(sp[1]) + 0.5


def _rand(n, seed, cx, cz, spread=3.0, rlo=0.05, rhi=0.4):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, _dtype())
    s["x"] = cx + rng.uniform(-spread, spread, n)
    s["z"] = cz + rng.uniform(-spread, spread, n)
    s["y"] = rng.uniform(0.2, 0.8, n)
    s["r"] = rng.uniform(rlo, rhi, n)
    s["refl"] = rng.uniform(0, 0.9, n)
    for c in ("cb", "cg", "cr"):
        s[c] = rng.uniform(0.1, 1.0, n)
    return s.astype(_dtype())


def hostile(cx, cz):
    """the box test's hostile values (tests/test_sphere_box.py), among a few ordinary spheres"""
    big = F(2.0 ** 31)
    vals = [np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, F(0)), np.nextafter(-big, F(0)), F(1e30), F(-1e30),
            F(1e-45), F(-1e-45), F(1e-39), F(-0.3), F(-40.0), F(1e-20), F(0.0), F(-0.0)]
    rows = []
    for v in vals:
        rows.append((v, 0.3, cx, 0.5, cz, 0.5, 0.6, 0.7))                  # a hostile radius
        rows.append((0.3, 0.3, v, 0.5, cz, 0.5, 0.6, 0.7))                 # a hostile x
        rows.append((0.3, 0.3, cx, v, cz + 1, 0.5, 0.6, 0.7))              # a hostile y
        rows.append((0.3, v, cx + 1, 0.5, v, v, 0.6, 0.7))                 # a hostile z, refl and colour
    rows += [(0.7, 0.2, -0.2, 0.5, cz, 1, 1, 1), (0.7, 0.2, 63.6, 0.5, 63.8, 1, 1, 1), (0.5, 0.2, -3.0, 0.5, cz, 1, 1, 1), (0.5, 0.2, 70.0, 0.5, 70.0, 1, 1, 1)]
    s = np.array(rows, dtype=_dtype())
    return np.concatenate([s, _rand(12, 5, cx, cz)])


def _scene_spheres(name, a):
    cx, cz = _spawn_xz(a)
    if name.startswith("n"):
        return _rand(int(name[1:]), 11 + int(name[1:]), cx, cz)
    if name == "level14":
        return np.ascontiguousarray(load_spheres("t0"), _dtype())
    if name in ("cell65", "cell130"):
        n = int(name[4:])
        s = _rand(n, 3, cx, cz, spread=0.0, rlo=0.02, rhi=0.1)
        rng = np.random.default_rng(4)
        s["x"] = np.floor(cx) + rng.uniform(0.15, 0.85, n)
        s["z"] = np.floor(cz) + 2 + rng.uniform(0.15, 0.85, n)
        return s
    if name == "whole_grid":
        return np.concatenate([np.array([(40.0, 0.3, 32.0, 0.5, 32.0, 0.2, 0.4, 0.9)], dtype=_dtype()), _rand(5, 9, cx, cz)])
    if name == "outside":
        s = _rand(40, 13, 0.0, 0.0, spread=1.5, rlo=0.3, rhi=0.9)
        t = _rand(40, 14, 64.0, 64.0, spread=1.5, rlo=0.3, rhi=0.9)
        u = _rand(10, 15, -9.0, 80.0, spread=2.0)
        return np.concatenate([s, t, u, _rand(6, 16, cx, cz)])
    if name == "hostile":
        return hostile(cx, cz)
    raise KeyError(name)


SMALL = ["n0", "n1", "n63", "n64", "n65", "n129", "level14", "cell65", "cell130", "whole_grid", "outside", "hostile"]
BIG = ["swarm_near", "swarm_all"]


def _load(name, oracle_lib=None):
    """(a, b, spheres) with the scene's level in both contexts"""
    if name in BIG:
        sc = big_scenes.scene(name, oracle_lib)
        a, b = _pair(sc.level)
        return a, b, np.ascontiguousarray(sc.spheres, _dtype())
    a, b = _pair()
    return a, b, _scene_spheres(name, a)


def _cams(r, n=3):
    import pwnfps_amd
    sp = r.get_level()[2]
    return np.stack([pwnfps_amd.spawn_camera(sp, ang_y=0.9 * i, ang_x=0.2 if i == 1 else 0.0).reshape(16) for i in range(n)]).astype(F)


def _compare_all(a, b, cams, what, frames=True):
    """every call family on both contexts, b's words against a's"""
    import pwnfps_amd
    cams4 = cams.copy()
    cams4[:, 3] = 0.125          # w components: the 4-lane kernels
    for cc, lanes in ((cams, 3), (cams4, 4)):
        for x, y, nm in zip(a.trace_view_hits(cc), b.trace_view_hits(cc), ("label", "cell", "dist")):
            _same(y, x, "%s: view hits %s, %d-lane" % (what, nm, lanes))
    secs = np.array([0.25 * i for i in range(len(cams))], F)
    for blur in (0, 1):
        a.set_blur_passes(blur)
        b.set_blur_passes(blur)
        for x, y, nm in zip(a.trace_views(cams, secs), b.trace_views(cams, secs), ("colour", "depth")):
            _same(y, x, "%s: views %s, blur %d" % (what, nm, blur))
    rays, _, _ = pwnfps_amd.pixel_rays(a.w, a.h, cams[1])
    _same(b.trace_hits(rays), a.trace_hits(rays), what + ": hit records")
    if not frames:
        return
    for x, y, nm in zip(a.trace_screen_centred(cams[0], 0.5), b.trace_screen_centred(cams[0], 0.5), ("colour", "depth")):
        _same(y, x, "%s: blocking frame %s" % (what, nm))
    got = []
    for r in (a, b):
        r.frames_config(2, sbuf=True, zbuf=True)
        r.submit_frame(cams[2], 0.75, 0)
        fr = r.wait_frame(0)
        got.append((fr["sbuf"].copy(), fr["zbuf"].copy()))
        r.frames_config(0)
    _same(got[1][0], got[0][0], what + ": frame in flight colour")
    _same(got[1][1], got[0][1], what + ": frame in flight depth")
    st = []
    for r in (a, b):
        r.set_counters(True)
        r.trace_screen_centred(cams[1], 0.5)
        st.append(hard_scenes.stats5(r.stats()))
        r.set_counters(False)
    assert st[0] == st[1], "%s: counters %s / %s" % (what, st[0], st[1])


# ---------------------------------------------------------------- 1: the state against the plan ----

@pytest.mark.parametrize("name", SMALL + BIG)
def test_state_is_the_plans(name, oracle_lib):
    a, b, s = _load(name, oracle_lib)
    pairs, cells, longest = _plan(s)
    before = b.spheres_device_state()["uploads"]
    b.upload_spheres_device(_tensor(s), pairs + 17)
    st = b.spheres_device_state()
    assert (st["pairs"], st["cells"], st["longest"]) == (pairs, cells, longest), (name, st)
    assert st["in_force"] == 1 and st["n"] == len(s) and st["max_pairs"] == pairs + 17 and st["reason"] == 0 and st["uploads"] == before + 1
    t = b.sphere_tables()
    assert t["form"] == 2 and (t["pairs"], t["cells"], t["longest"]) == (pairs + 17, min(4096, pairs + 17), min(PWN_LIST_MAX, pairs + 17))
    if name in BIG:
        assert len(s) >= 2048


# ---------------------------------------------------------------- 2: results ----

@pytest.mark.parametrize("name", SMALL + BIG)
def test_every_call_family_returns_the_hosts_bits(name, oracle_lib):
    a, b, s = _load(name, oracle_lib)
    pairs = _plan(s)[0]
    a.set_objects(s)
    b.upload_spheres_device(_tensor(s), pairs)          # (capacity equal to the pairs: built)
    assert b.spheres_device_state()["reason"] == 0
    _compare_all(a, b, _cams(a), name)


def _hard():
    return [sc for sc in hard_scenes.scenes(_dtype()) if len(sc.spheres) > 0]


def test_hard_scenes_with_spheres():
    """the sphere-bearing scenes of tests/hard_scenes.py at their own sizes: view hits, the scene's own frame with and without blur
    and its five counters; then every call family, where the width allows the views' blur"""
    scs = _hard()
    assert len(scs) >= 3
    for sc in scs:
        a, b = _pair(sc.level, sc.w, sc.h)
        s = np.ascontiguousarray(sc.spheres, _dtype())
        a.set_objects(s)
        b.upload_spheres_device(_tensor(s), _plan(s)[0] + 5)
        cam = sc.cam.reshape(1, 16)
        for x, y, nm in zip(a.trace_view_hits(cam), b.trace_view_hits(cam), ("label", "cell", "dist")):
            _same(y, x, "%s: view hits %s" % (sc.name, nm))
        for blur in ((0, 1) if sc.blur_ok else (0,)):
            st = []
            for r in (a, b):
                r.set_blur_passes(blur)
                r.set_counters(True)
                st.append(r.trace_screen_centred(sc.cam, sc.sec) + (hard_scenes.stats5(r.stats()),))
                r.set_counters(False)
            _same(st[1][0], st[0][0], "%s: colour, blur %d" % (sc.name, blur))
            _same(st[1][1], st[0][1], "%s: depth, blur %d" % (sc.name, blur))
            assert st[0][2] == st[1][2], sc.name
        if sc.blur_ok:          # (every family, as for the scenes above; the views' blur needs a width that is a multiple of four)
            _compare_all(a, b, np.stack([sc.cam.reshape(16)] * 3).astype(F), sc.name)
        _pairs.pop((sc.level, sc.w, sc.h))
        a.close()
        b.close()


# ---------------------------------------------------------------- 3: capacity ----

def test_capacity():
    a, b = _pair()
    cx, cz = _spawn_xz(a)
    s = _rand(200, 21, cx, cz, rlo=0.3, rhi=0.9)
    pairs = _plan(s)[0]
    cams = _cams(a)
    t = _tensor(s)
    # one pair short: the tables of no spheres, the full count reported
    a.set_objects(s[:0])
    b.upload_spheres_device(t, pairs - 1)
    st = b.spheres_device_state()
    assert st["reason"] == 1 and st["pairs"] == pairs and st["in_force"] == 1
    _compare_all(a, b, cams, "one pair short", frames=False)
    # room for exactly the pairs: built
    a.set_objects(s)
    b.upload_spheres_device(t, pairs)
    assert b.spheres_device_state()["reason"] == 0
    _compare_all(a, b, cams, "capacity = pairs", frames=False)
    # 4097 spheres in one cell with room to spare: a list too long, no spheres
    pile = _rand(PWN_LIST_MAX + 1, 22, cx, cz, spread=0.0, rlo=0.01, rhi=0.05)
    pile["x"] = np.floor(cx) + 0.5
    pile["z"] = np.floor(cz) + 1.5
    a.set_objects(s[:0])
    b.upload_spheres_device(_tensor(pile), 3 * PWN_LIST_MAX)
    st = b.spheres_device_state()
    assert st["reason"] == 2 and st["longest"] == PWN_LIST_MAX + 1 and st["pairs"] == PWN_LIST_MAX + 1 and st["cells"] == 1
    _compare_all(a, b, cams, "a list too long", frames=False)
    # the next fitting call builds again
    a.set_objects(s)
    b.upload_spheres_device(t, pairs + 1000)
    assert b.spheres_device_state()["reason"] == 0
    _compare_all(a, b, cams, "after the overflows", frames=False)


# ---------------------------------------------------------------- 4: the loop ----

def _loop_spheres_np(cams):
    n = len(cams)
    s = np.zeros(n, _dtype())
    s["r"] = 0.25
    s["refl"] = 0.2
    s["x"], s["y"], s["z"] = cams[:, 12], cams[:, 13], cams[:, 14]
    s["cb"], s["cg"], s["cr"] = 0.3, 0.6, 0.9
    return s


@pytest.mark.parametrize("two_streams", [False, True])
def test_ten_ticks_on_the_device(two_streams):
    """players_step_device, spheres made from the cameras in torch, upload_spheres_device, trace_view_hits_device: ten ticks, more
    than twice round the four copies, nothing waited for on the host in between; every tick's planes equal the host-driven loop's"""
    import pwnfps_amd
    import torch
    a, b = _pair()
    n, views, ticks = 96, 6, 10
    rng = np.random.default_rng(31)
    cams0, grav0, _ = pwnfps_amd.players_spawn(a.get_level()[2], n)
    for i in range(n):
        cams0[i] = pwnfps_amd.spawn_camera(a.get_level()[2], ang_y=0.07 * i).reshape(16)
    keys = rng.choice([16, 17, 18, 32, 64, 128, 0], n).astype(np.uint8)
    # the host-driven loop
    want = []
    hc, hg = cams0.copy(), grav0.copy()
    for _ in range(ticks):
        hc, hg, _t = a.players_step(keys, hc, hg, tdiff=1 / 60, ticks=3)
        hc = np.ascontiguousarray(hc, F).reshape(n, 16)
        a.set_objects(_loop_spheres_np(hc))
        want.append(a.trace_view_hits(hc[:views]))
    # the device loop
    dev = _dev()
    s1 = torch.cuda.Stream(dev)
    s2 = torch.cuda.Stream(dev) if two_streams else s1
    got = []
    with torch.cuda.stream(s1):
        d_keys = torch.from_numpy(keys).to(dev)
        d_cams = torch.from_numpy(cams0.copy()).to(dev)
        d_grav = torch.from_numpy(grav0.copy()).to(dev)
        d_sph = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        d_sph[:, 0] = 0.25
        d_sph[:, 1] = 0.2
        d_sph[:, 5], d_sph[:, 6], d_sph[:, 7] = 0.3, 0.6, 0.9
    for _ in range(ticks):
        with torch.cuda.stream(s1):
            b.players_step_device(d_keys, d_cams, d_grav, tdiff=1 / 60, ticks=3)
            d_sph[:, 2:5] = d_cams[:, 12:15]
            b.upload_spheres_device(d_sph, 4 * n)
        if two_streams:
            s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            label = torch.empty((views, H, W), dtype=torch.int32, device=dev)
            cell = torch.empty((views, H, W), dtype=torch.int32, device=dev)
            dist = torch.empty((views, H, W), dtype=torch.float32, device=dev)
            b.trace_view_hits_device(d_cams[:views], label, cell, dist)
            got.append((label, cell, dist))
        if two_streams:
            s1.wait_stream(s2)          # (the next step overwrites the cameras the observation reads)
    s1.synchronize()
    s2.synchronize()
    st = b.spheres_device_state()
    assert st["reason"] == 0 and st["n"] == n
    hit_kinds = set()
    for t in range(ticks):
        for x, y, nm in zip(want[t], got[t], ("label", "cell", "dist")):
            _same(y.cpu().numpy(), x, "tick %d: %s" % (t, nm))
        hit_kinds |= set(np.unique(pwnfps_amd.unpack_labels(want[t][0])[0]).tolist())
    assert 2 in hit_kinds, "no tick's views saw a sphere"
    assert any((_bits(want[t][0]) != _bits(want[0][0])).any() for t in range(1, ticks))


# ---------------------------------------------------------------- 5: ordering against launches ----

def test_a_launch_made_before_the_build_keeps_its_tables():
    """a views launch enqueued before the builds, behind a long launch, still shows the old spheres: it keeps its copy, and the build
    that comes round to that copy waits for it"""
    import torch
    a, b = _pair()
    cx, cz = _spawn_xz(a)
    old, new = _rand(40, 41, cx, cz), _rand(55, 42, cx, cz)
    cams = _cams(a)
    a.set_objects(old)
    want_old = a.trace_view_hits(cams)
    a.set_objects(new)
    want_new = a.trace_view_hits(cams)
    assert (_bits(want_old[0]) != _bits(want_new[0])).any()
    dev = _dev()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    d_cams = torch.from_numpy(cams).to(dev)
    t_old, t_new = _tensor(old), _tensor(new)
    big = torch.randn((4096, 4096), device=dev)
    planes = [[torch.empty((len(cams), H, W), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)] for _ in range(2)]
    torch.cuda.synchronize()
    b.upload_spheres_device(t_old, 4000, stream=s1)
    with torch.cuda.stream(s1):
        for _ in range(20):
            big = big @ big * 1e-3          # a long launch in front of the views
        b.trace_view_hits_device(d_cams, *planes[0])
    # on another stream, while s1 still works: four builds, the fourth into the very copy that the views on s1 have yet to read --
    # it waits for them on s2, the three before it wait for nothing
    for t in (t_new, t_old[:7], t_new[:9], t_new):
        b.upload_spheres_device(t, 4000, stream=s2)
    with torch.cuda.stream(s2):
        b.trace_view_hits_device(d_cams, *planes[1])
    torch.cuda.synchronize()
    for x, y, nm in zip(want_old, planes[0], ("label", "cell", "dist")):
        _same(y.cpu().numpy(), x, "enqueued before the build: " + nm)
    for x, y, nm in zip(want_new, planes[1], ("label", "cell", "dist")):
        _same(y.cpu().numpy(), x, "enqueued behind the build: " + nm)


# ---------------------------------------------------------------- 6: who owns the tables; refusals ----

def test_who_owns_the_tables():
    a, b = _pair("pwnfps_level", 48, 24)          # (contexts of its own: the two trace different numbers of frames here)
    cx, cz = _spawn_xz(a)
    host, devs = _rand(30, 51, cx, cz), _rand(45, 52, cx, cz)
    cam = _cams(a)[1]
    a.set_objects(host)
    f_host = a.trace_screen_centred(cam, 0.5)
    a.set_objects(devs)
    f_dev = a.trace_screen_centred(cam, 0.5)
    assert (_bits(f_host[0]) != _bits(f_dev[0])).any()
    t = _tensor(devs)

    def frame_is(want, what):
        got = b.trace_screen_centred(cam, 0.5)
        _same(got[0], want[0], what + ": colour")
        _same(got[1], want[1], what + ": depth")

    b.set_objects(host)
    b.set_counters(True)
    b.trace_screen_centred(cam, 0.5)
    b.set_counters(False)
    st0, waits0 = b.stats(), b.launch_order_waits()
    b.upload_spheres_device(t, 2000)
    assert b.spheres_device_state()["in_force"] == 1
    assert b.stats() == st0 and b.launch_order_waits() == waits0
    frame_is(f_dev, "device tables")
    # the host's queries go on describing the host's table
    _same(b.get_objects(), np.ascontiguousarray(host, _dtype()), "get_objects")
    assert int(b.get_bins()[0].astype(np.int64).sum()) == _plan(host)[0]
    # a scheduler change and back leaves the device tables' frame
    b.set_scheduler("refill")
    frame_is(f_dev, "under the refill scheduler")
    assert b.sphere_tables()["form"] == 2
    b.set_scheduler("units")
    frame_is(f_dev, "back under the units scheduler")
    assert b.spheres_device_state()["in_force"] == 1
    # each of the host's calls restores the host's frame
    b.level_prepare_render()
    assert b.spheres_device_state()["in_force"] == 0 and b.sphere_tables()["form"] != 2
    frame_is(f_host, "after prepare_render")
    b.upload_spheres_device(t, 2000)
    frame_is(f_dev, "device tables again")
    b.set_objects(host)
    frame_is(f_host, "after upload_spheres")
    b.upload_spheres_device(t, 2000)
    b.level_load(level_path("pwnfps_level"))
    assert b.spheres_device_state()["in_force"] == 0
    frame_is(f_host, "after a level load")
    b.upload_spheres_device(t, 2000)          # (a new base copy of the level first)
    frame_is(f_dev, "device tables after the level load")


def test_refusals_leave_the_frame():
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    a, b = _pair("pwnfps_level", 48, 24)
    cx, cz = _spawn_xz(a)
    s = _rand(20, 61, cx, cz)
    t = _tensor(s)
    cam = _cams(a)[0]
    b.upload_spheres_device(t, 500)
    before = b.trace_screen_centred(cam, 0.1)
    st0 = b.spheres_device_state()
    p = t.data_ptr()
    for args in ((None, 20, p, 500), (b._ctx, -1, p, 500), (b._ctx, 10001, p, 500), (b._ctx, 20, p, -1), (b._ctx, 20, None, 500), (b._ctx, 20, p + 4, 500), (b._ctx, 20, p + 8, 500)):
        assert L.pwn_upload_spheres_device(*args, None) == PWN_EINVAL, args
    assert L.pwn_upload_spheres_device(b._ctx, 20, p, (16 << 20) // 20 + 1, None) == PWN_ETOOBIG
    assert L.pwn_upload_spheres_device(b._ctx, 20, p, 2 ** 31 - 1, None) == PWN_ETOOBIG
    bare = pwnfps_amd.Renderer(W, H)
    assert L.pwn_upload_spheres_device(bare._ctx, 20, p, 500, None) == PWN_ENOLEVEL
    assert bare.spheres_device_state() == dict.fromkeys(("in_force", "n", "max_pairs", "pairs", "cells", "longest", "reason", "uploads"), 0)
    bare.close()
    g = pwnfps_amd.Renderer(W, H, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert L.pwn_upload_spheres_device(g._ctx, 20, p, 500, None) == PWN_ENOTSUP
    assert L.pwn_spheres_device_state(g._ctx, (C.c_uint64 * 8)()) == PWN_ENOTSUP
    g.close()
    r = pwnfps_amd.Renderer(W, H)
    r.level_load(level_path("pwnfps_level"))
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert L.pwn_upload_spheres_device(r._ctx, 20, p, 500, None) == PWN_EBUSY
    r.tiled_shutdown()
    r.close()
    assert b.spheres_device_state() == st0
    after = b.trace_screen_centred(cam, 0.1)
    _same(after[0], before[0], "after the refusals: colour")
    _same(after[1], before[1], "after the refusals: depth")


# ---------------------------------------------------------------- 7: the Python rules ----

class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


@pytest.mark.parametrize("what", ["dtype", "shape", "columns", "strided", "misaligned", "too_many", "max_pairs", "negative", "float_pairs", "cpu"])
def test_python_refuses_before_the_library_is_entered(monkeypatch, what):
    import pwnfps_amd
    import torch
    from pwnfps_amd import render
    monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = W, H, 0, C.c_void_p()
    dev = _dev()
    good = torch.zeros((6, 8), dtype=torch.float32, device=dev)
    cases = {
        "dtype": (torch.zeros((6, 8), dtype=torch.float64, device=dev), 10),
        "shape": (torch.zeros((48,), dtype=torch.float32, device=dev), 10),
        "columns": (torch.zeros((6, 7), dtype=torch.float32, device=dev), 10),
        "strided": (torch.zeros((6, 16), dtype=torch.float32, device=dev)[:, ::2], 10),
        "misaligned": (torch.zeros((7 * 8 + 1,), dtype=torch.float32, device=dev)[1:49].view(6, 8), 10),
        "too_many": (torch.zeros((10001, 8), dtype=torch.float32, device=dev), 10),
        "max_pairs": (good, 2 ** 31),
        "negative": (good, -1),
        "float_pairs": (good, 10.0),
        "cpu": (torch.zeros((6, 8), dtype=torch.float32), 10),
    }
    sph, mp = cases[what]
    with pytest.raises(ValueError):
        r.upload_spheres_device(sph, mp)
