"""pwn_trace_viewport_hits / pwn_trace_viewport_hits_device: first-hit planes (label, cell, distance) of views of their own sizes in
rectangles of one frame.  The ruler is the ray form: pixel (x, y) of rectangle i holds pack_labels, the cell word and the distance
bits of trace_hits(pixel_rays(w_i, h_i, cams[i])) for that pixel -- another mode of the trace kernel, on whatever context.  The
device context is 64 x 48 throughout and the layouts are those of tests/test_gpu_viewports_device.py (A: 96 x 40, five views not in
units order, wider than the context, uncovered area; B: 70 x 33, widths off every grid, a 1 x 1 view, ties; C64 / C332: one view).
The device form writes nothing outside the rectangles, the host form 0."""
import ctypes as C
import os

import numpy as np
import pytest

import big_scenes as BS
import test_gpu_viewports_device as VD
from conftest import GOLD, level_path, load_spheres
from test_gpu_viewports_device import A, B, LAYOUTS, CW, CH

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
POISON = 0x5a5a5a5a
GUARD = 64
NAMES = ("label", "cell", "dist")
LEVELS = [("pwnfps_level", "t0"), ("synth64", "synth64")]


def _dev():
    return VD._dev()


def _renderer(w, h, level=None, spheres=None):
    return VD._renderer(w, h, level, spheres, blur=0)


def _planes_of_hits(hits):
    """(label, cell word, dist bits) of HIT_DTYPE records"""
    import pwnfps_amd
    hits = np.ascontiguousarray(hits)
    words = hits.view(np.uint32).reshape(len(hits), 12)
    return pwnfps_amd.pack_labels(hits), words[:, 11].copy(), words[:, 4].copy()


def _ray_planes(r, layout, cams, counters=False):
    """the three planes of `layout` by the ray form on context r: (H,W) uint32 each, 0 outside the rectangles; with counters, the
    five counters summed over the rectangles' batches of rays as well"""
    import pwnfps_amd
    W, H, rects = layout
    out = [np.zeros((H, W), np.uint32) for _ in range(3)]
    total = np.zeros(5, np.int64)
    for (x, y, w, h), cam in zip(rects, np.asarray(cams, np.float32).reshape(len(rects), 4, 4)):
        rays, _, xy = pwnfps_amd.pixel_rays(w, h, cam)
        assert len(rays) == w * h
        planes = _planes_of_hits(r.trace_hits(rays))
        if counters:
            total += np.array(VD._stats5(r.stats()), np.int64)
        for o, p in zip(out, planes):
            o[y + xy[:, 1], x + xy[:, 0]] = p
    return tuple(out) + ((tuple(int(v) for v in total),) if counters else ())


_CTX = {}
_WANT = {}


def _ctx(level, key):
    """the device context of a level, 64 x 48 whatever the layout, kept for the module"""
    if (level, key) not in _CTX:
        _CTX[(level, key)] = _renderer(CW, CH, level, key)
    r = _CTX[(level, key)]
    r.set_counters(False)
    r.set_blur_passes(0)
    return r


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for r in _CTX.values():
        r.close()
    _CTX.clear()
    _WANT.clear()


def _want(level, key, layout, cams):
    """the ray form's planes for (level, layout, cams): computed once per process on the level's context, never changed"""
    k = (level, key, layout[0], layout[1], tuple(layout[2]), np.asarray(cams, np.float32).tobytes())
    if k not in _WANT:
        assert not os.environ.get("PWN_DBG_FORCE_HASW") and not os.environ.get("PWN_SPHERE_LISTS")
        _WANT[k] = _ray_planes(_ctx(level, key), layout, cams)
    return _WANT[k]


def _same(got, want, what, mask=None):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        d = (g != w) if mask is None else ((g != w) & mask)
        bad = np.argwhere(d)
        assert len(bad) == 0, (what, name, len(bad), bad[:3].tolist(), [hex(int(g[tuple(b)])) for b in bad[:3]], [hex(int(w[tuple(b)])) for b in bad[:3]])


def _host_form(r, rects, cams, want_cell=True, want_dist=True):
    label, cell, dist = r.trace_viewport_hits(rects, cams, want_cell=want_cell, want_dist=want_dist)
    assert label.shape == (r.h, r.w) and label.dtype == np.uint32
    if want_cell:
        assert cell.shape == (r.h, r.w, 2) and cell.dtype == np.int16
    if want_dist:
        assert dist.shape == (r.h, r.w) and dist.dtype == np.float32
    return label, cell.view(np.uint32).reshape(r.h, r.w) if want_cell else None, VD._bits(dist) if want_dist else None


class _Call:
    """the tensors of one device call: each plane given lies in a buffer of its own with GUARD words on each side, everything poisoned"""

    def __init__(self, layout, cams, planes=NAMES):
        import torch
        W, H, rects = layout
        dev = _dev()
        self.layout, self.planes = layout, planes
        self.cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(len(rects), 16).copy()).to(dev)
        self.buf = {k: torch.full((W * H + 2 * GUARD,), POISON, dtype=torch.int32, device=dev) for k in planes}
        self.t = {k: b[GUARD:GUARD + W * H].view(H, W) for k, b in self.buf.items()}

    def run(self, r, lay, has_w=False, stream=None):
        import torch
        dist = self.t["dist"].view(torch.float32) if "dist" in self.t else None
        r.trace_viewport_hits_device(lay, self.cams, self.t["label"], self.t.get("cell"), dist, has_w=has_w, stream=stream)
        return self

    def host(self):
        """(label, cell, dist) as uint32 (H,W), None where not given; the guard words checked"""
        W, H, _ = self.layout
        out = []
        for k in NAMES:
            if k not in self.buf:
                out.append(None)
                continue
            a = self.buf[k].cpu().numpy().view(np.uint32)
            assert (a[:GUARD] == POISON).all() and (a[GUARD + W * H:] == POISON).all(), (k, "guard words written")
            out.append(a[GUARD:GUARD + W * H].reshape(H, W))
        return tuple(out)

    def check(self, want, what):
        """every pixel of every rectangle against `want` in every plane given; every word outside the rectangles still the poison"""
        got = self.host()
        inside = VD._inside(self.layout)
        _same(got, want, what, mask=inside)
        for k, g in zip(NAMES, got):
            if g is not None:
                assert (g[~inside] == POISON).all(), (what, k, "written outside the rectangles")
        return got


def _one_call(r, layout, cams, has_w=False, planes=NAMES):
    """a layout made, used once on a stream of its own and freed -> the call's tensors, complete"""
    import torch
    lay = r.viewports_layout(*layout)
    s = torch.cuda.Stream(_dev())
    with torch.cuda.stream(s):
        c = _Call(layout, cams, planes).run(r, lay, has_w=has_w)
    lay.free()                                # (returns behind the call's trace launch)
    return c


# ---------------------------------------------------------------- 1. exactness, every pixel; 2. outside the rectangles ----

@pytest.mark.parametrize("level,key", LEVELS)
@pytest.mark.parametrize("name", ["A", "B", "C64", "C332"])
def test_every_pixel_equals_the_ray_form(oracle_lib, level, key, name):
    layout = LAYOUTS[name]
    W, H, rects = layout
    cams, _ = VD._cams_for(oracle_lib, level, len(rects), 0)
    want = _want(level, key, layout, cams)
    inside = VD._inside(layout)
    assert want[0][inside].any() and (want[2][inside] != 0).any() and len(np.unique(want[1][inside])) > 1
    # the device form: poisoned planes of the layout's size on the 64 x 48 context
    _one_call(_ctx(level, key), layout, cams).check(want, (level, name, "device form"))
    # the host form on a context of the layout's size: 0 outside the rectangles (want has 0 there)
    h = _renderer(W, H, level, key)
    full = h.trace_viewport_hits([(0, 0, W, H)], cams[:1])          # (first a call that fills the staging with a whole frame)
    assert (full[0] != 0).sum() > W * H // 2
    _same(_host_form(h, rects, cams), want, (level, name, "host form"))
    h.close()


@pytest.mark.parametrize("level,key", LEVELS)
def test_layout_a_equals_one_view_batches_at_each_size(oracle_lib, level, key):
    """the contract's first step: rectangle i is trace_view_hits of cams[i] alone on a context of w_i x h_i"""
    W, H, rects = A
    cams, _ = VD._cams_for(oracle_lib, level, len(rects), 1)
    got = _one_call(_ctx(level, key), A, cams).host()
    h = _renderer(W, H, level, key)
    host = _host_form(h, rects, cams)
    h.close()
    for i, (x, y, w, hh) in enumerate(rects):
        s = _renderer(w, hh, level, key)
        label, cell, dist = s.trace_view_hits(cams[i:i + 1])
        s.close()
        one = (label[0], cell.view(np.uint32).reshape(hh, w), VD._bits(dist[0]))
        for k in range(3):
            assert (got[k][y:y + hh, x:x + w] == one[k]).all(), (i, NAMES[k], "device form")
            assert (host[k][y:y + hh, x:x + w] == one[k]).all(), (i, NAMES[k], "host form")


CORRIDOR = ".........\n.A;;*;;A.\n.........\n"          # (tests/test_gpu_view_hits.py's: a corridor closed on itself by a portal pair)


def _corridor_cam(sign, eps, pos):
    """looking along +-x from pos, the middle row's rays climbing by eps per unit: pixel (w/2 - 1, h/2) is (sign, eps, 0) exactly"""
    cam = np.zeros((4, 4), np.float32)
    cam[0, :3] = (0, 0, 1)
    cam[1, :3] = (0, 1, 0)
    cam[2, :3] = (sign, eps, 0)
    cam[3] = (*pos, 1)
    return cam


def test_exhausted_pixels_hold_zero_over_the_poison():
    """the loop corridor: pixel (w/2 - 1, h/2) of a view runs along it and, with a climb below 5.5e-4 per unit, out of its 1000 steps
    -- one such pixel in each of four views of 16 x 8: 0 in all three planes over the poison, in both forms"""
    import pwnfps_amd
    layout = (96, 40, [(0, 0, 16, 8), (16, 0, 16, 8), (41, 9, 16, 8), (3, 20, 16, 8), (64, 20, 32, 20)])
    cams = np.stack([_corridor_cam(s, e, p) for s, e, p in [
        (1, 0.0, (2.25, 0.5, 1.5)), (-1, 0.0, (4.5, 0.5, 1.25)), (1, 1e-5, (6.75, 0.5, 1.5)), (1, -2e-4, (3.5, 0.5, 1.75)), (1, 0.01, (2.25, 0.5, 1.5))]])
    r = _renderer(CW, CH)
    r.level_load_text(CORRIDOR)
    r.set_objects(np.zeros(0, pwnfps_amd.SPHERE_DTYPE))
    want = _ray_planes(r, layout, cams)
    inside = VD._inside(layout)
    none = inside & (want[0] == 0)
    for x, y, w, h in layout[2][:4]:
        assert none[y + h // 2, x + w // 2 - 1], (x, y)
    assert (want[1][none] == 0).all() and (want[2][none] == 0).all()
    assert (pwnfps_amd.unpack_labels(want[0][inside & ~none])[0] != 0).all()
    got = _one_call(r, layout, cams).check(want, "corridor, device form")
    for g in got:
        assert (g[none] == 0).all()
    r.close()
    h = _renderer(96, 40)
    h.level_load_text(CORRIDOR)
    h.set_objects(np.zeros(0, pwnfps_amd.SPHERE_DTYPE))
    _same(_host_form(h, layout[2], cams), want, "corridor, host form")
    h.close()


# ---------------------------------------------------------------- 3. plane pointers ----

@pytest.mark.parametrize("planes", [("label",), ("label", "cell"), ("label", "dist"), NAMES], ids=["label", "cell", "dist", "all"])
def test_planes_left_out(oracle_lib, planes):
    level, key = "pwnfps_level", "t0"
    for name in ("A", "B"):
        layout = LAYOUTS[name]
        cams, _ = VD._cams_for(oracle_lib, level, len(layout[2]), 2)
        want = _want(level, key, layout, cams)
        got = _one_call(_ctx(level, key), layout, cams, planes=planes).check(want, (name, planes))
        assert [g is not None for g in got] == [k in planes for k in NAMES]
        h = _renderer(layout[0], layout[1], level, key)
        host = _host_form(h, layout[2], cams, want_cell="cell" in planes, want_dist="dist" in planes)
        h.close()
        assert [g is not None for g in host] == [k in planes for k in NAMES]
        _same(host, want, (name, planes, "host form"))


# ---------------------------------------------------------------- 4. w lanes and denormals ----

def test_denormal_cameras_w_lanes_and_forced_four_lanes(oracle_lib):
    level, key = "pwnfps_level", "t0"
    cams, with_w, _ = VD._special_cams(oracle_lib, level, 5)
    plain = _want(level, key, A, cams)
    want_w = _want(level, key, A, with_w)
    assert any((a != b).any() for a, b in zip(want_w, plain))
    r = _ctx(level, key)
    _one_call(r, A, cams).check(plain, "denormal entries")
    _one_call(r, A, cams, has_w=True).check(plain, "denormal entries, PWN_VIEWS_HAS_W")
    _one_call(r, A, with_w, has_w=True).check(want_w, "w lanes, PWN_VIEWS_HAS_W")
    _one_call(r, A, with_w).check(plain, "w lanes without the flag: taken as 0, 0, 0, 1")
    h = _renderer(A[0], A[1], level, key)
    _same(_host_form(h, A[2], cams), plain, "host form, denormal entries")
    _same(_host_form(h, A[2], with_w), want_w, "host form, w lanes: it looks at the cameras")
    h.close()
    with VD._env(PWN_DBG_FORCE_HASW=1):                   # (read when a context is created)
        f = _renderer(CW, CH, level, key)
        fh = _renderer(A[0], A[1], level, key)
    _one_call(f, A, cams).check(plain, "PWN_DBG_FORCE_HASW")
    _one_call(f, A, with_w, has_w=True).check(want_w, "PWN_DBG_FORCE_HASW, w lanes")
    _same(_host_form(fh, A[2], cams), plain, "host form, PWN_DBG_FORCE_HASW")
    f.close()
    fh.close()


# ---------------------------------------------------------------- 5. the forms of the sphere lists ----

@pytest.mark.parametrize("form", ["indexed", "inline", "global"])
def test_every_form_of_the_sphere_lists(oracle_lib, form):
    level, key = "pwnfps_level", "t0"
    cams, _ = VD._cams_for(oracle_lib, level, 5, 2)
    want = _want(level, key, A, cams)
    with VD._env(PWN_SPHERE_LISTS=form):                  # (set before the context is created)
        r = _renderer(CW, CH, level, key)
        h = _renderer(A[0], A[1], level, key)
    assert r.sphere_tables()["form"] == {"indexed": 0, "inline": 1, "global": 2}[form] == h.sphere_tables()["form"]
    _one_call(r, A, cams).check(want, form)
    _one_call(r, A, cams, has_w=True).check(want, (form, "four lanes"))
    _same(_host_form(h, A[2], cams), want, (form, "host form"))
    r.close()
    h.close()


def test_tables_built_on_the_device(oracle_lib):
    import torch
    import pwnfps_amd
    level, key = "pwnfps_level", "t0"
    cams, _ = VD._cams_for(oracle_lib, level, 5, 2)
    want = _want(level, key, A, cams)
    s = np.ascontiguousarray(load_spheres(key), pwnfps_amd.SPHERE_DTYPE)
    r = _renderer(CW, CH)
    r.level_load(level_path(level))
    t = torch.from_numpy(s.view(np.int32).reshape(len(s), 8).copy()).to(_dev()).view(torch.float32)
    r.upload_spheres_device(t, pwnfps_amd.sphere_tables_plan(s)["pairs"] + 16)
    c = _one_call(r, A, cams)
    st = r.spheres_device_state()
    assert st["in_force"] == 1 and st["reason"] == 0 and st["n"] == len(s)
    c.check(want, "tables of pwn_upload_spheres_device")
    r.close()


def test_objects_beyond_2047(oracle_lib):
    """swarm_near, 2100 live spheres (lists in device memory): a view placed in front of a sphere with an index above 2047; that index
    comes back through the label's 14-bit field"""
    import pwnfps_amd
    sc = BS.scene("swarm_near", oracle_lib)
    assert len(sc.spheres) == 2100
    r = _renderer(CW, CH)
    r.level_load(BS.level_path(sc.level))
    r.set_objects(sc.spheres)
    assert r.sphere_tables()["form"] == 2
    layout = (70, 33, [(37, 5, 32, 24), (0, 0, 33, 7)])
    cams = None
    for i in range(2048, 2068):
        s = sc.spheres[i]
        c = np.eye(4, dtype=np.float32)
        c[3, :3] = (s["x"], s["y"], s["z"] - s["r"] - np.float32(0.15))
        want = _ray_planes(r, layout, np.stack([c, c]))
        objects = pwnfps_amd.unpack_labels(want[0])[2]
        if (objects > 2047).any():
            cams = np.stack([c, c])
            break
    assert cams is not None, "no view sees a sphere above 2047"
    got = _one_call(r, layout, cams).check(want, "swarm_near")
    assert (pwnfps_amd.unpack_labels(got[0][VD._inside(layout)])[2] > 2047).any()
    r.close()


# ---------------------------------------------------------------- 6. counters ----

def test_counters_are_the_ray_forms_summed(oracle_lib):
    level, key = "pwnfps_level", "t0"
    r = _ctx(level, key)
    for name in ("A", "B"):
        layout = LAYOUTS[name]
        W, H, rects = layout
        cams, _ = VD._cams_for(oracle_lib, level, len(rects), 1)
        r.set_counters(True)
        want = _ray_planes(r, layout, cams, counters=True)
        assert want[3][0] == sum(w * h for _, _, w, h in rects) and want[3][1] > want[3][0]
        st0 = r.stats()
        c = _one_call(r, layout, cams)
        st = r.stats()
        c.check(want, ("counters", name))
        assert VD._stats5(st) == want[3], (name, "device form")
        assert (st["trace_ms"], st["blur_ms"], st["total_ms"]) == (st0["trace_ms"], st0["blur_ms"], st0["total_ms"])      # (no timings)
        r.set_counters(False)
        h = _renderer(W, H, level, key)
        h.set_counters(True)
        _same(_host_form(h, rects, cams), want, ("counters", name, "host form"))
        st = h.stats()
        assert VD._stats5(st) == want[3], (name, "host form")
        assert st["blur_ms"] == 0.0 and st["total_ms"] >= st["trace_ms"] > 0.0
        h.close()
    exhausted = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)[0:1]
    r = _ctx("synth256", "synth256")
    r.set_counters(True)
    layout = (96, 40, [(16, 0, 64, 40)])
    want = _ray_planes(r, layout, exhausted, counters=True)
    c = _one_call(r, layout, exhausted)
    st = r.stats()
    r.set_counters(False)
    c.check(want, "synth256")
    assert VD._stats5(st) == want[3] and st["exhausted"] == int((want[0][VD._inside(layout)] == 0).sum()) > 0


# ---------------------------------------------------------------- 7. stream order, the records' rotation ----

@pytest.mark.parametrize("streams", [1, 2], ids=["one_stream", "two_alternating"])
def test_ten_calls_without_synchronisation(oracle_lib, streams):
    import torch
    level, key = "pwnfps_level", "t0"
    sets = [VD._cams_for(oracle_lib, level, 5, 10 + k)[0] for k in range(10)]
    want = [_want(level, key, A, cams) for cams in sets]
    assert any((want[k][0] != want[0][0]).any() for k in range(1, 10))
    r = _ctx(level, key)
    lay = r.viewports_layout(*A)
    st = [torch.cuda.Stream(_dev()) for _ in range(streams)]
    calls = [_Call(A, cams) for cams in sets]
    torch.cuda.synchronize()
    waits = r.launch_order_waits()
    for k, c in enumerate(calls):
        with torch.cuda.stream(st[k % streams]):
            c.run(r, lay)
    # (the first call on the second stream leaves the one-stream pattern of what ran before; the rest rotate by themselves)
    assert r.launch_order_waits() - waits <= 2
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        c.check(want[k], (streams, k))
    lay.free()


def test_hits_and_colour_calls_of_one_layout_interleaved(oracle_lib):
    """ten calls of one layout alternating between two streams, every third a colour call: both families rotate through the same records"""
    import torch
    level, key = "pwnfps_level", "t0"
    sets = [VD._cams_for(oracle_lib, level, 5, 10 + k) for k in range(10)]
    colour = [k % 3 == 1 for k in range(10)]
    want = [VD._ruler(level, key, A, 0, *sets[k]) if colour[k] else _want(level, key, A, sets[k][0]) for k in range(10)]
    r = _ctx(level, key)
    lay = r.viewports_layout(*A)
    st = [torch.cuda.Stream(_dev()) for _ in range(2)]
    calls = [VD._Call(A, *sets[k]) if colour[k] else _Call(A, sets[k][0]) for k in range(10)]
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        with torch.cuda.stream(st[k % 2]):
            if colour[k]:
                c.run(r, lay, 0)
            else:
                c.run(r, lay)
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        c.check(want[k], ("interleaved", k))
    lay.free()


def test_a_call_behind_a_long_launch_keeps_its_records(oracle_lib):
    """a call enqueued behind a long launch on one stream, then four calls with other cameras and another layout on a second stream,
    which go round the ticket sets: the first call's records are still its own"""
    import torch
    level, key = "pwnfps_level", "t0"
    A2 = (96, 40, [(0, 0, 48, 40), (48, 0, 48, 20), (48, 20, 16, 20), (64, 20, 32, 8), (64, 28, 32, 12)])
    sets = [VD._cams_for(oracle_lib, level, 5, 30 + k)[0] for k in range(5)]
    want = [_want(level, key, A if k == 0 else A2, sets[k]) for k in range(5)]
    r = _ctx(level, key)
    la, lb = r.viewports_layout(*A), r.viewports_layout(*A2)
    dev = _dev()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    calls = [_Call(A if k == 0 else A2, sets[k]) for k in range(5)]
    big = torch.randn((4096, 4096), device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(20):
            big = big @ big * 1e-3          # a long launch in front of the call
        calls[0].run(r, la)
    with torch.cuda.stream(s2):
        for k in range(1, 5):
            calls[k].run(r, lb)
    la.free()                               # (queued behind the long launch: returns only after the call's trace launch)
    calls[0].check(want[0], "behind the long launch")
    torch.cuda.synchronize()
    for k in range(1, 5):
        calls[k].check(want[k], ("round the sets", k))
    lb.free()


# ---------------------------------------------------------------- 8. the loop ----

def test_five_ticks_of_six_players_into_a_label_atlas():
    """players_step_device -> upload_spheres_device -> trace_viewport_hits_device, 6 players into a 96 x 40 atlas of 32 x 20 views, five
    ticks on one stream with nothing waited for on the host; every tick's planes equal the host-driven loop's"""
    import torch
    import pwnfps_amd
    level = "pwnfps_level"
    n, ticks = 6, 5
    atlas = (96, 40, [(32 * (i % 3), 20 * (i // 3), 32, 20) for i in range(n)])
    a = _renderer(96, 40)
    a.level_load(level_path(level))
    b = _renderer(CW, CH)
    b.level_load(level_path(level))
    sp = a.get_level()[2]
    cams0, grav0, _ = pwnfps_amd.players_spawn(sp, n)
    for i in range(n):
        cams0[i] = pwnfps_amd.spawn_camera(sp, ang_y=0.9 * i).reshape(16)
    keys = np.array([16, 17, 18, 32, 64, 128], np.uint8)

    def spheres_np(c):
        s = np.zeros(n, pwnfps_amd.SPHERE_DTYPE)
        s["r"], s["refl"] = 0.25, 0.2
        s["x"], s["y"], s["z"] = c[:, 12], c[:, 13], c[:, 14]
        s["cb"], s["cg"], s["cr"] = 0.3, 0.6, 0.9
        return s

    want = []
    hc, hg = cams0.copy(), grav0.copy()
    for t in range(ticks):
        hc, hg, _t = a.players_step(keys, hc, hg, tdiff=1 / 60, ticks=3)
        hc = np.ascontiguousarray(hc, np.float32).reshape(n, 16)
        a.set_objects(spheres_np(hc))
        want.append(_host_form(a, atlas[2], hc))
        if t == 0:
            _same(want[0], _ray_planes(a, atlas, hc), "the host-driven loop's first tick against the ray form")
    a.close()
    dev = _dev()
    lay = b.viewports_layout(*atlas)
    s1 = torch.cuda.Stream(dev)
    got = []
    with torch.cuda.stream(s1):
        d_keys = torch.from_numpy(keys).to(dev)
        d_cams = torch.from_numpy(cams0.copy()).to(dev)
        d_grav = torch.from_numpy(grav0.copy()).to(dev)
        d_sph = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        d_sph[:, 0], d_sph[:, 1] = 0.25, 0.2
        d_sph[:, 5], d_sph[:, 6], d_sph[:, 7] = 0.3, 0.6, 0.9
        for _ in range(ticks):
            b.players_step_device(d_keys, d_cams, d_grav, tdiff=1 / 60, ticks=3)
            d_sph[:, 2:5] = d_cams[:, 12:15]
            b.upload_spheres_device(d_sph, 4 * n)
            pl = [torch.full((40, 96), POISON, dtype=torch.int32, device=dev) for _ in range(3)]
            b.trace_viewport_hits_device(lay, d_cams, pl[0], pl[1], pl[2].view(torch.float32))
            got.append(pl)
    s1.synchronize()
    for t in range(ticks):
        _same(tuple(p.cpu().numpy().view(np.uint32) for p in got[t]), want[t], ("tick", t))
    assert any((want[t][0] != want[0][0]).any() for t in range(1, ticks))
    objects = pwnfps_amd.unpack_labels(want[ticks - 1][0])[2]
    assert (objects >= 0).any()                      # (the players see each other's spheres)
    lay.free()
    b.close()


# ---------------------------------------------------------------- 9. ownership ----

def _sequence(r, cams, between):
    """blocking frames (depth persistence on synth256), host-form batches of views and viewports (their depth plane persists), view
    hits and the counters of each; calls of the new family, both forms, in between when asked"""
    import torch
    out = []
    vp = [(0, 0, 240, 272), (240, 0, 240, 136)]
    rects = [(0, 0, 64, 40), (64, 0, 32, 20)]
    lay = r.viewports_layout(CW + 32, CH - 8, rects) if between else None

    def new_family():
        if between:
            c = _Call((CW + 32, CH - 8, rects), np.stack([cams[0], cams[3]]))
            c.run(r, lay)
            torch.cuda.synchronize()
            r.trace_viewport_hits([(8, 8, 200, 100), (240, 136, 240, 136)], np.stack([cams[0], cams[1]]))

    def stats():
        return np.array(VD._stats5(r.stats()), np.int64)

    new_family()
    out += list(r.trace_screen_centred(cams[1], 0.0)) + [stats()]
    new_family()
    out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32))) + [stats()]
    out += list(r.trace_viewports(vp, np.stack([cams[1], cams[2]]), [0.0, 0.0])) + [stats()]
    new_family()
    out += list(r.trace_screen_centred(cams[0], 0.0)) + [stats()]          # rays of cams[0] run out of steps: depth of cams[1] stays
    new_family()
    out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32))) + [stats()]
    out += list(r.trace_viewports(vp, np.stack([cams[0], cams[3]]), [0.0, 0.0])) + [stats()]      # ... and in the viewports' depth plane
    new_family()
    out += list(r.trace_view_hits(np.stack([cams[0], cams[2]]))) + [stats()]
    r.frames_config(2, sbuf=True, zbuf=True)
    r.submit_frame(cams[3], 0.25, 0)
    r.submit_frame(cams[2], 0.5, 1)
    if between:                                                # (the device form beside frames in flight)
        _Call((CW + 32, CH - 8, rects), np.stack([cams[0], cams[3]])).run(r, lay)
    for i in range(2):
        fr = r.wait_frame(i)
        out += [fr["sbuf"].copy(), fr["zbuf"].copy()]
    r.frames_config(0)
    new_family()
    out += list(r.trace_screen_centred(cams[1], 0.0)) + [stats()]
    if lay is not None:
        torch.cuda.synchronize()
        lay.free()
    return out


def test_other_calls_are_not_disturbed():
    """frames, view slots, the viewports' planes and depth, view hits, frames in flight and the counters of each, interleaved with
    calls of the new family, stay bit-identical to the same sequence without them"""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    res = []
    for between in (False, True):
        r = VD._renderer(480, 272, "synth256", "synth256", blur=1)
        r.set_counters(True)
        res.append(_sequence(r, cams, between))
        r.close()
    assert len(res[0]) == len(res[1])
    for i, (a, b) in enumerate(zip(*res)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), i


# ---------------------------------------------------------------- 10. refusals ----

def _raw(r, lay, cams, flags, label, cell, dist, stream=None):
    from pwnfps_amd._lib import lib
    return lib.pwn_trace_viewport_hits_device(r._ctx if r is not None else None, lay, C.c_void_p(cams), flags,
                                              C.c_void_p(label), C.c_void_p(cell), C.c_void_p(dist), C.c_void_p(stream))


def test_refusals(oracle_lib):
    """every refusal leaves the planes as they were and the next valid call right"""
    import torch
    import pwnfps_amd
    from pwnfps_amd._lib import lib
    level, key = "pwnfps_level", "t0"
    W, H, rects = A
    cams, _ = VD._cams_for(oracle_lib, level, 5, 0)
    want = _want(level, key, A, cams)
    r = _ctx(level, key)
    r.set_blur_passes(1)                                  # (ignored: layout B, which no blur could take, is accepted below)
    other = _renderer(CW, CH, level, key)
    la, lb, lo = r.viewports_layout(*A), r.viewports_layout(*B), other.viewports_layout(*A)
    dev = _dev()
    plane = W * H * 4
    # three planes in ONE allocation with a spare behind each, so that pointers can be shifted and made to overlap on purpose
    pool = torch.full((6, H, W), POISON, dtype=torch.int32, device=dev)
    p_label, p_cell, p_dist = pool[0].data_ptr(), pool[2].data_ptr(), pool[4].data_ptr()
    t_cams = torch.from_numpy(cams.reshape(5, 16).copy()).to(dev)
    pc = t_cams.data_ptr()
    good = dict(lay=la._ptr, cams=pc, flags=0, label=p_label, cell=p_cell, dist=p_dist)
    assert _raw(None, **good) == PWN_EINVAL
    bad = [dict(lay=None), dict(cams=None), dict(label=None),
           dict(lay=lo._ptr),                                                                                    # another context's layout
           dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(cams=pc + 4), dict(label=p_label + 4), dict(cell=p_cell + 8), dict(dist=p_dist + 12),
           dict(cell=p_label), dict(dist=p_label), dict(dist=p_cell),                                            # two planes the same
           dict(cell=p_label + plane - 16), dict(dist=p_cell + plane - 16), dict(label=p_dist - plane + 16, cell=None)]      # ... or a word in common
    for kw in bad:
        assert _raw(r, **dict(good, **kw)) == PWN_EINVAL, kw
    freed = r.viewports_layout(*A)
    fp = freed._ptr
    freed.free()
    assert _raw(r, **dict(good, lay=fp)) == PWN_EINVAL                                                          # a layout already freed
    # before a level; a pwn_init_multi handle; a row tiling -- both forms
    hr = np.array(rects, np.int32)
    hp = [np.full((CH, CW), POISON, np.uint32) for _ in range(3)]
    small = np.array([(0, 0, 40, 30), (40, 30, 24, 18)], np.int32)

    def host(rr, rc=small, n=2, cams_=cams, label=hp[0], cell=hp[1], dist=hp[2]):
        return lib.pwn_trace_viewport_hits(rr._ctx if rr is not None else None, n, rc.ctypes.data if rc is not None else None,
                                           cams_.ctypes.data if cams_ is not None else None, label.ctypes.data if label is not None else None,
                                           cell.ctypes.data if cell is not None else None, dist.ctypes.data if dist is not None else None)

    nl = _renderer(CW, CH)
    ln = nl.viewports_layout(*A)                                                                                 # (creation needs no level)
    assert _raw(nl, **dict(good, lay=ln._ptr)) == PWN_ENOLEVEL and host(nl) == PWN_ENOLEVEL
    nl.close()
    g = pwnfps_amd.Renderer(CW, CH, devices=[0, 0])
    g.level_load(level_path(level))
    g.set_objects(load_spheres(key))
    assert _raw(g, **good) == PWN_ENOTSUP and host(g) == PWN_ENOTSUP
    g.close()
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert _raw(r, **good) == PWN_EBUSY and host(r) == PWN_EBUSY
    r.tiled_shutdown()
    # the host form's own arguments, and what pwn_viewports_plan refuses (layout A is wider than this context)
    assert host(None) == PWN_EINVAL and host(r, rc=None) == PWN_EINVAL and host(r, cams_=None) == PWN_EINVAL and host(r, label=None) == PWN_EINVAL
    assert host(r, rc=hr, n=5) == PWN_EINVAL and host(r, n=0) == PWN_EINVAL
    assert host(r, rc=np.array([(0, 0, 40, 30), (39, 29, 4, 4)], np.int32)) == PWN_EINVAL
    assert host(r, rc=np.array([(0, 0, 0, 4), (8, 8, 4, 4)], np.int32)) == PWN_EINVAL
    assert all((p == POISON).all() for p in hp)
    torch.cuda.synchronize()
    assert (pool.cpu().numpy().view(np.uint32) == POISON).all()                                                  # nothing was written by any of it
    # the same ranges, in order, are accepted (planes that touch are fine; blur passes play no part), and the pixels are right
    assert _raw(r, **dict(good, label=p_cell - plane, dist=p_cell + plane)) == 0
    assert _raw(r, **dict(good, lay=lb._ptr, cell=None)) == 0                                                    # (70 x 33 words of them)
    assert host(r) == 0 and all((p[:30, :40] != POISON).all() and (p[30:, :40] == 0).all() for p in hp)
    torch.cuda.synchronize()
    _one_call(r, A, cams).check(want, "after the refusals")
    # the binding's own checks
    c = _Call(A, cams)
    lab, cel, dis = c.t["label"], c.t["cell"], c.t["dist"].view(torch.float32)
    for kw in (dict(dist=c.t["dist"]),                                                                           # distance must be float32
               dict(label=dis),
               dict(cams=c.cams[:4]),                                                                            # n is the layout's
               dict(label=lab[:-1]), dict(cell=cel[:, :-1]), dict(label=lab.cpu()), dict(cams=c.cams.cpu()),
               dict(lay=lo),                                                                                     # another renderer's layout
               dict(lay=freed),
               dict(label=torch.zeros(W * H + 1, dtype=torch.int32, device=dev)[1:].view(H, W))):                # not 16-byte aligned
        a = dict(dict(lay=la, cams=c.cams, label=lab, cell=cel, dist=dis), **kw)
        with pytest.raises(ValueError):
            r.trace_viewport_hits_device(a["lay"], a["cams"], a["label"], a["cell"], a["dist"])
    for g_ in c.host():
        assert (g_ == POISON).all()
    # (cell as (H,W,2) int16 is taken)
    pairs = torch.full((H, W, 2), 0x5a5a, dtype=torch.int16, device=dev)
    r.trace_viewport_hits_device(la, c.cams, lab, pairs, dis)
    torch.cuda.synchronize()
    inside = VD._inside(A)
    assert (pairs.cpu().numpy().view(np.uint32).reshape(H, W)[inside] == want[1][inside]).all()
    la.free()
    lb.free()
    other.close()                                                                                                # (lo goes with its renderer)
    assert lo._ptr is None
    r.set_blur_passes(0)
