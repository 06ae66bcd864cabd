"""pwn_trace_viewports_device: views of their own sizes from cameras in device memory into planes of the caller's, of a frame size
the caller chooses.  The ruler is the host form pwn_trace_viewports on a SECOND context of the layout's W x H with the same level
and objects (in one test: pwn_trace_screen_centred on contexts of w_i x h_i); the device context is deliberately of another size,
64 x 48, so that no pixel can depend on it.  Rectangle i is bit-identical, colour and depth; nothing outside the rectangles is
written; the set-up kernel gives the bits of the host's frame_setup for a view of its own size, denormals included."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
CW, CH = 64, 48                       # the device context's own size
POISON = 0x5a5a5a5a

# Layout A: frame 96 x 40, usable with blur.  The given order is not the rising-units order (24, 12, 2, 3, 16 units); the frame and
# the widest view are wider than the context, and 24 blur groups exceed the context's 17 table entries; x 48..95 of rows 20..23 is
# covered by nothing.
A = (96, 40, [(0, 0, 96, 16), (0, 16, 32, 24), (32, 16, 16, 8), (48, 16, 48, 4), (32, 24, 64, 16)])
# Layout B: frame 70 x 33, blur off only.  Widths off the 16- and 32-pixel grid, a 1 x 1 view, views of 6 units each (ties),
# uncovered area.
B = (70, 33, [(0, 0, 37, 21), (37, 0, 33, 5), (37, 5, 1, 1), (38, 5, 20, 12), (3, 21, 17, 12)])
# Layout C: one view, the whole frame
C64 = (64, 48, [(0, 0, 64, 48)])
C332 = (332, 202, [(0, 0, 332, 202)])
LAYOUTS = {"A": A, "B": B, "C64": C64, "C332": C332}


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


def _dev():
    import torch
    return torch.device("cuda", 0)


def _renderer(w, h, level=None, spheres=None, blur=1):
    import pwnfps_amd
    r = pwnfps_amd.Renderer(w, h)
    if level is not None:
        r.level_load(level_path(level))
        r.set_objects(load_spheres(spheres))
    r.set_blur_passes(blur)
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stats5(st):
    return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])


def _random_cams(rng, oracle_lib, level, n):
    """(tests/test_gpu_viewports.py's cameras: a free cell, any heading, a pitch up to 1.2)"""
    O = oracle_lib.Oracle()
    O.load_level(level_path(level))
    data, _, _ = O.get_level()
    free = [(x, z) for z in range(64) for x in range(64) if chr(data[z, x]) in ';$"#&><,^']
    cams = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        x, z = free[rng.integers(len(free))]
        ay, ax = rng.uniform(0, 6.28), rng.uniform(-1.2, 1.2)
        cy, sy, cx, sx = np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
        cam = np.eye(4, dtype=np.float32)
        cam[:3, :3] = (np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])).astype(np.float32)
        cam[3, :3] = (x + rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95), z + rng.uniform(0.05, 0.95))
        cams[i] = cam
    secs = rng.uniform(0, 50, n).astype(np.float32)
    return cams, secs


_CAMS = {}


def _cams_for(oracle_lib, level, n, seed):
    """camera set `seed` for n views of a level, the same for every test that uses it"""
    k = (level, n, seed)
    if k not in _CAMS:
        _CAMS[k] = _random_cams(np.random.default_rng(20261020 + 977 * seed + n), oracle_lib, level, n)
    return _CAMS[k]


_RULER = {}


def _ruler(level, key, layout, blur, cams, secs, counters=False):
    """(colour, depth, counters) of the host form on a FRESH context of the layout's size: computed once per process, never changed"""
    W, H, rects = layout
    k = (level, key, W, H, tuple(rects), blur, np.asarray(cams, np.float32).tobytes(), np.asarray(secs, np.float32).tobytes(), counters)
    if k not in _RULER:
        assert not os.environ.get("PWN_DBG_FORCE_HASW") and not os.environ.get("PWN_SPHERE_LISTS")
        r = _renderer(W, H, level, key, blur=blur)
        r.set_counters(counters)
        sb, zb = r.trace_viewports(rects, cams, secs)
        _RULER[k] = (sb.copy(), zb.copy(), _stats5(r.stats()) if counters else None)
        r.close()
    return _RULER[k]


def _inside(layout):
    W, H, rects = layout
    m = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        m[y:y + h, x:x + w] = True
    return m


class _Call:
    """the tensors of one call: colour and work poisoned, depth zero inside the rectangles (a fresh context's plane) and poisoned
    outside, or what the caller gives"""

    def __init__(self, layout, cams, secs, z_in=None):
        import torch
        W, H, rects = layout
        dev = _dev()
        n = len(rects)
        self.layout = layout
        self.cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
        self.secs = torch.from_numpy(np.ascontiguousarray(secs, np.float32).copy()).to(dev)
        self.sb = torch.full((H, W), POISON, dtype=torch.int32, device=dev)
        self.work = torch.full((H, W), POISON, dtype=torch.int32, device=dev)
        if z_in is None:
            z_in = np.full((H, W), POISON, np.uint32)
            z_in[_inside(layout)] = 0
        self.z_in = np.ascontiguousarray(z_in).view(np.uint32).copy()
        self.z = torch.from_numpy(self.z_in.view(np.float32).copy()).to(dev)

    def run(self, r, lay, blur, has_w=False, stream=None):
        r.trace_viewports_device(lay, self.cams, self.secs, self.sb, self.z, work=self.work if blur > 0 else None, has_w=has_w, stream=stream)
        return self

    def host(self):
        return self.sb.cpu().numpy().view(np.uint32), self.z.cpu().numpy()

    def check(self, want, what, skip=()):
        """every rectangle against `want` (colour, depth, ...); every word outside the rectangles as it came in"""
        W, H, rects = self.layout
        sb, z = self.host()
        for i, (x, y, w, h) in enumerate(rects):
            if i in skip:
                continue
            bad = int((sb[y:y + h, x:x + w] != want[0][y:y + h, x:x + w]).sum())
            assert bad == 0, (what, i, (x, y, w, h), bad)
            assert (_bits(z[y:y + h, x:x + w]) == _bits(want[1][y:y + h, x:x + w])).all(), (what, i, (x, y, w, h))
        out = ~_inside(self.layout)
        assert (sb[out] == POISON).all(), (what, "colour outside the rectangles")
        assert (_bits(z)[out] == self.z_in[out]).all(), (what, "depth outside the rectangles")


_DEVCTX = {}


def _devctx(level, key):
    """the device context of a level (64 x 48 whatever the layout), kept for the module; blur and counters as the caller sets them"""
    if (level, key) not in _DEVCTX:
        _DEVCTX[(level, key)] = _renderer(CW, CH, level, key)
    r = _DEVCTX[(level, key)]
    r.set_counters(False)
    return r


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for r in _DEVCTX.values():
        r.close()
    _DEVCTX.clear()


def _one_call(r, layout, cams, secs, blur, has_w=False):
    """a layout made, used once on a stream of its own and freed -> the call's tensors, complete"""
    import torch
    r.set_blur_passes(blur)
    lay = r.viewports_layout(layout[0], layout[1], layout[2])
    s = torch.cuda.Stream(_dev())
    with torch.cuda.stream(s):
        c = _Call(layout, cams, secs).run(r, lay, blur, has_w=has_w)
    lay.free()                                # (returns behind the call's last launch)
    return c


# ---------------------------------------------------------------- bit-for-bit parity, untouched area ----

@pytest.mark.parametrize("level,key", [("pwnfps_level", "t0"), ("synth64", "synth64")])
@pytest.mark.parametrize("name,blur", [("A", 0), ("A", 1), ("A", 2), ("B", 0), ("C64", 0), ("C332", 0)])
def test_each_rectangle_equals_the_host_form(oracle_lib, level, key, name, blur):
    layout = LAYOUTS[name]
    r = _devctx(level, key)
    for seed in range(3):
        cams, secs = _cams_for(oracle_lib, level, len(layout[2]), seed)
        want = _ruler(level, key, layout, blur, cams, secs)
        assert want[0][_inside(layout)].any()
        _one_call(r, layout, cams, secs, blur).check(want, (level, name, blur, seed))


def test_layout_info_and_the_context_own_size():
    r = _devctx("pwnfps_level", "t0")
    assert (r.w, r.h) == (CW, CH)
    for name, units, blur_ok in (("A", 57, True), ("B", 37, False), ("C64", 48, True), ("C332", 21 * 51, True)):
        W, H, rects = LAYOUTS[name]
        lay = r.viewports_layout(W, H, rects)
        assert lay.info() == dict(W=W, H=H, n=len(rects), units=units, pixels=sum(w * h for _, _, w, h in rects), blur_ok=blur_ok), name
        lay.free()
        lay.free()
        with pytest.raises(ValueError):
            lay.info()


def test_each_rectangle_equals_the_blocking_call_at_its_size(oracle_lib):
    """the ruler of the host form's own contract: pwn_trace_screen_centred on fresh contexts of w_i x h_i"""
    level, key, blur = "pwnfps_level", "t0", 1
    W, H, rects = A
    cams, secs = _cams_for(oracle_lib, level, len(rects), 0)
    sb, z = _one_call(_devctx(level, key), A, cams, secs, blur).host()
    for i, (x, y, w, h) in enumerate(rects):
        s = _renderer(w, h, level, key, blur=blur)
        a, za = s.trace_screen_centred(cams[i], secs[i])
        s.close()
        assert (sb[y:y + h, x:x + w] == a).all() and (_bits(z[y:y + h, x:x + w]) == _bits(za)).all(), i


# ---------------------------------------------------------------- the set-up kernel's records ----

def _hostile_cameras(rng, xsrat, ysrat):
    """(tests/test_gpu_views_device.py's) 64 cameras: random ones, then every special value in every place of the formulas"""
    f = np.float32
    cams = rng.uniform(-2, 2, (64, 16)).astype(np.float32)
    d = f(2.0 ** -127)                                    # a denormal whose double is normal
    cams[8, 0:4] = d; cams[8, 8:12] = d; cams[8, 4:8] = 0.0        # c0 + c8: two denormals, a normal sum
    cams[9, 0:4] = d; cams[9, 8:12] = -d                 # ... that cancel
    cams[10, 0:4] = f(2.0 ** -149); cams[10, 8:12] = f(2.0 ** -149)
    cams[11, :] = d                                       # every product and sum of denormals
    cams[12, :] = f(2.0 ** -140)
    for row, e in ((13, -126), (14, -122), (15, -118)):    # products with xsrat / ysrat that are denormal, or just normal
        cams[row, 0:4] = f(2.0 ** e) / abs(xsrat) * f(0.75)
        cams[row, 4:8] = f(2.0 ** e) / abs(ysrat) * f(-0.75)
    cams[16, :] = 0.0
    cams[17, :] = -0.0
    cams[18, 0:4] = 0.0; cams[18, 8:12] = -0.0; cams[18, 4:8] = -0.0
    cams[19, :] = 3e38                                    # c0 + c8 overflows
    cams[20, :] = -3e38
    cams[21, 0:4] = 3e38; cams[21, 8:12] = -3e38; cams[21, 4:8] = 3e38
    cams[22, :] = np.inf
    cams[23, 0:4] = np.inf; cams[23, 8:12] = -np.inf     # inf - inf
    cams[24, 4:8] = -np.inf
    cams[25, :] = np.nan
    cams[27, 12:16] = (d, -0.0, np.inf, np.nan)           # `from` is copied as it is
    secs = rng.uniform(0, 50, 64).astype(np.float32)
    secs[8], secs[9], secs[10], secs[11] = d, -0.0, np.inf, 1e-45
    return cams, secs


def _scalars(w, h):
    """pwn_frame_setup_scalars in float32, every operation rounded on its own: (-yrat, xsrat, ysrat)"""
    f = np.float32
    dimx, dimy = f(w), f(h)
    yrat = (-dimy) / dimx
    xsrat = f(-2.0) / dimx
    ysrat = (yrat + yrat) / dimy
    assert all(v.dtype == np.float32 for v in (yrat, xsrat, ysrat))
    return -yrat, xsrat, ysrat


def test_setup_kernel_records():
    """pwn_launch_viewport_setup by itself, 64 records of views of 64 different sizes, the cameras in another order than the records:
    the 128-byte records as bits against frame_setup restated with each view's OWN scalars; the geometry words are the master's"""
    import torch
    from pwnfps_amd._lib import lib
    assert np.float32(2 ** -127) + np.float32(2 ** -127) != 0          # (a process that flushes denormals proves nothing)
    n = 64
    rng = np.random.default_rng(96 * 40)
    sizes = [(int(rng.integers(1, 700)), int(rng.integers(1, 500))) for _ in range(n)]
    sizes[8:16] = [(3, 7), (160, 120), (320, 240), (40, 20), (3, 7), (160, 120), (320, 240), (40, 20)]
    perm = rng.permutation(n).astype(np.uint32)
    assert (perm != np.arange(n)).any()
    scal = np.zeros((n, 4), np.float32)
    for j in range(n):
        scal[j, :3] = _scalars(*sizes[j])
    # the hostile rows are made for the scalars of the record that reads them
    cams = np.zeros((n, 16), np.float32)
    secs = np.zeros(n, np.float32)
    for j in range(n):
        hc, hs = _hostile_cameras(np.random.default_rng(j), scal[j, 1], scal[j, 2])
        cams[perm[j]], secs[perm[j]] = hc[j], hs[j]
    master = rng.integers(0, 2 ** 32, (n, 32), dtype=np.uint64).astype(np.uint32)
    want = master.copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            c = cams[perm[j]]
            rec = np.zeros(17, np.float32)
            rec[0:4] = (c[0:4] + c[8:12]) + scal[j, 0] * c[4:8]
            rec[4:8] = scal[j, 1] * c[0:4]
            rec[8:12] = scal[j, 2] * c[4:8]
            rec[12:16] = c[12:16]
            rec[16] = secs[perm[j]]
            want[j, :17] = rec.view(np.uint32)
    tiny = np.finfo(np.float32).tiny
    assert (want[8, 0:4].view(np.float32) == tiny).all()               # (two denormals, a normal sum)
    w13 = want[13, 4:12].view(np.float32)
    assert (abs(w13) < tiny).all() and (w13 != 0).all()                 # (denormal products)
    dev = _dev()
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in
         dict(master=master, scal=scal, perm=perm, cams=cams, secs=secs).items()}
    t_out = torch.full((n + 1, 32), 7, dtype=torch.int32, device=dev)
    fn = lib.pwn_launch_viewport_setup
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    assert all(t[k].data_ptr() % 16 == 0 for k in t) and t_out.data_ptr() % 16 == 0
    assert fn(t["master"].data_ptr(), t["scal"].data_ptr(), t["perm"].data_ptr(), t["cams"].data_ptr(), t["secs"].data_ptr(), t_out.data_ptr(),
              n, torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    got = t_out.cpu().numpy().view(np.uint32)
    assert (got[n] == 7).all()                                          # nothing behind the n records
    got = got[:n]
    nan = np.zeros(want.shape, bool)
    nan[:, :12] = np.isnan(want[:, :12].view(np.float32))               # (computed NaNs: any NaN; copied words: their bits)
    assert np.isnan(got.view(np.float32)[nan]).all()
    bad = np.argwhere(~nan & (got != want))
    assert len(bad) == 0, [(int(i), int(k), hex(got[i, k]), hex(want[i, k])) for i, k in bad[:8]]


def _special_cams(oracle_lib, level, n):
    """camera set 0 with denormal entries in rows x, y and z of some views (sums and products of denormals in the set-up) and w
    components in one view"""
    cams, secs = _cams_for(oracle_lib, level, n, 0)
    cams = cams.copy()
    d = np.float32(2.0 ** -127)
    cams[0, 0, 1] = d; cams[0, 2, 1] = d                  # c0 + c8: two denormals, a normal sum
    cams[1, 1, 0] = np.float32(2.0 ** -140)               # ysrat * c4 and yrat * c4: denormal products
    cams[2 % n, 0, 2] = -d; cams[2 % n, 2, 2] = np.float32(2.0 ** -149)
    with_w = cams.copy()
    with_w[3 % n, :, 3] = (0.03, -0.01, 0.05, 0.8)
    return cams, with_w, secs


def test_denormal_cameras_w_lanes_and_forced_four_lanes(oracle_lib):
    level, key, blur = "pwnfps_level", "t0", 1
    cams, with_w, secs = _special_cams(oracle_lib, level, 5)
    plain = _ruler(level, key, A, blur, cams, secs)
    want_w = _ruler(level, key, A, blur, with_w, secs)
    assert (want_w[0] != plain[0]).any()
    r = _devctx(level, key)
    _one_call(r, A, cams, secs, blur).check(plain, "denormal entries")
    _one_call(r, A, cams, secs, blur, has_w=True).check(plain, "denormal entries, PWN_VIEWS_HAS_W")
    _one_call(r, A, with_w, secs, blur, has_w=True).check(want_w, "w lanes, PWN_VIEWS_HAS_W")
    _one_call(r, A, with_w, secs, blur).check(plain, "w lanes without the flag: taken as 0, 0, 0, 1")
    with _env(PWN_DBG_FORCE_HASW=1):                      # (read when a context is created)
        f = _renderer(CW, CH, level, key)
    _one_call(f, A, cams, secs, blur).check(plain, "PWN_DBG_FORCE_HASW")
    _one_call(f, A, with_w, secs, blur, has_w=True).check(want_w, "PWN_DBG_FORCE_HASW, w lanes")
    f.close()


def test_counters_equal_the_rulers(oracle_lib):
    level, key = "pwnfps_level", "t0"
    for name, blur in (("A", 1), ("B", 0)):
        layout = LAYOUTS[name]
        cams, secs = _cams_for(oracle_lib, level, len(layout[2]), 1)
        want = _ruler(level, key, layout, blur, cams, secs, counters=True)
        r = _devctx(level, key)
        r.set_counters(True)
        st0 = r.stats()
        c = _one_call(r, layout, cams, secs, blur)
        st = r.stats()
        r.set_counters(False)
        c.check(want, ("counters", name))
        assert _stats5(st) == want[2] and want[2][0] >= sum(w * h for _, _, w, h in layout[2]), name
        assert (st["trace_ms"], st["blur_ms"], st["total_ms"]) == (st0["trace_ms"], st0["blur_ms"], st0["total_ms"])      # (no timings)


@pytest.mark.parametrize("form", ["indexed", "inline", "global"])
def test_every_form_of_the_sphere_lists(oracle_lib, form):
    level, key, blur = "pwnfps_level", "t0", 1
    cams, secs = _cams_for(oracle_lib, level, 5, 2)
    want = _ruler(level, key, A, blur, cams, secs)
    with _env(PWN_SPHERE_LISTS=form):                     # (set before the context is created)
        r = _renderer(CW, CH, level, key)
        assert r.sphere_tables()["form"] == {"indexed": 0, "inline": 1, "global": 2}[form]
        _one_call(r, A, cams, secs, blur).check(want, form)
        r.close()


def test_tables_built_on_the_device(oracle_lib):
    import torch
    import pwnfps_amd
    level, key, blur = "pwnfps_level", "t0", 1
    cams, secs = _cams_for(oracle_lib, level, 5, 2)
    want = _ruler(level, key, A, blur, cams, secs)
    s = np.ascontiguousarray(load_spheres(key), pwnfps_amd.SPHERE_DTYPE)
    r = _renderer(CW, CH, blur=blur)
    r.level_load(level_path(level))
    t = torch.from_numpy(s.view(np.int32).reshape(len(s), 8).copy()).to(_dev()).view(torch.float32)
    r.upload_spheres_device(t, pwnfps_amd.sphere_tables_plan(s)["pairs"] + 16)
    c = _one_call(r, A, cams, secs, blur)
    st = r.spheres_device_state()
    assert st["in_force"] == 1 and st["reason"] == 0 and st["n"] == len(s)
    c.check(want, "tables of pwn_upload_spheres_device")
    r.close()


# ---------------------------------------------------------------- depth in / out ----

def test_depth_persists_by_destination_pixel_through_the_callers_plane():
    """synth256: rays of cams[0] run out of steps and keep the depth cams[1] left at their DESTINATION pixel -- three calls into one
    depth plane of the caller's, against three calls of the host form on one context of 512 x 288"""
    import torch
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    W, H, rect, side = 512, 288, (16, 8, 480, 272), (496, 0, 16, 288)
    calls = [([rect], cams[1:2], [0.0]), ([side, rect], np.stack([cams[0], cams[0]]), [0.0, 0.0]), ([rect], cams[0:1], [0.0])]
    for blur in (0, 1):
        ruler = _renderer(W, H, "synth256", "synth256", blur=blur)
        want = [tuple(a.copy() for a in ruler.trace_viewports(rects, cs, ss)) for rects, cs, ss in calls]
        ruler.close()
        fresh = _ruler("synth256", "synth256", (W, H, calls[1][0]), blur, calls[1][1], calls[1][2])
        assert (_bits(fresh[1]) != _bits(want[1][1])).any()          # (the second call's depth does depend on the first)
        r = _devctx("synth256", "synth256")
        r.set_blur_passes(blur)
        z = np.zeros((H, W), np.float32)
        for k, (rects, cs, ss) in enumerate(calls):
            lay = r.viewports_layout(W, H, rects)
            c = _Call((W, H, rects), cs, ss, z_in=z)
            c.run(r, lay, blur)
            torch.cuda.synchronize()
            lay.free()
            sb, z = c.host()
            for x, y, w, h in rects:
                assert (sb[y:y + h, x:x + w] == want[k][0][y:y + h, x:x + w]).all(), (blur, k)
            assert (_bits(z) == _bits(want[k][1])).all(), (blur, k)          # (the whole plane: outside the rectangles it is what it was)


# ---------------------------------------------------------------- stream order, the records' rotation ----

@pytest.mark.parametrize("streams", [1, 2], ids=["one_stream", "two_alternating"])
def test_ten_calls_without_synchronisation(oracle_lib, streams):
    import torch
    level, key, blur = "pwnfps_level", "t0", 1
    sets = [_cams_for(oracle_lib, level, 5, 10 + k) for k in range(10)]
    want = [_ruler(level, key, A, blur, cams, secs) for cams, secs in sets]
    assert any((want[k][0] != want[0][0]).any() for k in range(1, 10))
    r = _devctx(level, key)
    r.set_blur_passes(blur)
    lay = r.viewports_layout(*A)
    st = [torch.cuda.Stream(_dev()) for _ in range(streams)]
    calls = [_Call(A, cams, secs) for cams, secs in sets]
    torch.cuda.synchronize()
    waits = r.launch_order_waits()
    for k, c in enumerate(calls):
        with torch.cuda.stream(st[k % streams]):
            c.run(r, lay, blur)
    # (the first call on the second stream leaves the one-stream pattern of what ran before; the rest rotate by themselves)
    assert r.launch_order_waits() - waits <= 2
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        c.check(want[k], (streams, k))
    lay.free()


def test_launches_that_run_beside_each_other_have_records_of_their_own(oracle_lib):
    """six calls of eight 512 x 512 views alternating between two streams, the cameras other ones in every call: a trace launch reads
    its records unit by unit for as long as it runs (a third of a millisecond here), and the next call's set-up, on the other stream,
    runs beside it -- into the records of another ticket set"""
    import torch
    level, key, blur = "pwnfps_level", "t0", 0
    big = (2048, 1024, [(512 * (i % 4), 512 * (i // 4), 512, 512) for i in range(8)])
    sets = [_cams_for(oracle_lib, level, 8, 50 + k) for k in range(6)]
    want = [_ruler(level, key, big, blur, cams, secs) for cams, secs in sets]
    r = _devctx(level, key)
    r.set_blur_passes(blur)
    lay = r.viewports_layout(*big)
    st = [torch.cuda.Stream(_dev()) for _ in range(2)]
    calls = [_Call(big, cams, secs) for cams, secs in sets]
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        with torch.cuda.stream(st[k % 2]):
            c.run(r, lay, blur)
    lay.free()
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        c.check(want[k], ("beside each other", k))


def test_a_call_behind_a_long_launch_keeps_its_records(oracle_lib):
    """a call enqueued behind a long launch on one stream, then four calls with other cameras and another layout on a second stream,
    which go round the ticket sets: the first call's records, and the rectangles its blur reads, are still its own"""
    import torch
    level, key, blur = "pwnfps_level", "t0", 1
    A2 = (96, 40, [(0, 0, 48, 40), (48, 0, 48, 20), (48, 20, 16, 20), (64, 20, 32, 8), (64, 28, 32, 12)])
    sets = [_cams_for(oracle_lib, level, 5, 30 + k) for k in range(5)]
    want = [_ruler(level, key, A if k == 0 else A2, blur, *sets[k]) for k in range(5)]
    r = _devctx(level, key)
    r.set_blur_passes(blur)
    la, lb = r.viewports_layout(*A), r.viewports_layout(*A2)
    dev = _dev()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    calls = [_Call(A if k == 0 else A2, *sets[k]) for k in range(5)]
    big = torch.randn((4096, 4096), device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(20):
            big = big @ big * 1e-3          # a long launch in front of the call
        calls[0].run(r, la, blur)
    with torch.cuda.stream(s2):
        for k in range(1, 5):
            calls[k].run(r, lb, blur)
    la.free()                               # (queued behind the long launch: returns only after the call's last blur pass)
    calls[0].check(want[0], "behind the long launch")
    torch.cuda.synchronize()
    for k in range(1, 5):
        calls[k].check(want[k], ("round the sets", k))
    lb.free()


# ---------------------------------------------------------------- the loop ----

def test_five_ticks_of_six_players_into_an_atlas():
    """players_step_device -> upload_spheres_device -> trace_viewports_device, 6 players into a 96 x 40 atlas of 32 x 20 views, five
    ticks on one stream with nothing waited for on the host; every tick's atlas equals the host-driven loop's"""
    import torch
    import pwnfps_amd
    level, blur = "pwnfps_level", 1
    n, ticks = 6, 5
    atlas = (96, 40, [(32 * (i % 3), 20 * (i // 3), 32, 20) for i in range(n)])
    a = _renderer(96, 40, blur=blur)
    a.level_load(level_path(level))
    b = _renderer(CW, CH, blur=blur)
    b.level_load(level_path(level))
    sp = a.get_level()[2]
    cams0, grav0, _ = pwnfps_amd.players_spawn(sp, n)
    for i in range(n):
        cams0[i] = pwnfps_amd.spawn_camera(sp, ang_y=0.9 * i).reshape(16)
    keys = np.array([16, 17, 18, 32, 64, 128], np.uint8)
    secs = np.arange(n, dtype=np.float32) * 0.25

    def spheres_np(c):
        s = np.zeros(n, pwnfps_amd.SPHERE_DTYPE)
        s["r"], s["refl"] = 0.25, 0.2
        s["x"], s["y"], s["z"] = c[:, 12], c[:, 13], c[:, 14]
        s["cb"], s["cg"], s["cr"] = 0.3, 0.6, 0.9
        return s

    # the host-driven loop; the host form's depth plane persists over the ticks, as the atlas's does below
    want = []
    hc, hg = cams0.copy(), grav0.copy()
    for _ in range(ticks):
        hc, hg, _t = a.players_step(keys, hc, hg, tdiff=1 / 60, ticks=3)
        hc = np.ascontiguousarray(hc, np.float32).reshape(n, 16)
        a.set_objects(spheres_np(hc))
        want.append(tuple(x.copy() for x in a.trace_viewports(atlas[2], hc, secs)))
    a.close()
    dev = _dev()
    lay = b.viewports_layout(*atlas)
    s1 = torch.cuda.Stream(dev)
    got = []
    with torch.cuda.stream(s1):
        d_keys = torch.from_numpy(keys).to(dev)
        d_cams = torch.from_numpy(cams0.copy()).to(dev)
        d_grav = torch.from_numpy(grav0.copy()).to(dev)
        d_secs = torch.from_numpy(secs).to(dev)
        d_sph = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        d_sph[:, 0], d_sph[:, 1] = 0.25, 0.2
        d_sph[:, 5], d_sph[:, 6], d_sph[:, 7] = 0.3, 0.6, 0.9
        d_z = torch.zeros((40, 96), dtype=torch.float32, device=dev)
        d_work = torch.empty((40, 96), dtype=torch.int32, device=dev)
        for _ in range(ticks):
            b.players_step_device(d_keys, d_cams, d_grav, tdiff=1 / 60, ticks=3)
            d_sph[:, 2:5] = d_cams[:, 12:15]
            b.upload_spheres_device(d_sph, 4 * n)
            d_sb = torch.empty((40, 96), dtype=torch.int32, device=dev)
            b.trace_viewports_device(lay, d_cams, d_secs, d_sb, d_z, work=d_work)
            got.append((d_sb, d_z.clone()))
    s1.synchronize()
    for t in range(ticks):
        assert (got[t][0].cpu().numpy().view(np.uint32) == want[t][0]).all(), t
        assert (_bits(got[t][1].cpu().numpy()) == _bits(want[t][1])).all(), t
    assert any((want[t][0] != want[0][0]).any() for t in range(1, ticks))
    lay.free()
    b.close()


# ---------------------------------------------------------------- ownership ----

def _sequence(r, cams, blur, between):
    """(tests/test_gpu_views_device.py's sequence, with the host form of the viewports in it) blocking frames (depth persistence on
    synth256), host-form batches of views and viewports, frames in flight and upscale; device-form viewport calls in between when asked"""
    import torch
    out = []
    vp = [(0, 0, 240, 272), (240, 0, 240, 136)]
    lay = r.viewports_layout(CW + 32, CH - 8, [(0, 0, 64, 40), (64, 0, 32, 20)]) if between else None

    def device_call():
        if between:
            c = _Call((CW + 32, CH - 8, [(0, 0, 64, 40), (64, 0, 32, 20)]), np.stack([cams[0], cams[3]]), np.full(2, 0.5, np.float32))
            c.z.fill_(7.0)
            c.run(r, lay, blur)
            torch.cuda.synchronize()

    device_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    device_call()
    out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32)))
    out += list(r.trace_viewports(vp, np.stack([cams[1], cams[2]]), [0.0, 0.0]))
    device_call()
    out.append(r.screen_upscale(None, 2))
    out += list(r.trace_screen_centred(cams[0], 0.0))          # rays of cams[0] run out of steps: depth of cams[1] stays
    device_call()
    out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32)))
    out += list(r.trace_viewports(vp, np.stack([cams[0], cams[3]]), [0.0, 0.0]))      # ... and in the host form's depth plane
    r.frames_config(2, sbuf=True, zbuf=True)
    r.submit_frame(cams[3], 0.25, 0)
    r.submit_frame(cams[2], 0.5, 1)
    device_call()                                              # (beside frames in flight)
    for i in range(2):
        fr = r.wait_frame(i)
        out += [fr["sbuf"].copy(), fr["zbuf"].copy()]
    r.frames_config(0)
    device_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    if lay is not None:
        lay.free()
    return out


def test_other_calls_are_not_disturbed():
    """blocking frames, view slots, the host form's planes and depth and frames in flight, interleaved with device-form viewport
    calls, stay bit-identical to the same sequence without them"""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    w, h = 480, 272
    for blur in (0, 1):
        res = []
        for between in (False, True):
            r = _renderer(w, h, "synth256", "synth256", blur=blur)
            res.append(_sequence(r, cams, blur, between))
            r.close()
        assert len(res[0]) == len(res[1])
        for i, (a, b) in enumerate(zip(*res)):
            assert a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(), (blur, i)


# ---------------------------------------------------------------- refusals ----

def _raw(r, lay, cams, secs, flags, work, sb, z, stream=None):
    from pwnfps_amd._lib import lib
    return lib.pwn_trace_viewports_device(r._ctx if r is not None else None, lay, C.c_void_p(cams), C.c_void_p(secs), flags,
                                          C.c_void_p(work), C.c_void_p(sb), C.c_void_p(z), C.c_void_p(stream))


def test_refusals(oracle_lib):
    """every refusal leaves the planes as they were and the next valid call right"""
    import torch
    import pwnfps_amd
    level, key, blur = "pwnfps_level", "t0", 1
    W, H, rects = A
    cams, secs = _cams_for(oracle_lib, level, 5, 0)
    want = _ruler(level, key, A, blur, cams, secs)
    r = _devctx(level, key)
    r.set_blur_passes(blur)
    other = _renderer(CW, CH, level, key)
    la, lb, lo = r.viewports_layout(*A), r.viewports_layout(*B), other.viewports_layout(*A)
    dev = _dev()
    plane = W * H * 4
    # three planes in ONE allocation with a spare behind each, so that pointers can be shifted and made to overlap on purpose
    pool = torch.full((6, H, W), POISON, dtype=torch.int32, device=dev)
    p_work, p_sb, p_z = pool[0].data_ptr(), pool[2].data_ptr(), pool[4].data_ptr()
    t_cams = torch.from_numpy(cams.reshape(5, 16).copy()).to(dev)
    t_secs = torch.zeros(8, dtype=torch.float32, device=dev)
    pc, ps = t_cams.data_ptr(), t_secs.data_ptr()
    good = dict(lay=la._ptr, cams=pc, secs=ps, flags=0, work=p_work, sb=p_sb, z=p_z)
    assert _raw(None, **good) == PWN_EINVAL
    bad = [dict(lay=None), dict(cams=None), dict(secs=None), dict(sb=None), dict(z=None), dict(work=None),          # (blur is on)
           dict(lay=lo._ptr),                                                                                    # another context's layout
           dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(cams=pc + 4), dict(secs=ps + 4), dict(work=p_work + 4), dict(sb=p_sb + 8), dict(z=p_z + 12),
           dict(sb=p_z), dict(work=p_sb), dict(work=p_z),                                                        # two planes the same
           dict(sb=p_work + plane - 16), dict(z=p_sb + plane - 16), dict(work=p_z - plane + 16),                 # ... or a word in common
           dict(lay=lb._ptr)]                                                                                    # blur on, a layout without the blur rules
    for kw in bad:
        assert _raw(r, **dict(good, **kw)) == PWN_EINVAL, kw
    freed = r.viewports_layout(*A)
    fp = freed._ptr
    freed.free()
    assert _raw(r, **dict(good, lay=fp)) == PWN_EINVAL                                                          # a layout already freed
    from pwnfps_amd._lib import lib
    assert lib.pwn_viewports_layout_free(r._ctx, fp) == PWN_EINVAL and lib.pwn_viewports_layout_free(r._ctx, lo._ptr) == PWN_EINVAL
    # before a level; a pwn_init_multi handle; a row tiling
    nl = _renderer(CW, CH)
    ln = nl.viewports_layout(*A)                                                                                 # (creation needs no level)
    assert _raw(nl, **dict(good, lay=ln._ptr)) == PWN_ENOLEVEL
    nl.close()
    g = pwnfps_amd.Renderer(CW, CH, devices=[0, 0])
    g.level_load(level_path(level))
    g.set_objects(load_spheres(key))
    assert _raw(g, **good) == PWN_ENOTSUP
    with pytest.raises(pwnfps_amd.PwnError):
        g.viewports_layout(*A)
    g.close()
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert _raw(r, **good) == PWN_EBUSY
    r.tiled_shutdown()
    # layout creation: what pwn_viewports_plan refuses
    for W2, H2, rs in ((96, 40, [(0, 0, 96, 16), (95, 15, 1, 1)]), (96, 40, [(90, 0, 8, 8)]), (96, 40, [(0, 0, 0, 4)]), (0, 40, [(0, 0, 1, 1)]),
                       (96, 32769, [(0, 0, 1, 1)])):
        with pytest.raises(pwnfps_amd.PwnError):
            r.viewports_layout(W2, H2, rs)
    torch.cuda.synchronize()
    assert (pool.cpu().numpy().view(np.uint32) == POISON).all()                                                  # nothing was written by any of it
    # the same ranges, in order, are accepted (planes that touch are fine; no work plane with blur off), and the pixels are right
    assert _raw(r, **dict(good, work=p_sb - plane, z=p_sb + plane)) == 0
    r.set_blur_passes(0)
    assert _raw(r, **dict(good, work=None)) == 0
    assert _raw(r, **dict(good, lay=lb._ptr, work=None, sb=p_sb, z=p_z)) == 0                                    # (70 x 33 words of them)
    r.set_blur_passes(blur)
    torch.cuda.synchronize()
    _one_call(r, A, cams, secs, blur).check(want, "after the refusals")
    # the binding's own checks
    c = _Call(A, cams, secs)
    with pytest.raises(ValueError):
        r.trace_viewports_device(la, c.cams, c.secs, c.sb, c.z.view(torch.int32), work=c.work)                   # depth must be float32
    with pytest.raises(ValueError):
        r.trace_viewports_device(la, c.cams[:4], c.secs[:4], c.sb, c.z, work=c.work)                             # n is the layout's
    with pytest.raises(ValueError):
        r.trace_viewports_device(la, c.cams, c.secs, c.sb[:-1], c.z, work=c.work)
    with pytest.raises(ValueError):
        r.trace_viewports_device(la, c.cams.cpu(), c.secs, c.sb, c.z, work=c.work)
    with pytest.raises(ValueError):
        r.trace_viewports_device(lo, c.cams, c.secs, c.sb, c.z, work=c.work)                                     # another renderer's layout
    with pytest.raises(ValueError):
        r.trace_viewports_device(la, c.cams, torch.zeros(9, device=dev)[1:6], c.sb, c.z, work=c.work)            # not 16-byte aligned
    c.check((np.zeros((H, W), np.uint32), np.zeros((H, W), np.float32)), "refused by the binding", skip=range(5))
    la.free()
    lb.free()
    other.close()                                                                                                # (lo goes with its renderer)
    assert lo._ptr is None
