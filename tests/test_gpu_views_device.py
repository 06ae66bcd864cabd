"""pwn_trace_views_device: a batch of views from cameras in device memory into planes in device memory, stream-ordered.  View i
is bit-identical, colour and depth, to view i of pwn_trace_views with the same cameras, times and blur passes, when the caller's
depth planes hold on entry what that call's view slots held; the camera set-up runs on the device (pwn_view_setup_kernel) and
gives the bits of the host's frame_setup, denormals included."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
PWN_VIEWS_MAX = 1024


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


def _renderer(w, h, level=None, spheres=None, blur=1):
    import pwnfps_amd
    r = pwnfps_amd.Renderer(w, h)
    if level is not None:
        r.level_load(level_path(level))
        r.set_objects(load_spheres(spheres))
    r.set_blur_passes(blur)
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stats5(st):
    return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])


def _enqueue(r, cams, secs, blur, has_w=False, zfill=0.0, work=True):
    """the tensors of one batch, made on torch's current stream, and the call on that stream; nothing is waited for"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(cams)
    t_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
    t_secs = torch.from_numpy(np.ascontiguousarray(secs, np.float32).copy()).to(dev)
    t_sb = torch.full((n, r.h, r.w), -1, dtype=torch.int32, device=dev)
    t_z = torch.full((n, r.h, r.w), float(zfill), dtype=torch.float32, device=dev)
    t_work = torch.full((n, r.h, r.w), -1, dtype=torch.int32, device=dev) if (blur > 0 or work) else None
    r.trace_views_device(t_cams, t_secs, t_sb, t_z, work=t_work, has_w=has_w)
    return t_sb, t_z, (t_cams, t_secs, t_work)


def _device_views(r, cams, secs, blur, has_w=False, zfill=0.0, work=True, stream=None):
    """one batch on a non-default stream -> (colour, depth) on the host"""
    import torch
    s = stream if stream is not None else torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(s):
        t_sb, t_z, keep = _enqueue(r, cams, secs, blur, has_w, zfill, work)
        sb = t_sb.cpu().numpy().view(np.uint32)
        z = t_z.cpu().numpy()
    s.synchronize()
    del keep
    return sb, z


# ---------------------------------------------------------------- goldens ----

GROUPS = [("pwnfps_level", "t0", 320, 240, 5), ("synth64", "synth64", 480, 272, 4)]


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
def test_golden_cases_in_batches(oracle_lib, cases, monkeypatch, force_hasw):
    """each group of golden cases as ONE batch on a non-default stream: pre (blur 0, no work plane), post (blur 1) and depth
    hashes per view with the depth planes zeroed, and the counters summed over the views"""
    if force_hasw:
        monkeypatch.setenv("PWN_DBG_FORCE_HASW", "1")       # (read when a context is created)
    for level, key, w, h, count in GROUPS:
        cs = [c for c in cases if c["level"] == level and c["spheres"] == key and c["w"] == w and c["h"] == h]
        assert len(cs) == count, (level, w, h)
        if level == "pwnfps_level":
            assert sorted({c["sec"] for c in cs}) == [0.0, 1.5, 12.25, 1000.5]
        cams = np.array([c["cam"] for c in cs], np.float32)
        secs = np.array([c["sec"] for c in cs], np.float32)
        r = _renderer(w, h, level, key, blur=0)
        r.set_counters(True)
        pre, z = _device_views(r, cams, secs, 0, work=False)
        st = r.stats()
        for i, c in enumerate(cs):
            assert oracle_lib.fnv64(pre[i]) == c["pre"], c["name"]
            assert oracle_lib.fnv64(z[i]) == c["z"], c["name"]
        want = tuple(sum(c[k] for c in cs) for k in ("rays", "steps", "portals", "sphere_tests", "exhausted"))
        assert _stats5(st) == want, (level, w, h)
        r.set_counters(False)
        r.set_blur_passes(1)
        post, z = _device_views(r, cams.reshape(-1, 4, 4), secs, 1)
        for i, c in enumerate(cs):
            assert oracle_lib.fnv64(post[i]) == c["post"], c["name"]
            assert oracle_lib.fnv64(z[i]) == c["z"], c["name"]
        r.close()


# ---------------------------------------------------------------- against the host form ----

def _random_cams(rng, oracle_lib, level, n, w_frac=0.0):
    """(tests/test_gpu_views.py's cameras: somewhere in a free cell, turned and tilted; a share of them with w components)"""
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
        if rng.uniform() < w_frac:
            cam[:, 3] = (0.03, -0.01, 0.05, 0.8)
        cams[i] = cam
    secs = rng.uniform(0, 50, n).astype(np.float32)
    return cams, secs


def _host_views(w, h, level, key, blur, cams, secs):
    """Renderer.trace_views on a fresh context: every view slot's depth starts at zero"""
    r = _renderer(w, h, level, key, blur=blur)
    sb, z = r.trace_views(cams, secs)
    r.close()
    return sb, z


def _check_case(oracle_lib, rng, w, h, n, level="pwnfps_level", key="t0", blurs=(0, 1, 2)):
    with_w = _random_cams(rng, oracle_lib, level, n, w_frac=0.5)
    plain = _random_cams(rng, oracle_lib, level, n)
    r = _renderer(w, h, level, key)
    for blur in blurs:
        r.set_blur_passes(blur)
        for (cams, secs), flags in ((with_w, (True,)), (plain, (False, True))):
            want, want_z = _host_views(w, h, level, key, blur, cams, secs)
            for has_w in flags:
                sb, z = _device_views(r, cams, secs, blur, has_w=has_w)
                assert sb.shape == (n, h, w) and z.shape == (n, h, w)
                assert (sb == want).all(), (w, h, n, blur, has_w, int((sb != want).sum()))
                assert (_bits(z) == _bits(want_z)).all(), (w, h, n, blur, has_w)
    r.close()


@pytest.mark.parametrize("n", [1, 3, 7, 64])
@pytest.mark.parametrize("w,h", [(40, 20), (16, 4), (64, 36)])
def test_batch_equals_host_form(oracle_lib, w, h, n):
    """40 x 20: a partly filled unit column; 16 x 4: one unit per view; n = 3 and 7: the division by n that is no shift"""
    _check_case(oracle_lib, np.random.default_rng(20261018 + 1000 * w + n), w, h, n)


def test_views_max_equals_host_form(oracle_lib):
    _check_case(oracle_lib, np.random.default_rng(1024), 16, 4, PWN_VIEWS_MAX)


def test_sphere_lists_in_device_memory(oracle_lib):
    with _env(PWN_SPHERE_LISTS="global"):
        r = _renderer(64, 36, "pwnfps_level", "t0")
        assert r.sphere_tables()["form"] == 2
        r.close()
        _check_case(oracle_lib, np.random.default_rng(2), 40, 20, 7, blurs=(1,))


# ---------------------------------------------------------------- the set-up kernel's records ----

def _hostile_cameras(rng, xsrat, ysrat):
    """64 cameras: random ones, then every special value in every place of the formulas"""
    f = np.float32
    cams = rng.uniform(-2, 2, (64, 16)).astype(np.float32)
    d = f(2.0 ** -127)                                    # a denormal whose double is normal
    cams[8, 0:4] = d; cams[8, 8:12] = d; cams[8, 4:8] = 0.0        # c0 + c8: two denormals, a normal sum
    cams[9, 0:4] = d; cams[9, 8:12] = -d                 # ... that cancel
    cams[10, 0:4] = f(2.0 ** -149); cams[10, 8:12] = f(2.0 ** -149)
    cams[11, :] = d                                       # every product and sum of denormals
    cams[12, :] = f(2.0 ** -140)
    # entries whose product with xsrat / ysrat is denormal (and ones where it is just normal)
    for row, e in ((13, -126), (14, -122), (15, -118)):
        cams[row, 0:4] = f(2.0 ** e) / abs(xsrat) * f(0.75)
        cams[row, 4:8] = f(2.0 ** e) / abs(ysrat) * f(-0.75)
    cams[16, :] = 0.0
    cams[17, :] = -0.0
    cams[18, 0:4] = 0.0; cams[18, 8:12] = -0.0; cams[18, 4:8] = -0.0
    cams[19, :] = 3e38                                    # c0 + c8 overflows
    cams[20, :] = -3e38
    cams[21, 0:4] = 3e38; cams[21, 8:12] = -3e38; cams[21, 4:8] = 3e38          # ... cancels, and (3 x 7) yrat * c4 overflows
    cams[22, :] = np.inf
    cams[23, 0:4] = np.inf; cams[23, 8:12] = -np.inf     # inf - inf
    cams[24, 4:8] = -np.inf
    cams[25, :] = np.nan
    cams[26, 0] = np.nan; cams[26, 5] = np.nan; cams[26, 10] = np.nan; cams[26, 15] = np.nan
    cams[27, 12:16] = (d, -0.0, np.inf, np.nan)           # `from` is copied as it is
    secs = rng.uniform(0, 50, 64).astype(np.float32)
    secs[8], secs[9], secs[10], secs[11] = d, -0.0, np.inf, 1e-45
    return cams, secs


def _records_restated(cams, secs, w, h):
    """frame_setup's four formulas in float32, every operation rounded on its own"""
    f = np.float32
    dimx, dimy = f(w), f(h)
    yrat = (-dimy) / dimx
    xsrat = f(-2.0) / dimx
    ysrat = (yrat + yrat) / dimy
    assert all(v.dtype == np.float32 for v in (yrat, xsrat, ysrat))
    c0, c4, c8, c12 = cams[:, 0:4], cams[:, 4:8], cams[:, 8:12], cams[:, 12:16]
    rec = np.zeros((len(cams), 20), np.float32)
    with np.errstate(all="ignore"):
        s = c0 + c8
        m = (-yrat) * c4
        rec[:, 0:4] = s + m
        rec[:, 4:8] = xsrat * c0
        rec[:, 8:12] = ysrat * c4
    rec[:, 12:16] = c12
    rec[:, 16] = secs
    return rec, xsrat, ysrat


@pytest.mark.parametrize("w,h", [(320, 240), (40, 20), (3, 7)])
def test_setup_kernel_records(w, h):
    """pwn_launch_view_setup by itself: the 80-byte records as bits against the restatement; any NaN where that has NaN"""
    import torch
    from pwnfps_amd._lib import lib
    assert np.float32(2 ** -127) + np.float32(2 ** -127) != 0          # (a process that flushes denormals proves nothing)
    _, xsrat, ysrat = _records_restated(np.zeros((1, 16), np.float32), np.zeros(1, np.float32), w, h)
    cams, secs = _hostile_cameras(np.random.default_rng(w * 100 + h), xsrat, ysrat)
    want, _, _ = _records_restated(cams, secs, w, h)
    # (the cases are what they are meant to be)
    tiny = np.finfo(np.float32).tiny
    assert (want[8, 0:4] == tiny).all()
    assert (abs(want[13, 4:8]) < tiny).all() and (want[13, 4:8] != 0).all() and (abs(want[13, 8:12]) < tiny).all() and (want[13, 8:12] != 0).all()
    assert np.isinf(want[19, 0:4]).all() and np.isnan(want[23, 0:4]).all() and np.isnan(want[25, 0:12]).all()
    dev = torch.device("cuda", 0)
    n = len(cams)
    t_cams = torch.from_numpy(cams).to(dev)
    t_secs = torch.from_numpy(secs).to(dev)
    t_out = torch.full((n + 1, 20), 7.0, dtype=torch.float32, device=dev)
    fn = lib.pwn_launch_view_setup
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert t_cams.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0
    assert fn(t_cams.data_ptr(), t_secs.data_ptr(), t_out.data_ptr(), n, w, h, torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    got = t_out.cpu().numpy()
    assert (got[n] == 7.0).all()                              # nothing behind the n records
    got = got[:n]
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all()
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(~nan & (gb != wb))
    assert len(bad) == 0, [(int(i), int(k), hex(gb[i, k]), hex(wb[i, k])) for i, k in bad[:8]]
    assert (gb[:, 17:20] == 0).all()                          # the padding


# ---------------------------------------------------------------- depth in / out ----

def test_exhausted_rays_keep_the_callers_depth(oracle_lib, cases):
    """synth256 cam0: the primary ray that runs out of steps keeps the sentinel the caller's plane came in with"""
    c = next(x for x in cases if x["name"] == "synth256_cam0_480x272")
    assert c["exhausted"] == 1
    w, h = c["w"], c["h"]
    cam = np.array(c["cam"], np.float32)
    sentinel = np.float32(-12345.5)
    O = oracle_lib.Oracle()
    O.load_level(level_path("synth256"))
    O.set_spheres(load_spheres("synth256"))
    sb, zb, st = O.trace_rows(w, h, 0, h, cam, sec=np.float32(c["sec"]), zb=np.full((h, w), sentinel, np.float32))
    assert st.exhausted == 1
    r = _renderer(w, h, "synth256", "synth256", blur=0)
    r.set_counters(True)
    col, z = _device_views(r, np.stack([cam, cam]), np.full(2, c["sec"], np.float32), 0, zfill=sentinel)
    assert r.stats()["exhausted"] == 2
    for i in range(2):
        assert (col[i] == sb).all() and (_bits(z[i]) == _bits(zb)).all()
        assert (z[i] == sentinel).sum() >= 1
    r.close()


# ---------------------------------------------------------------- stream order and record rotation ----

@pytest.fixture(scope="module")
def four_batches(oracle_lib):
    """four camera sets of 64 views of 320 x 240 and what the host form renders for them, each on a fresh context"""
    rng = np.random.default_rng(64)
    sets = [_random_cams(rng, oracle_lib, "pwnfps_level", 64) for _ in range(4)]
    want = [_host_views(320, 240, "pwnfps_level", "t0", 1, cams, secs) for cams, secs in sets]
    return sets, want


@pytest.mark.parametrize("streams", [1, 2], ids=["one_stream", "two_alternating"])
def test_four_batches_without_synchronisation(four_batches, streams):
    """the batches' records rotate with the work-queue counter sets: nothing is overwritten while a launch may read it"""
    import torch
    sets, want = four_batches
    dev = torch.device("cuda", 0)
    st = [torch.cuda.Stream(dev) for _ in range(streams)]
    r = _renderer(320, 240, "pwnfps_level", "t0", blur=1)
    waits = r.launch_order_waits()
    outs = []
    for k, (cams, secs) in enumerate(sets):
        with torch.cuda.stream(st[k % streams]):
            outs.append(_enqueue(r, cams, secs, 1))
    assert r.launch_order_waits() == waits
    torch.cuda.synchronize()
    for k, (t_sb, t_z, _) in enumerate(outs):
        assert (t_sb.cpu().numpy().view(np.uint32) == want[k][0]).all(), (streams, k)
        assert (_bits(t_z.cpu().numpy()) == _bits(want[k][1])).all(), (streams, k)
    r.close()


# ---------------------------------------------------------------- no disturbance ----

def _sequence(r, cams, blur, between):
    """(tests/test_gpu_rays.py's sequence) blocking frames (depth persistence on synth256), host-form view batches, frames in flight
    and upscale; device-form view batches in between when asked"""
    import torch
    out = []

    def device_batch():
        if between:
            keep = _enqueue(r, np.stack([cams[0], cams[3], cams[1]]), np.full(3, 0.5, np.float32), blur, zfill=7.0)
            torch.cuda.synchronize()
            del keep

    device_batch()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    device_batch()
    out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32)))
    device_batch()
    out.append(r.screen_upscale(None, 2))
    out += list(r.trace_screen_centred(cams[0], 0.0))          # rays of cams[0] run out of steps: depth of cams[1] stays
    device_batch()
    out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32)))
    r.frames_config(2, sbuf=True, zbuf=True)
    r.submit_frame(cams[3], 0.25, 0)
    r.submit_frame(cams[2], 0.5, 1)
    device_batch()
    for i in range(2):
        fr = r.wait_frame(i)
        out += [fr["sbuf"].copy(), fr["zbuf"].copy()]
    r.frames_config(0)
    device_batch()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    return out


def test_other_calls_are_not_disturbed(oracle_lib):
    """blocking frames, frames in flight, host-form batches and upscale, interleaved with device-form batches, stay bit-identical
    to the same sequence without them"""
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

class _Planes:
    """three ranges of n planes in ONE allocation, a spare plane behind each: pointers can be shifted and made to overlap on purpose"""

    def __init__(self, n, w, h):
        import torch
        dev = torch.device("cuda", 0)
        self.n = n
        self.cams = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        self.secs = torch.zeros(n + 4, dtype=torch.float32, device=dev)
        self.pool = torch.zeros((3 * n + 3, h, w), dtype=torch.int32, device=dev)
        self.t_work, self.t_sb = self.pool[0:n], self.pool[n + 1:2 * n + 1]
        self.t_z = self.pool[2 * n + 2:3 * n + 2].view(torch.float32)
        self.work, self.sb, self.z = self.t_work.data_ptr(), self.t_sb.data_ptr(), self.t_z.data_ptr()
        self.plane = w * h * 4

    def set_cams(self, cams, secs):
        import torch
        self.cams.copy_(torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(-1, 16)))
        self.secs[:len(secs)].copy_(torch.from_numpy(np.ascontiguousarray(secs, np.float32)))

    def args(self, **kw):
        a = dict(n=self.n, cams=self.cams.data_ptr(), secs=self.secs.data_ptr(), flags=0, work=self.work, sb=self.sb, z=self.z)
        a.update(kw)
        return a


def _call(r, n, cams, secs, flags, work, sb, z, stream=None):
    from pwnfps_amd._lib import lib
    return lib.pwn_trace_views_device(r._ctx if r is not None else None, n, C.c_void_p(cams), C.c_void_p(secs), flags,
                                      C.c_void_p(work), C.c_void_p(sb), C.c_void_p(z), C.c_void_p(stream))


def _ok_after(r, cams, secs, blur, golden=None, oracle_lib=None):
    """a correct call on the same context gives the right frame: the host form's on this context, or the golden's hash"""
    sb, z = _device_views(r, cams, secs, blur)
    want, want_z = r.trace_views(cams, secs)
    assert (sb == want).all() and (_bits(z) == _bits(want_z)).all()
    if golden is not None:
        assert oracle_lib.fnv64(sb[0]) == golden["post"] and oracle_lib.fnv64(z[0]) == golden["z"]


def test_refusals(oracle_lib, cases):
    import torch
    import pwnfps_amd
    c = next(x for x in cases if x["name"] == "level_spawn_320x240")
    assert c["exhausted"] == 0
    w, h = c["w"], c["h"]
    cams = np.tile(np.array(c["cam"], np.float32), (4, 1))
    secs = np.full(4, c["sec"], np.float32)
    P = _Planes(4, w, h)
    P.set_cams(cams, secs)
    r = _renderer(w, h, "pwnfps_level", "t0", blur=1)
    assert _call(None, **P.args()) == PWN_EINVAL
    b2 = 2 * P.plane                                    # the bytes of a range of two views
    bad = [dict(cams=None), dict(secs=None), dict(sb=None), dict(z=None), dict(work=None),          # (blur is on)
           dict(n=0), dict(n=-3), dict(n=PWN_VIEWS_MAX + 1),
           dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(cams=P.cams.data_ptr() + 4), dict(secs=P.secs.data_ptr() + 4), dict(work=P.work + 4), dict(sb=P.sb + 8), dict(z=P.z + 12),
           dict(sb=P.z), dict(work=P.sb), dict(work=P.z),                                           # two planes the same
           dict(n=2, sb=P.work + b2 - 16), dict(n=2, z=P.sb + b2 - 16), dict(n=2, work=P.z + b2 - 16)]        # ... or a word in common
    for kw in bad:
        torch.cuda.synchronize()
        assert _call(r, **P.args(**kw)) == PWN_EINVAL, kw
        _ok_after(r, cams[:1], secs[:1], 1, c, oracle_lib)
    # (ranges that touch are fine, and so is no work plane with blur off)
    assert _call(r, **P.args(n=2, sb=P.work + b2, z=P.work + 2 * b2)) == 0
    r.set_blur_passes(0)
    assert _call(r, **P.args(work=None)) == 0
    torch.cuda.synchronize()
    r.set_blur_passes(1)
    # more than 2^28 pixels in the batch
    big = _renderer(4096, 4096, "pwnfps_level", "t0", blur=0)
    assert _call(big, **P.args(n=17, work=None)) == PWN_EINVAL
    _ok_after(big, cams[:1], secs[:1], 0)
    big.close()
    # w % 4 != 0 with blur on
    odd = _renderer(322, 200, "pwnfps_level", "t0", blur=1)
    assert _call(odd, **P.args(n=2)) == PWN_EINVAL
    odd.set_blur_passes(0)
    _ok_after(odd, cams[:2], secs[:2], 0)
    odd.close()
    # before a level
    nl = _renderer(w, h)
    assert _call(nl, **P.args()) == PWN_ENOLEVEL
    nl.level_load(level_path("pwnfps_level"))
    nl.set_objects(load_spheres("t0"))
    _ok_after(nl, cams[:2], secs[:2], 1, c, oracle_lib)
    nl.close()
    # a pwn_init_multi handle, one ordinal twice
    g = pwnfps_amd.Renderer(w, h, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    g.set_objects(load_spheres("t0"))
    assert _call(g, **P.args()) == PWN_ENOTSUP
    with pytest.raises(pwnfps_amd.PwnError):
        g.trace_views_device(P.cams, P.secs[:4], P.t_sb, P.t_z, work=P.t_work)
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert _call(r, **P.args()) == PWN_EBUSY
    r.tiled_shutdown()
    _ok_after(r, cams, secs, 1, c, oracle_lib)
    # the binding's own checks
    with pytest.raises(ValueError):
        r.trace_views_device(P.cams, P.secs[:4], P.t_sb, P.t_z.view(torch.int32), work=P.t_work)          # depth must be float32
    with pytest.raises(ValueError):
        r.trace_views_device(P.cams, P.secs[:3], P.t_sb, P.t_z, work=P.t_work)
    with pytest.raises(ValueError):
        r.trace_views_device(P.cams.cpu(), P.secs[:4], P.t_sb, P.t_z, work=P.t_work)
    with pytest.raises(ValueError):
        r.trace_views_device(P.cams, P.secs[:4], P.t_sb[:, :-1], P.t_z, work=P.t_work)
    r.close()
