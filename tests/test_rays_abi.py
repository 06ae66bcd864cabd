"""pwn_trace_rays without a GPU: the exports, the header's constants against the binding's, the C entries' argument checks,
Renderer's shape checks before it calls into the library, and pwn_pixel_rays against a NumPy restatement of the frame
kernel's add chain (screen.h:12-21)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_pixel_rays", "pwn_trace_rays", "pwn_trace_rays_device")


def _lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    from pwnfps_amd import _lib as binding
    return binding.lib


def test_entries_are_exported_and_bound():
    _lib()
    raw = C.CDLL(LIB)
    from pwnfps_amd import _lib as binding
    names = {n for n, _, _ in binding.ABI}
    for e in ENTRIES:
        assert hasattr(raw, e), e
        assert e in names, e


def test_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    from pwnfps_amd import _lib as binding
    m = re.search(r"^#define\s+PWN_RAYS_HAS_W\s+(\d+)", hdr, re.M)
    assert m is not None and int(m.group(1)) == binding.PWN_RAYS_HAS_W == 1
    m = re.search(r"^#define\s+PWN_RAYS_MAX\s+\(1\s*<<\s*(\d+)\)", hdr, re.M)
    assert m is not None and (1 << int(m.group(1))) == binding.PWN_RAYS_MAX == 1 << 28
    for e in ENTRIES:
        assert re.search(r"^int %s\(" % e, hdr, re.M), e


def test_c_entries_refuse_bad_arguments_without_a_context():
    lib = _lib()
    rays = np.zeros((4, 8), np.float32)
    col = np.zeros(4, np.uint32)
    z = np.zeros(4, np.float32)
    cam = np.eye(4, dtype=np.float32).ravel()
    xy = np.zeros((4, 2), np.int32)
    seeds = np.zeros(4, np.uint32)
    # NULL context
    assert lib.pwn_trace_rays(None, 4, rays.ctypes.data, None, 0.0, col.ctypes.data, z.ctypes.data) == PWN_EINVAL
    assert lib.pwn_trace_rays(None, 0, None, None, 0.0, col.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_trace_rays_device(None, 4, rays.ctypes.data, None, 0.0, 0, col.ctypes.data, z.ctypes.data, None) == PWN_EINVAL
    # pwn_pixel_rays needs no context: its own checks
    ok = lib.pwn_pixel_rays(8, 4, cam.ctypes.data, 4, xy.ctypes.data, rays.ctypes.data, seeds.ctypes.data)
    assert ok == 0
    assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, 0, None, None, None) == 0
    assert lib.pwn_pixel_rays(8, 4, None, 4, xy.ctypes.data, rays.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, -1, xy.ctypes.data, rays.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, (1 << 28) + 1, xy.ctypes.data, rays.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, 4, None, rays.ctypes.data, None) == PWN_EINVAL
    assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, 4, xy.ctypes.data, None, None) == PWN_EINVAL
    for w, h in ((0, 4), (8, 0), (-3, 4), (32769, 4), (8, 32769)):
        assert lib.pwn_pixel_rays(w, h, cam.ctypes.data, 4, xy.ctypes.data, rays.ctypes.data, None) == PWN_EINVAL, (w, h)
    for bad in ((8, 0), (0, 4), (-1, 0), (0, -1), (100, 100)):
        q = xy.copy()
        q[2] = bad
        assert lib.pwn_pixel_rays(8, 4, cam.ctypes.data, 4, q.ctypes.data, rays.ctypes.data, None) == PWN_EINVAL, bad


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _bare_renderer(monkeypatch):
    import pwnfps_amd
    from pwnfps_amd import render
    monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    return r


@pytest.mark.parametrize("kw", [
    dict(rays=np.zeros((3, 7), np.float32)),
    dict(rays=np.zeros(8, np.float32)),
    dict(rays=np.zeros((3, 8, 1), np.float32)),
    dict(rays=(np.zeros((3, 3)), np.zeros((2, 3)))),
    dict(rays=(np.zeros((3, 2)), np.zeros((3, 3)))),
    dict(rays=(np.zeros((3, 3)), np.zeros((3, 5)))),
    dict(rays=(np.zeros(3), np.zeros((3, 3)))),
    dict(rays=np.zeros((3, 8), np.float32), seeds=np.zeros(4, np.uint32)),
    dict(rays=np.zeros((3, 8), np.float32), seeds=np.zeros((3, 1), np.uint32)),
    dict(rays=np.zeros((3, 8), np.float32), depth=np.zeros(2, np.float32)),
    dict(rays=np.zeros((3, 8), np.float32), depth=np.zeros((1, 3), np.float32)),
])
def test_trace_rays_rejects_bad_shapes_before_the_call(monkeypatch, kw):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_rays(**kw)


@pytest.mark.parametrize("kw", [
    dict(cam=np.zeros(15, np.float32)),
    dict(cam=np.eye(4), xy=np.zeros((3, 3), np.int32)),
    dict(cam=np.eye(4), xy=np.zeros(6, np.int32)),
    dict(cam=np.eye(4), order="columns"),
])
def test_pixel_rays_rejects_bad_shapes_before_the_call(monkeypatch, kw):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.pixel_rays(**kw)


def test_trace_rays_device_rejects_bad_arguments_before_the_call(monkeypatch):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.trace_rays_device(0x1000, 0x2000, 0x3000)                 # pointers without n
    with pytest.raises(ValueError):
        r.trace_rays_device(0x1000, 0x2000, 0x3000, n=-1)
    with pytest.raises(ValueError):
        r.trace_rays_device(0x1000, 0x2000, 0x3000, n=(1 << 28) + 1)
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    with pytest.raises(ValueError):                                  # host tensors
        r.trace_rays_device(rays, torch.zeros(4, dtype=torch.int32), torch.zeros(4))


def test_trace_rays_passes_good_shapes_to_the_library():
    """(with no context behind it the library answers PWN_EINVAL: the call got through, w lanes filled in)"""
    import pwnfps_amd
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    for rays in (np.zeros((3, 8), np.float64), (np.zeros((3, 3)), np.zeros((3, 4))), [np.zeros((3, 4)), np.zeros((3, 3))]):
        with pytest.raises(pwnfps_amd.PwnError) as e:
            r.trace_rays(rays, seeds=[1, 2, 3], depth=[0.0, 1.0, 2.0])
        assert e.value.code == PWN_EINVAL
    from pwnfps_amd.render import _ray_records
    rec = _ray_records((np.ones((2, 3)), np.full((2, 3), 2.0)), "t")
    assert rec.dtype == np.float32 and rec.shape == (2, 8)
    assert (rec == np.array([1, 1, 1, 1, 2, 2, 2, 0], np.float32)).all()


# ---------------------------------------------------------------- pwn_pixel_rays against NumPy ----

def _ftz(a):
    """FTZ|DAZ on fp32: denormals are +-0 (the reference executable's MXCSR, the device's mode)"""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < np.float32(1.17549435e-38), np.copysign(np.float32(0), a), a).astype(np.float32)


def _numpy_rays(w, h, cam, xy, oracle_lib):
    """(cx*rdx + rayb) + y*rdy, then x - cx + 1 additions of rdx, in fp32 with FTZ|DAZ; rayb, rdx, rdy from pwno_frame_setup;
    seeds from pwno_pixel_seed"""
    L = oracle_lib.lib()
    cam = np.ascontiguousarray(cam, np.float32).reshape(16)
    rb, dx, dy = (np.zeros(4, np.float32) for _ in range(3))
    L.pwno_frame_setup(w, h, cam.ctypes.data, rb.ctypes.data, dx.ctypes.data, dy.ctypes.data)
    rb, dx, dy = _ftz(rb), _ftz(dx), _ftz(dy)
    rays = np.zeros((len(xy), 8), np.float32)
    seeds = np.zeros(len(xy), np.uint32)
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(xy):
            cx = np.float32(x & ~31)
            v = _ftz(_ftz(_ftz(cx * dx) + rb) + _ftz(np.float32(y) * dy))
            for _ in range(x - (x & ~31) + 1):
                v = _ftz(v + dx)
            rays[i, :4] = cam[12:16]
            rays[i, 4:] = v
            seeds[i] = L.pwno_pixel_seed(int(x), int(y), w)
    return rays, seeds


def _random_cam(rng, w_lanes):
    cam = rng.uniform(-2, 2, (4, 4)).astype(np.float32)
    cam[3, :3] = rng.uniform(-5, 70, 3)
    if not w_lanes:
        cam[:3, 3] = 0.0
        cam[3, 3] = 1.0
    return cam


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 5), (320, 240), (1920, 1080), (32768, 17)])
def test_pixel_rays_equal_the_numpy_chain(oracle_lib, w, h):
    import pwnfps_amd
    rng = np.random.default_rng(w * 7 + h)
    for k in range(6):
        cam = _random_cam(rng, w_lanes=k % 2 == 1)
        n = 200
        xy = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], 1).astype(np.int32)
        xy[0] = (w - 1, h - 1)
        xy[1] = (0, 0)
        rays, seeds, xy_out = pwnfps_amd.pixel_rays(w, h, cam, xy)
        want, wseeds = _numpy_rays(w, h, cam, xy, oracle_lib)
        assert (xy_out == xy).all()
        assert (rays.view(np.uint32) == want.view(np.uint32)).all(), (w, h, k)
        assert (seeds == wseeds).all(), (w, h, k)
        if k % 2 == 0:
            assert (rays[:, 3] == 1.0).all() and (rays[:, 7] == 0.0).all()          # an ordinary camera: the 3-lane rule


def test_pixel_rays_flush_denormals_like_the_device(oracle_lib):
    """a camera with denormal entries: the chain runs under FTZ|DAZ, as on the device and in the reference executable"""
    import pwnfps_amd
    w, h = 64, 8
    cam = np.eye(4, dtype=np.float32)
    cam[0, :3] = (3e-39, -2e-39, 1.0)
    cam[1, :3] = (1e-38, 5e-39, -4e-39)
    cam[2, :3] = (-6e-39, 0.5, 2e-39)
    cam[3, :3] = (10.5, 0.5, 20.5)
    xy = np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
    rays, seeds, _ = pwnfps_amd.pixel_rays(w, h, cam, xy)
    want, wseeds = _numpy_rays(w, h, cam, xy, oracle_lib)
    assert (rays.view(np.uint32) == want.view(np.uint32)).all()


def test_pixel_rays_orders_cover_the_frame():
    import pwnfps_amd
    cam = pwnfps_amd.spawn_camera([10, 20], 0.6)
    for w, h in ((40, 9), (16, 4), (1, 1), (33, 7)):
        a, sa, xa = pwnfps_amd.pixel_rays(w, h, cam, order="rows")
        b, sb, xb = pwnfps_amd.pixel_rays(w, h, cam, order="units")
        assert len(xa) == len(xb) == w * h
        assert (xa[:, 1] * w + xa[:, 0] == np.arange(w * h)).all()
        idx = xb[:, 1] * w + xb[:, 0]
        assert sorted(idx.tolist()) == list(range(w * h))
        assert (b.view(np.uint32) == a[idx].view(np.uint32)).all() and (sb == sa[idx]).all()
        if w % 16 == 0 and h % 4 == 0:
            u = xb[:64]
            assert (u[:, 0] == np.tile(np.arange(16), 4)).all() and (u[:, 1] == np.repeat(np.arange(4), 16)).all()
