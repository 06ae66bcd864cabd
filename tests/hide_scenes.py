"""What the tests of the *_hide_device calls share (tests/test_gpu_*_hide.py): the scene, the cameras, the four forms of the sphere
tables, and the REFERENCE -- which is never the code under test: the existing call without `_hide` on a context whose table is the
same spheres with the hidden one taken out.  References are computed once per (hidden sphere, form-independent) and kept.

Scene: pwnfps_level with the t0 spheres (14, all binned to cell (9, 5)), views of 40 x 26 (partial units in both directions).
Camera 0 sits at sphere 0's centre + (0.1, 0.05, 0), yaw 0 -- inside its own r = 0.3 body; camera 1 inside sphere 1 (r = 0.1),
camera 2 a tenth of a unit outside sphere 5, both turned towards their sphere's centre (on the CPU oracle hiding changes 530, 979 and
422 of the 1040 pixels)."""
import contextlib
import functools
import os

import numpy as np

from conftest import GOLD, level_path

W, H = 40, 26
LEVEL = "pwnfps_level"
HIDE_NONE = -1
FORMS = ("indexed", "inline", "global", "device")
FORM_CODE = {"indexed": 0, "inline": 1, "global": 2, "device": 2}      # sphere_tables()["form"] (tables.h PWN_LF_*)
MAX_PAIRS = 4096


def spheres_t0():
    return np.load(os.path.join(GOLD, "spheres_t0.npy"))


def without(spheres, k):
    """the table with entry k taken out and the order otherwise kept; a k that is no index takes nothing out"""
    return np.delete(spheres, k) if 0 <= k < len(spheres) else spheres.copy()


def full_numbers(obj, k):
    """object numbers of a reduced table (entry k taken out) in the full table's numbering: j -> j + (j >= k); -1 stays"""
    obj = np.asarray(obj).astype(np.int64)
    return np.where((obj >= 0) & (obj >= k), obj + 1, obj) if k >= 0 else obj


def cameras():
    import pwnfps_amd
    s = spheres_t0()
    cams = np.zeros((3, 4, 4), np.float32)
    for i, (k, off, yaw) in enumerate(((0, (0.1, 0.05, 0.0), 0.0), (1, (0.03, 0.02, 0.0), 4.0), (5, (0.0, 0.0, -0.2), 0.5))):
        cam = pwnfps_amd.spawn_camera((0, 0), ang_y=yaw)
        cam[3, :3] = (s["x"][k] + np.float32(off[0]), s["y"][k] + np.float32(off[1]), s["z"][k] + np.float32(off[2]))
        cams[i] = cam
    return cams


SECS = np.array([1.25, 0.0, 7.5], np.float32)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sphere_tensor(spheres):
    """(n, 8) float32 on the GPU, SPHERE_DTYPE's field order: what upload_spheres_device takes"""
    import torch
    a = np.ascontiguousarray(spheres).view(np.float32).reshape(len(spheres), 8).copy()
    return torch.from_numpy(a).to(torch.device("cuda", 0))


@contextlib.contextmanager
def renderer(form, spheres, blur=0, counters=False, force_hasw=False, w=W, h=H):
    """a context with `spheres` in force in the given form of the tables; PWN_SPHERE_LISTS stays set while the context lives"""
    import torch
    import pwnfps_amd
    forced = form if form in ("indexed", "inline", "global") else None
    with env(PWN_SPHERE_LISTS=forced, PWN_DBG_FORCE_HASW="1" if force_hasw else None):
        r = pwnfps_amd.Renderer(w, h)
        try:
            r.level_load(level_path(LEVEL))
            if form == "device":
                t = sphere_tensor(spheres)
                r.upload_spheres_device(t, MAX_PAIRS)
                st = r.spheres_device_state()
                assert st["in_force"] == 1 and st["n"] == len(spheres), st
            else:
                r.set_objects(spheres)
            r.set_blur_passes(blur)
            r.set_counters(counters)
            if form is not None:
                assert r.sphere_tables()["form"] == FORM_CODE[form], (form, r.sphere_tables())
            yield r
            torch.cuda.synchronize()
        finally:
            r.close()


POISON = -1


def views_call(r, cams, secs, hide=None, blur=0, stream=None):
    """trace_views_device (hide given: pwn_trace_views_hide_device) of the whole batch on a non-default stream -> colour (n,h,w)
    uint32, depth bits (n,h,w) uint32.  The depth planes start at 0, as a fresh context's view slots."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(cams)
    s = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
        t_secs = torch.from_numpy(np.ascontiguousarray(secs, np.float32).copy()).to(dev)
        t_sb = torch.full((n, r.h, r.w), POISON, dtype=torch.int32, device=dev)
        t_z = torch.zeros((n, r.h, r.w), dtype=torch.float32, device=dev)
        t_work = torch.full((n, r.h, r.w), POISON, dtype=torch.int32, device=dev) if blur > 0 else None
        t_hide = torch.tensor(list(hide), dtype=torch.int32, device=dev) if hide is not None else None
        r.trace_views_device(t_cams, t_secs, t_sb, t_z, work=t_work, hide=t_hide)
        sb = t_sb.cpu().numpy().view(np.uint32)
        z = t_z.cpu().numpy().view(np.uint32)
    s.synchronize()
    return sb, z


def view_hits_call(r, cams, hide=None, cell=True, dist=True):
    """trace_view_hits_device (hide given: pwn_trace_view_hits_hide_device) -> label, cell, dist bits, each (n,h,w) uint32 or None"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(cams)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
        t_l = torch.full((n, r.h, r.w), POISON, dtype=torch.int32, device=dev)
        t_c = torch.full((n, r.h, r.w), POISON, dtype=torch.int32, device=dev) if cell else None
        t_d = torch.full((n, r.h, r.w), float("nan"), dtype=torch.float32, device=dev) if dist else None
        t_hide = torch.tensor(list(hide), dtype=torch.int32, device=dev) if hide is not None else None
        r.trace_view_hits_device(t_cams, t_l, cell=t_c, dist=t_d, hide=t_hide)
        out = tuple(None if t is None else t.cpu().numpy().view(np.uint32) for t in (t_l, t_c, t_d))
    s.synchronize()
    return out


def stats4(st):
    """the counters of the exactness contract (sphere_tests is not one of them: include/pwnhip.h)"""
    return (st["rays"], st["steps"], st["portals"], st["exhausted"])


def stats5(st):
    return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])


@functools.lru_cache(maxsize=None)
def reference_views(k):
    """The reference for "sphere k hidden": pwn_trace_views_device on the t0 table without entry k (k = -1: the whole table), the
    tables in whatever form the library picks.  -> dict: (blur, "col" | "z") -> (3,h,w) uint32; ("stats", i) -> the four counters of
    view i traced alone (blur 0)."""
    cams = cameras()
    out = {}
    with renderer(None, without(spheres_t0(), k)) as r:
        for blur in (0, 1):
            r.set_blur_passes(blur)
            out[(blur, "col")], out[(blur, "z")] = views_call(r, cams, SECS, blur=blur)
        r.set_blur_passes(0)
        r.set_counters(True)
        for i in range(len(cams)):
            views_call(r, cams[i:i + 1], SECS[i:i + 1])
            out[("stats", i)] = stats4(r.stats())
    return out


@functools.lru_cache(maxsize=None)
def reference_view_hits(k):
    """pwn_trace_view_hits_device on the table without entry k -> (label, cell, dist) with the label's object field in the FULL
    table's numbering"""
    import pwnfps_amd
    with renderer(None, without(spheres_t0(), k)) as r:
        label, cell, dist = view_hits_call(r, cameras())
    obj = full_numbers(pwnfps_amd.unpack_labels(label)[2], k)
    relabel = (label & ~np.uint32(0x3fff << 5)) | ((obj + 1).astype(np.uint32) << np.uint32(5))
    return relabel.astype(np.uint32), cell, dist
