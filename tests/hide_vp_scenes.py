"""What the tests of pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device and pwn_trace_rays_hide_device share
(tests/test_gpu_*_hide.py for viewports and colour rays): the layout, the cameras, the calls, and the REFERENCES -- never the code
under test: the call without `_hide` on a context whose table is the t0 spheres with the hidden one taken out.  The scene, `without`,
`full_numbers`, the three cameras and the contexts are tests/hide_scenes.py's; references are computed once per hidden sphere and kept.

The device context is 64 x 48 -- of another size than the layout's frame and than any view.  Layout HV: a frame of 96 x 40 with four
rectangles, usable with blur (every x and w a multiple of 4).  Their units are 21, 16, 18 and 1, so the records' order (rising units:
3, 1, 2, 0) is not the caller's and `perm` is exercised; partial units in both directions (40 x 26: 2.5 x 6.5; 56 x 16: 3.5 units
across), one view wider than the context (96 > 64), one view of a single partial unit (4 x 4), and rows 16 .. 25 right of x = 44 and
the rest of rows 20 .. 25 covered by nothing."""
import functools

import numpy as np

import hide_scenes as S

CW, CH = 64, 48
FW, FH = 96, 40
RECTS = [(0, 0, 40, 26), (40, 0, 56, 16), (0, 26, 96, 12), (40, 16, 4, 4)]
HIDES = ([0, 1, 5, S.HIDE_NONE], [13, S.HIDE_NONE, 0, 0])
SECS = np.array([1.25, 0.0, 7.5, 1.25], np.float32)
POISON = S.POISON
RAY_SEC = 1.25
RAY_DEPTH0 = 3.5
RAY_HIDES = (-1, 0, 1, 5, 13)
RAY_POOL = 4097


def cameras():
    """hide_scenes' three cameras and camera 0 again"""
    c = S.cameras()
    return np.concatenate([c, c[:1]])


def inside_mask():
    m = np.zeros((FH, FW), bool)
    for x, y, w, h in RECTS:
        m[y:y + h, x:x + w] = True
    return m


def rect(a, i, rects=RECTS):
    x, y, w, h = rects[i]
    return a[y:y + h, x:x + w]


def context(form, spheres, **kw):
    return S.renderer(form, spheres, w=CW, h=CH, **kw)


def _dev():
    import torch
    return torch.device("cuda", 0)


def viewports_call(r, lay, cams, secs, hide=None, blur=0, stream=None, frame=(FW, FH)):
    """trace_viewports_device (hide given: pwn_trace_viewports_hide_device) on a stream of its own -> colour, depth bits, each (H,W)
    uint32.  Colour and work start poisoned, the depth plane at zero."""
    import torch
    dev = _dev()
    n = len(cams)
    s = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
        t_secs = torch.from_numpy(np.ascontiguousarray(secs, np.float32).copy()).to(dev)
        t_sb = torch.full((frame[1], frame[0]), POISON, dtype=torch.int32, device=dev)
        t_z = torch.zeros((frame[1], frame[0]), dtype=torch.float32, device=dev)
        t_work = torch.full((frame[1], frame[0]), POISON, dtype=torch.int32, device=dev) if blur > 0 else None
        t_hide = torch.tensor(list(hide), dtype=torch.int32, device=dev) if hide is not None else None
        r.trace_viewports_device(lay, t_cams, t_secs, t_sb, t_z, work=t_work, hide=t_hide)
        sb = t_sb.cpu().numpy().view(np.uint32)
        z = t_z.cpu().numpy().view(np.uint32)
    s.synchronize()
    return sb, z


GUARD = 4          # words in front of and behind every plane of viewport_hits_call


def viewport_hits_call(r, lay, cams, hide=None, cell=True, dist=True, stream=None, frame=(FW, FH)):
    """trace_viewport_hits_device (hide given: pwn_trace_viewport_hits_hide_device) -> label, cell, dist bits, each (H,W) uint32 or
    None.  Every plane lies between guard words, which are checked here; the planes start poisoned."""
    import torch
    dev = _dev()
    n = len(cams)
    words = frame[0] * frame[1]
    s = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(n, 16).copy()).to(dev)
        flat = [torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device=dev) if on else None for on in (True, cell, dist)]
        t_l, t_c, t_d = (None if f is None else f[GUARD:GUARD + words].view(frame[1], frame[0]) for f in flat)
        if t_d is not None:
            t_d = t_d.view(torch.float32)
        t_hide = torch.tensor(list(hide), dtype=torch.int32, device=dev) if hide is not None else None
        r.trace_viewport_hits_device(lay, t_cams, t_l, cell=t_c, dist=t_d, hide=t_hide)
        host = [None if f is None else f.cpu().numpy().view(np.uint32) for f in flat]
    s.synchronize()
    for f in host:
        assert f is None or ((f[:GUARD] == np.uint32(0xffffffff)).all() and (f[-GUARD:] == np.uint32(0xffffffff)).all())
    return tuple(None if f is None else f[GUARD:GUARD + words].reshape(frame[1], frame[0]) for f in host)


def relabel(label, k):
    """a reduced table's labels with the object field in the FULL table's numbering"""
    import pwnfps_amd
    obj = S.full_numbers(pwnfps_amd.unpack_labels(label)[2], k)
    return ((label & ~np.uint32(0x3fff << 5)) | ((obj + 1).astype(np.uint32) << np.uint32(5))).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(k):
    """The reference for "sphere k hidden": the calls without `_hide` on a 64 x 48 context that holds the t0 table without entry k
    (k = -1: the whole table), the tables in whatever form the library picks, layout HV with the four cameras and times.
    -> dict: (blur, "col" | "z") -> (FH,FW) uint32; "label" (full numbering), "cell", "dist"; ("stats", i) / ("hstats", i) -> the four
    counters of rectangle i traced alone, as a one-rectangle layout of the same frame, colour / first hits."""
    cams = cameras()
    out = {}
    with context(None, S.without(S.spheres_t0(), k)) as r:
        lay = r.viewports_layout(FW, FH, RECTS)
        for blur in (0, 1):
            r.set_blur_passes(blur)
            out[(blur, "col")], out[(blur, "z")] = viewports_call(r, lay, cams, SECS, blur=blur)
        r.set_blur_passes(0)
        label, out["cell"], out["dist"] = viewport_hits_call(r, lay, cams)
        out["label"] = relabel(label, k)
        lay.free()
        r.set_counters(True)
        for i in range(len(RECTS)):
            one = r.viewports_layout(FW, FH, RECTS[i:i + 1])
            viewports_call(r, one, cams[i:i + 1], SECS[i:i + 1])
            out[("stats", i)] = S.stats4(r.stats())
            viewport_hits_call(r, one, cams[i:i + 1])
            out[("hstats", i)] = S.stats4(r.stats())
            one.free()
    return out


# ---- colour rays ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ray_pool():
    """RAY_POOL rays in a fixed shuffled order: every pixel ray and seed of the three cameras at 40 x 26 (3120) and hand-made rays that
    start inside sphere 0 (r = 0.3) in directions all round, with seeds of their own; a hide value per ray drawn from RAY_HIDES.
    -> rays (n,8) float32, seeds (n,) uint32, hide (n,) int32"""
    import pwnfps_amd
    rng = np.random.default_rng(20)
    rays, seeds = [], []
    for cam in S.cameras():
        ry, sd, _ = pwnfps_amd.pixel_rays(S.W, S.H, cam)
        rays.append(np.asarray(ry, np.float32).reshape(-1, 8))
        seeds.append(np.asarray(sd, np.uint32))
    m = RAY_POOL - sum(len(a) for a in rays)
    s0 = S.spheres_t0()[0]
    hand = np.zeros((m, 8), np.float32)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    off = rng.uniform(-0.15, 0.15, size=(m, 3))            # |off| <= 0.26 < r
    hand[:, 0:3] = np.array([s0["x"], s0["y"], s0["z"]], np.float32) + off.astype(np.float32)
    hand[:, 3] = 1.0
    hand[:, 4:7] = d.astype(np.float32)
    rays.append(hand)
    seeds.append(rng.integers(0, 2 ** 31, size=m, dtype=np.uint32))
    rays, seeds = np.concatenate(rays), np.concatenate(seeds)
    order = rng.permutation(RAY_POOL)
    hide = rng.choice(np.array(RAY_HIDES, np.int32), size=RAY_POOL).astype(np.int32)
    # (the first ray, which is all that n = 1 traces: camera 0's pixel (30, 13), deep in the half of its frame where the CPU oracle sees
    # sphere 0 from inside, with sphere 0 hidden)
    first = S.W * (S.H // 2) + 30
    order = np.concatenate([[first], order[order != first]])
    hide[0] = 0
    return np.ascontiguousarray(rays[order]), np.ascontiguousarray(seeds[order]), hide


def rays_call(r, rays, seeds, hide=None, sec=RAY_SEC, depth0=RAY_DEPTH0, stream=None):
    """trace_rays_device (hide given: pwn_trace_rays_hide_device) -> colour (n,) uint32, depth bits (n,) uint32; the colours start
    poisoned, every depth at depth0 (in / out)"""
    import torch
    dev = _dev()
    n = len(rays)
    s = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t_rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
        t_seeds = torch.from_numpy(np.ascontiguousarray(seeds).view(np.int32).copy()).to(dev)
        t_col = torch.full((n,), POISON, dtype=torch.int32, device=dev)
        t_z = torch.full((n,), depth0, dtype=torch.float32, device=dev)
        t_hide = torch.from_numpy(np.ascontiguousarray(hide, np.int32).copy()).to(dev) if hide is not None else None
        r.trace_rays_device(t_rays, t_col, t_z, seeds=t_seeds, sec_current=sec, hide=t_hide)
        col = t_col.cpu().numpy().view(np.uint32)
        z = t_z.cpu().numpy().view(np.uint32)
    s.synchronize()
    return col, z


@functools.lru_cache(maxsize=None)
def ray_reference(k):
    """pwn_trace_rays_device of the whole pool on the t0 table without entry k -> colour, depth bits (a ray's result does not depend on
    the batch it is in: the first n of these are the reference of a batch of the pool's first n)"""
    rays, seeds, _ = ray_pool()
    with context(None, S.without(S.spheres_t0(), k)) as r:
        return rays_call(r, rays, seeds)
