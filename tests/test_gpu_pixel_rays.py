"""pwn_pixel_rays_device on the GPU: every ray record and every seed bit-identical to the host's pwn_pixel_rays -- in both layouts of
the pixels and for the whole frame, over the batch sizes around a wave, for cameras with denormal entries, entries around FLT_MIN
and w components, beside a camera of NaN -- the formula's values for pixels outside the frame (a NumPy float32 restatement, on
cameras where no denormal can arise), wild pixels without a fault, guard words around every range, the rays traced against
pwn_trace_views_device's views, step -> aim -> hits on one stream against the host route, what the call leaves alone, its refusals,
and the Python wrapper's rules."""
import ctypes as C

import numpy as np
import pytest

import players_model as M
from conftest import level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_EBUSY, PWN_ENOTSUP = -1, -8, -9
SHARED = 1
POISON = np.uint32(0x7fc0dead)            # a NaN pattern no computation makes
GUARD = 64                                # words on both sides of every range (256 B: the range keeps its alignment)
F = np.float32
TINY = np.finfo(np.float32).tiny
SPAWN = (9, 4)


def _dev():
    import torch
    return torch.device("cuda", 0)


class Guarded:
    """`words` 32-bit words of device memory, poisoned, with poisoned guard words on both sides"""

    def __init__(self, words, fill=None):
        import torch
        self.words = int(words)
        self.t = torch.full((self.words + 2 * GUARD,), int(POISON), dtype=torch.int32, device=_dev())
        if fill is not None:
            self.t[GUARD:GUARD + self.words] = torch.from_numpy(np.ascontiguousarray(fill).view(np.int32).ravel()).to(_dev())
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def read(self):
        a = self.t.cpu().numpy().view(np.uint32)
        assert (a[:GUARD] == POISON).all() and (a[GUARD + self.words:] == POISON).all(), "a guard word was written"
        return a[GUARD:GUARD + self.words]


def _lib():
    from pwnfps_amd import _lib
    return _lib.lib


def _call(ctx, w, h, cams, m, xy, flags, seeds=True, stream=None):
    """one pwn_pixel_rays_device on guarded, poisoned ranges -> (rc, rays (T,8) uint32, seeds (T,) uint32 or None, Guarded work)"""
    import torch
    cams = np.ascontiguousarray(cams, F).reshape(-1, 16)
    n = len(cams)
    T = n * m
    g_cams = Guarded(16 * n, cams)
    g_xy = Guarded(xy.size, np.ascontiguousarray(xy, np.int32)) if xy is not None else None
    g_work, g_rays, g_seeds = Guarded(20 * n), Guarded(8 * T), Guarded(T)
    rc = _lib().pwn_pixel_rays_device(ctx, w, h, n, g_cams.ptr, m, g_xy.ptr if g_xy is not None else None, flags, g_work.ptr, g_rays.ptr,
                                      g_seeds.ptr if seeds else None, stream)
    torch.cuda.synchronize()
    assert (g_cams.read() == cams.view(np.uint32).ravel()).all()
    if g_xy is not None:
        assert (g_xy.read() == np.ascontiguousarray(xy, np.int32).view(np.uint32).ravel()).all()
    g_work.read()
    got_s = g_seeds.read()
    if not seeds:
        assert (got_s == POISON).all()
    return rc, g_rays.read().reshape(T, 8), got_s if seeds else None, g_work


def _host(w, h, cams, xy):
    """the host's pwn_pixel_rays per camera: xy (m,2) for all, or (n,m,2), or None = the frame row-major -> rays (n*m,8), seeds (n*m,) as uint32"""
    import pwnfps_amd
    cams = np.asarray(cams, F).reshape(-1, 16)
    rays, seeds = [], []
    for i, cam in enumerate(cams):
        r, s, _ = pwnfps_amd.pixel_rays(w, h, cam, None if xy is None else (xy if xy.ndim == 2 else xy[i]))
        rays.append(r)
        seeds.append(s)
    return np.concatenate(rays).view(np.uint32), np.concatenate(seeds)


def _cams(n):
    """spawn cameras turned by i, the second one pitched"""
    import pwnfps_amd
    return np.stack([pwnfps_amd.spawn_camera(SPAWN, ang_y=0.37 * i, ang_x=0.3 if i == 1 else 0.0).reshape(16) for i in range(n)]).astype(F)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d words differ, first at %s: got %#x want %#x" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def rdr():
    import pwnfps_amd
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    yield r
    r.close()


# ---------------------------------------------------------------- 1: guarded arrays ----

@pytest.mark.parametrize("per_camera", [False, True])
@pytest.mark.parametrize("w,h", [(33, 5), (48, 20)])
def test_guarded_arrays(rdr, w, h, per_camera):
    """the pixels around the tile's edges, the batch sizes around a wave, one pixel and 65 a camera, both layouts: the host's bits,
    every word written, every guard untouched"""
    P = np.array([(x, y) for y in (0, h - 1) for x in (0, 15, 16, 31, 32, w - 1)], np.int32)
    for n in (1, 2, 63, 64, 65, 130):
        cams = _cams(n)
        for m in (1, 65):
            if per_camera:
                xy = np.stack([P[(7 * i + np.arange(m)) % len(P)] for i in range(n)])
            else:
                xy = P[(n + np.arange(m)) % len(P)]
            rc, rays, seeds, _ = _call(rdr._ctx, w, h, cams, m, xy, 0 if per_camera else SHARED)
            assert rc == 0
            want_r, want_s = _host(w, h, cams, xy)
            assert (want_r != POISON).all()
            _same(rays, want_r, "rays %dx%d n %d m %d" % (w, h, n, m))
            _same(seeds, want_s, "seeds %dx%d n %d m %d" % (w, h, n, m))


# ---------------------------------------------------------------- 2: the whole frame ----

def test_whole_frame_is_the_hosts_and_traces_to_the_views():
    """d_xy NULL: the host's row-major rays; traced with their seeds from depth 0 they are the views of pwn_trace_views_device, colour
    and depth (no blur, zero depth planes)"""
    import pwnfps_amd
    import torch
    w, h, n = 48, 20, 3
    cams = _cams(n)
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    r.set_blur_passes(0)
    cams[:, 12:15] = pwnfps_amd.spawn_camera(r.get_level()[2]).reshape(16)[12:15]
    rc, rays, seeds, _ = _call(r._ctx, w, h, cams, w * h, None, SHARED)
    assert rc == 0
    want_r, want_s = _host(w, h, cams, None)
    _same(rays, want_r, "rays")
    _same(seeds, want_s, "seeds")
    # the wrapper, and what it returns handed on as it is
    dev = _dev()
    t_cams = torch.from_numpy(cams).to(dev)
    t_rays, t_seeds = r.pixel_rays_device(t_cams)
    assert tuple(t_rays.shape) == (n * w * h, 8) and tuple(t_seeds.shape) == (n * w * h,)
    col = torch.zeros(n * w * h, dtype=torch.int32, device=dev)
    depth = torch.zeros(n * w * h, dtype=torch.float32, device=dev)
    r.trace_rays_device(t_rays, col, depth, seeds=t_seeds)
    sb = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    zb = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    r.trace_views_device(t_cams, torch.zeros(n, dtype=torch.float32, device=dev), sb, zb)
    torch.cuda.synchronize()
    _same(t_rays.cpu().numpy().view(np.uint32), want_r, "the wrapper's rays")
    _same(t_seeds.cpu().numpy().view(np.uint32), want_s, "the wrapper's seeds")
    assert (col.cpu().numpy().reshape(n, h, w) == sb.cpu().numpy()).all()
    assert (depth.cpu().numpy().view(np.uint32).reshape(n, h, w) == zb.cpu().numpy().view(np.uint32)).all()
    assert len(np.unique(sb.cpu().numpy())) > 8
    r.close()


# ---------------------------------------------------------------- 3: hostile cameras ----

def _hostile_cameras():
    rng = np.random.default_rng(950)
    cams = _cams(64)
    d = F(2.0 ** -127)
    # 0: the sum of two denormals is the host's normal number, and reaches the ray because the set-up keeps it
    cams[0] = 0
    cams[0, 0:4] = d
    cams[0, 8:12] = d
    cams[0, 12:16] = (d, -d, F(1e-45), 1.0)
    # 1..3: denormal entries in every row, both signs
    for i in (1, 2, 3):
        cams[i] = (rng.integers(1, 1 << 23, 16).astype(np.uint32) | (rng.integers(0, 2, 16).astype(np.uint32) << 31)).view(F)
    # 4..35: entries of 2^-132 .. 2^-116, so that the set-up's products and sums, cx0 * rdx, y * rdy and the chain's sums land on both
    # sides of FLT_MIN
    for i in range(4, 36):
        e = rng.integers(-132, -115, 16).astype(np.float64)
        cams[i] = (np.ldexp(1.0 + rng.random(16), e.astype(int)) * rng.choice([-1.0, 1.0], 16)).astype(F)
    # 36..39: w components in every row
    for i in range(36, 40):
        cams[i, [3, 7, 11]] = rng.uniform(-1, 1, 3).astype(F)
        cams[i, 15] = F(0.75)
    # 40, 41: NaN, beside ordinary cameras
    cams[40] = np.nan
    cams[41, 5] = np.nan
    return cams


def test_hostile_cameras(rdr):
    assert F(2.0 ** -127) + F(2.0 ** -127) != 0          # (a process that flushes denormals proves nothing)
    w, h = 48, 20
    cams = _hostile_cameras()
    n = len(cams)
    xy = np.array([(x, y) for y in (0, 1, 7, h - 1) for x in (0, 1, 15, 31, 32, 33, w - 1)], np.int32)
    m = len(xy)
    rc, rays, seeds, _ = _call(rdr._ctx, w, h, cams, m, xy, SHARED)
    assert rc == 0
    with np.errstate(all="ignore"):
        want_r, want_s = _host(w, h, cams, xy)
    wf = want_r.view(F).reshape(n, m, 8)
    # (the cases are what they are meant to be)
    assert (wf[0, :, 4] == TINY).all() and (wf[0, :, 0] == F(2.0 ** -127)).all()
    low = wf[4:36, :, 4:8]
    assert (low == 0).sum() > 100 and ((np.abs(low) >= TINY) & (np.abs(low) < 2 * TINY)).sum() > 20 and (np.abs(low) >= 2 * TINY).sum() > 100
    assert ((low != 0) & (np.abs(low) < TINY)).sum() == 0          # the chain runs flushed
    assert (wf[36:40, :, 3] == F(0.75)).all() and (wf[36:40, :, 7] != 0).all()
    good = np.ones(n, bool)
    good[[40, 41]] = False
    got = rays.reshape(n, m, 8)
    _same(got[good], want_r.reshape(n, m, 8)[good], "the cameras beside the NaN")
    _same(got[:, :, 0:4], want_r.reshape(n, m, 8)[:, :, 0:4], "every origin, the NaN cameras' included: a copy")
    assert np.isnan(got.view(F)[40, :, 4:8]).all()
    _same(seeds, want_s, "seeds")


# ---------------------------------------------------------------- 4: pixels outside the frame ----

def _restated(w, h, cams, xy):
    """pwn_pixel_rays' formula in NumPy float32, every operation rounded on its own; xy (m,2), shared -> rays (n*m,8) uint32, seeds"""
    dimx, dimy = F(w), F(h)
    yrat = (-dimy) / dimx
    xsrat = F(-2.0) / dimx
    ysrat = (yrat + yrat) / dimy
    rays = np.zeros((len(cams), len(xy), 8), F)
    seeds = np.zeros((len(cams), len(xy)), np.uint32)
    for i, cam in enumerate(np.asarray(cams, F).reshape(-1, 16)):
        rayb = (cam[0:4] + cam[8:12]) + (-yrat) * cam[4:8]
        rdx = xsrat * cam[0:4]
        rdy = ysrat * cam[4:8]
        for j, (x, y) in enumerate(xy):
            x, y = int(x), int(y)
            cx0 = x & ~31
            steps = [rayb, rdx, rdy, F(cx0) * rdx, F(cx0) * rdx + rayb, F(y) * rdy]
            v = steps[4] + steps[5]
            for _ in range((x & 31) + 1):
                v = v + rdx
                steps.append(v)
            assert v.dtype == np.float32
            # no denormal arises anywhere: NumPy's arithmetic is then the flushed one's
            assert not any(((s != 0) & (np.abs(s) < TINY)).any() for s in steps)
            rays[i, j, 0:4] = cam[12:16]
            rays[i, j, 4:8] = v
            sd = ((x & 0xffffffff) + (y & 0xffffffff) * (y & 0xffffffff) * (w + 1)) & 0xffffffff
            sd = (sd * sd * sd) & 0xffffffff
            sd = (sd * sd * sd) & 0xffffffff
            seeds[i, j] = sd
    return rays.reshape(-1, 8).view(np.uint32), seeds.ravel()


def test_pixels_outside_the_frame(rdr):
    w, h = 48, 20
    cams = _cams(5)
    inside = np.array([(0, 0), (31, 3), (32, 19), (47, 7)], np.int32)
    r0, s0 = _restated(w, h, cams, inside)
    h0, hs0 = _host(w, h, cams, inside)
    _same(r0, h0, "the restatement is the host's formula (rays)")
    _same(s0, hs0, "the restatement is the host's formula (seeds)")
    outside = np.array([(-1, -1), (-32, 0), (w, h), (-32768, 65535), (65535, -32768), (-33, 5), (64, -7)], np.int32)
    rc, rays, seeds, _ = _call(rdr._ctx, w, h, cams, len(outside), outside, SHARED)
    assert rc == 0
    want_r, want_s = _restated(w, h, cams, outside)
    _same(rays, want_r, "rays")
    _same(seeds, want_s, "seeds")
    # wild values: unspecified records, PWN_OK, every word written and no guard touched (in both layouts)
    wild = np.array([(-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31), (2 ** 31 - 32, 0), (-2 ** 31 + 31, 1 << 30), (1 << 24, -(1 << 24))], np.int32)
    rc, rays, _, _ = _call(rdr._ctx, w, h, cams, len(wild), wild, SHARED)
    assert rc == 0 and (rays != POISON).all()
    rc, rays, _, _ = _call(rdr._ctx, w, h, cams, len(wild), np.stack([wild] * len(cams)), 0)
    assert rc == 0 and (rays != POISON).all()


# ---------------------------------------------------------------- 5: no seeds; the seed's wrap-around ----

def test_no_seeds_and_the_seed_words_wrap(rdr):
    w = h = 32768
    cams = _cams(3)
    xy = np.array([(0, 32767), (32767, 32767), (12345, 32767), (31, 1), (32767, 0)], np.int32)
    want_r, want_s = _host(w, h, cams, xy)
    assert 32767 * 32767 * 32769 > 1 << 32
    rc, rays, seeds, _ = _call(rdr._ctx, w, h, cams, len(xy), xy, SHARED)
    assert rc == 0
    _same(rays, want_r, "rays")
    _same(seeds, want_s, "seeds")
    # (_call itself looks at the range that would have been the seeds': still poison)
    rc, rays, seeds, _ = _call(rdr._ctx, w, h, cams, len(xy), xy, SHARED, seeds=False)
    assert rc == 0 and seeds is None
    _same(rays, want_r, "rays without seeds")


# ---------------------------------------------------------------- 6: the loop ----

def test_step_aim_hits_on_one_stream(rdr):
    """players_step_device, pixel_rays_device of the crosshair, trace_hits_device: one stream, nothing waited for between them; the
    records are the host route's -- the model's cameras, the host's pwn_pixel_rays, pwn_trace_hits"""
    import pwnfps_amd
    import torch
    w, h, n = 32, 16, 4096
    data, pmap = M.shipped_level()
    start = M.corpus_states(data, n, seed=77)
    start[1][:, 4:8] = [0, 1, 0, 0]
    want_state = M.model_step(data, pmap, start[0], 1 / 60, 5, *start[1:])
    cross = np.array([(w // 2, h // 2)], np.int32)
    want_rays = _host(w, h, want_state[0], cross)[0].view(F)
    want_hits = rdr.trace_hits(want_rays)
    # (the corpus has gravities with a w lane: some origins have w != 1, the host form then runs the 4-lane kernels by itself, and the
    # device form has to be told, as the header says)
    has_w = not ((want_rays[:, 3] == 1).all() and (want_rays[:, 7] == 0).all())
    assert has_w
    dev = _dev()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        keys = torch.from_numpy(np.array(start[0], np.uint8)).to(dev)
        t_cams = torch.from_numpy(np.array(start[1], F)).to(dev)
        grav = torch.from_numpy(np.array(start[2], F)).to(dev)
        trav = torch.from_numpy(np.array(start[3], np.int32)).to(dev)
        xy = torch.from_numpy(cross).to(dev)
        hits = torch.zeros((n, 12), dtype=torch.int32, device=dev)
        rdr.players_step_device(keys, t_cams, grav, trav, tdiff=1 / 60, ticks=5)
        rays, _ = rdr.pixel_rays_device(t_cams, xy, seeds=False)
        rdr.trace_hits_device(rays, hits, has_w=has_w)
        got_hits, got_rays = hits.cpu().numpy(), rays.cpu().numpy()
    s.synchronize()
    _same(got_rays.view(np.uint32), want_rays.view(np.uint32), "the crosshair rays")
    _same(got_hits.view(np.uint32), np.ascontiguousarray(want_hits).view(np.uint32).reshape(n, 12), "the hits")
    assert len(np.unique(want_hits["dist"])) > 100 and len(np.unique(want_hits["face"])) > 2


# ---------------------------------------------------------------- 7: refusals; what is left alone ----

def test_refusals_and_what_is_left_alone(rdr):
    import pwnfps_amd
    import torch
    L = _lib()
    w, h, n, m = 32, 16, 5, 3
    T = n * m
    cams = _cams(n)
    xy = np.array([(0, 0), (31, 15), (16, 8)], np.int32)
    g_cams, g_xy = Guarded(16 * n, cams), Guarded(2 * T, np.stack([xy] * n))
    g_work, g_rays, g_seeds = Guarded(20 * n), Guarded(8 * T), Guarded(T)
    pc, px, pw, pr, ps = g_cams.ptr, g_xy.ptr, g_work.ptr, g_rays.ptr, g_seeds.ptr

    def d(ctx, w_=w, h_=h, n_=n, c=pc, m_=m, x=px, f=0, wk=pw, r=pr, s=ps):
        return L.pwn_pixel_rays_device(ctx, w_, h_, n_, c, m_, x, f, wk, r, s, None)

    def untouched():
        torch.cuda.synchronize()
        return all((g.read() == POISON).all() for g in (g_work, g_rays, g_seeds))

    bare = pwnfps_amd.Renderer(32, 16)          # no level
    for ctx in (None, rdr._ctx, bare._ctx):
        for kw in (dict(w_=0), dict(w_=32769), dict(h_=0), dict(h_=32769), dict(n_=-1), dict(n_=(1 << 20) + 1), dict(m_=-1),
                   dict(n_=1 << 20, m_=257, f=SHARED), dict(n_=1 << 16, m_=1 << 16, f=SHARED), dict(f=2), dict(f=SHARED | 4),
                   dict(c=None), dict(wk=None), dict(r=None), dict(x=None), dict(x=None, f=SHARED), dict(x=None, w_=3, h_=1)):
            assert d(ctx, **kw) == PWN_EINVAL, kw
    for ctx in (rdr._ctx, bare._ctx):
        for kw in (dict(c=pc + 4), dict(c=pc + 8), dict(x=px + 4), dict(wk=pw + 8), dict(r=pr + 4), dict(s=ps + 2),              # a misaligned pointer
                   dict(x=pc + 64 * n - 8), dict(wk=pc + 64 * (n - 1)), dict(r=pw + 80 * n - 16), dict(s=pr + 32 * T - 4),      # two ranges overlap
                   dict(s=px + 8 * T - 4), dict(c=pr + 32 * T - 16), dict(wk=pr), dict(s=pc)):
            assert d(ctx, **kw) == PWN_EINVAL, kw
    assert untouched()
    # an empty call is PWN_OK and launches nothing; the call needs no level
    for ctx in (rdr._ctx, bare._ctx):
        assert d(ctx, n_=0) == 0 and d(ctx, m_=0) == 0 and d(ctx, n_=0, c=None, x=None, wk=None, r=None, s=None) == 0
    assert untouched()
    rc, rays, seeds, _ = _call(bare._ctx, w, h, cams, m, xy, SHARED)
    assert rc == 0
    want_r, want_s = _host(w, h, cams, xy)
    _same(rays, want_r, "before a level: rays")
    _same(seeds, want_s, "before a level: seeds")
    bare.close()
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(32, 16, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert d(g._ctx) == PWN_ENOTSUP
    g.close()
    assert untouched()
    # while the context runs a row tiling
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert d(r._ctx) == PWN_EBUSY
    r.tiled_shutdown()
    assert untouched()
    assert d(r._ctx) == 0          # the same context serves again
    torch.cuda.synchronize()
    _same(g_rays.read().reshape(T, 8), want_r, "after the refusals: rays")
    r.close()


def test_other_calls_are_not_disturbed():
    """the stats of a counted frame, the launch-order waits and a blocking frame, before and after calls in both layouts"""
    import pwnfps_amd
    r = pwnfps_amd.Renderer(48, 20)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    r.set_counters(True)
    cam = pwnfps_amd.spawn_camera(r.get_level()[2], ang_y=0.6).reshape(16)
    before = r.trace_screen_centred(cam, 0.25)
    st0, waits0 = r.stats(), r.launch_order_waits()
    cams = _cams(70)
    xy = np.array([(24, 10), (0, 0)], np.int32)
    for _ in range(3):
        assert _call(r._ctx, 48, 20, cams, 2, xy, SHARED)[0] == 0
        assert _call(r._ctx, 33, 5, cams, 2, np.stack([xy % (33, 5)] * 70), 0)[0] == 0
    assert r.stats() == st0 and r.launch_order_waits() == waits0
    after = r.trace_screen_centred(cam, 0.25)
    for a, b in zip(before, after):
        assert (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()
    st1 = r.stats()
    for k in ("rays", "steps", "portals", "sphere_tests", "exhausted"):
        assert st1[k] == st0[k], k
    assert r.launch_order_waits() == waits0
    r.close()


# ---------------------------------------------------------------- 8: the Python rules ----

class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


PY_REFUSALS = ["cams 4 bytes in", "cams float64", "cams (n,15)", "cams strided", "cams 1-d", "cams on the CPU", "xy int64", "xy (m,3)",
               "xy (n+1,m,2)", "xy 1-d", "xy strided", "xy 4 bytes in", "xy on the CPU", "shared with (n,m,2)", "not shared with (m,2)",
               "not shared with the whole frame", "width 0", "width 32769", "height 1.5", "rays (T,7)", "rays float64", "rays T-1 rows",
               "rays 4 bytes in", "rays strided", "seeds int64", "seeds T+1", "seeds on the CPU", "work (n,19)", "work n-1 rows",
               "work 4 bytes in", "work float64"]


@pytest.mark.parametrize("what", PY_REFUSALS)
def test_python_refuses_before_the_library_is_entered(monkeypatch, what):
    """pixel_rays_device's shape, dtype, contiguity, device and alignment rules on real GPU tensors, with the library replaced by an
    object that fails on any call: each raises ValueError first (and the good sets get through to the library)"""
    import torch
    from pwnfps_amd import render
    import pwnfps_amd
    dev = _dev()
    n, m = 6, 3
    T = n * m
    z = lambda shape, dt=torch.float32, **kw: torch.zeros(shape, dtype=dt, device=kw.get("device", dev))
    cbuf, xbuf, rbuf, wbuf = z(16 * n + 4), z(2 * m + 4, torch.int32), z(8 * T + 4), z(20 * n + 4)
    good = dict(cams=cbuf[:16 * n].view(n, 16), xy=xbuf[:2 * m].view(m, 2), rays=rbuf[:8 * T].view(T, 8), seeds=z(T, torch.int32),
                work=wbuf[:20 * n].view(n, 20))
    bad = {
        "cams 4 bytes in": dict(cams=cbuf[1:16 * n + 1].view(n, 16)),
        "cams float64": dict(cams=z((n, 16), torch.float64)),
        "cams (n,15)": dict(cams=z((n, 15))),
        "cams strided": dict(cams=z((n, 32))[:, ::2]),
        "cams 1-d": dict(cams=z(16 * n)),
        "cams on the CPU": dict(cams=z((n, 16), device="cpu")),
        "xy int64": dict(xy=z((m, 2), torch.int64)),
        "xy (m,3)": dict(xy=z((m, 3), torch.int32)),
        "xy (n+1,m,2)": dict(xy=z((n + 1, m, 2), torch.int32)),
        "xy 1-d": dict(xy=z(2 * m, torch.int32)),
        "xy strided": dict(xy=z((m, 4), torch.int32)[:, ::2]),
        "xy 4 bytes in": dict(xy=xbuf[1:2 * m + 1].view(m, 2)),
        "xy on the CPU": dict(xy=z((m, 2), torch.int32, device="cpu")),
        "shared with (n,m,2)": dict(xy=z((n, m, 2), torch.int32), shared=True),
        "not shared with (m,2)": dict(shared=False),
        "not shared with the whole frame": dict(xy=None, shared=False, rays=None, seeds=None),
        "width 0": dict(width=0), "width 32769": dict(width=32769), "height 1.5": dict(height=1.5),
        "rays (T,7)": dict(rays=z((T, 7))),
        "rays float64": dict(rays=z((T, 8), torch.float64)),
        "rays T-1 rows": dict(rays=z((T - 1, 8))),
        "rays 4 bytes in": dict(rays=rbuf[1:8 * T + 1].view(T, 8)),
        "rays strided": dict(rays=z((T, 16))[:, ::2]),
        "seeds int64": dict(seeds=z(T, torch.int64)),
        "seeds T+1": dict(seeds=z(T + 1, torch.int32)),
        "seeds on the CPU": dict(seeds=z(T, torch.int32, device="cpu")),
        "work (n,19)": dict(work=z((n, 19))),
        "work n-1 rows": dict(work=z((n - 1, 20))),
        "work 4 bytes in": dict(work=wbuf[1:20 * n + 1].view(n, 20)),
        "work float64": dict(work=z((n, 20), torch.float64)),
    }[what]
    for k in ("cams", "rays", "work"):
        assert good[k].data_ptr() % 16 == 0
    if "bytes in" in what:
        t = list(bad.values())[0]
        assert t.data_ptr() % 8 == 4 and t.is_contiguous()
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 32, 16, 0, None
    monkeypatch.setattr(render, "lib", _NoCall())
    with pytest.raises(ValueError):
        r.pixel_rays_device(**dict(good, **bad))
    # the good sets pass every check: it is the library that is reached
    for kw in (good, dict(good, cams=good["cams"].view(n, 4, 4), xy=z((n, m, 2), torch.int32), rays=good["rays"].view(n, m, 8), seeds=False, shared=False),
               dict(cams=good["cams"]), dict(cams=good["cams"], xy=good["xy"], width=33, height=5, shared=True, work=good["work"])):
        with pytest.raises(AssertionError, match="called into the library"):
            r.pixel_rays_device(**kw)
