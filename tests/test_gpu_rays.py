"""pwn_trace_rays: caller-supplied rays through the level.  Ray i is trace_ray (trace.h:186) from its own origin, direction, seed
and entry depth: bit-identical, colour and depth, to the pixel of the pre-blur frame that pwn_pixel_rays made it from, and to
the oracle on any ray with a pixel's seed (the oracle trick: a camera whose x and y rows are zero, z row D and w row O gives every
pixel of its frame the ray (O, D) exactly).

Time limit: the module runs in well under 300 s on one MI355X (most of it the oracle on the hard scenes and the trick batches).
"""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
from conftest import GOLD, level_path, load_spheres
from oracle import SPHERE_DTYPE

pytestmark = pytest.mark.gpu

SCENES = HS.scenes(SPHERE_DTYPE)
IDS = [s.name for s in SCENES]
PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9


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


def _renderer(level=None, spheres=None, w=64, h=64, env=None):
    import pwnfps_amd
    with _env(**(env or {})):
        r = pwnfps_amd.Renderer(w, h)
    if level is not None:
        r.level_load(level_path(level))
        r.set_objects(load_spheres(spheres))
    r.set_blur_passes(0)
    return r


def _plane(col, z, xy, w, h):
    """the rays' results back on the frame's pixels"""
    pre = np.zeros((h, w), np.uint32)
    zz = np.zeros((h, w), np.float32)
    pre[xy[:, 1], xy[:, 0]] = col
    zz[xy[:, 1], xy[:, 0]] = z
    return pre, zz


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- golden frames ----

@pytest.mark.parametrize("order", ["rows", "units"])
@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
def test_golden_frames_as_rays(oracle_lib, cases, order, force_hasw):
    """every pixel of every golden case up to 1920x1080 as a ray: colour hashes to `pre`, depth to `z`, counters equal"""
    import pwnfps_amd
    env = {"PWN_DBG_FORCE_HASW": "1"} if force_hasw else {}
    done = 0
    ctxs = {}
    for c in cases:
        if c["w"] * c["h"] > 1920 * 1080 or "rays" not in c:
            continue
        key = (c["level"], c["spheres"])
        if key not in ctxs:
            ctxs[key] = _renderer(c["level"], c["spheres"], env=env)
            ctxs[key].set_counters(True)
        r = ctxs[key]
        rays, seeds, xy = pwnfps_amd.pixel_rays(c["w"], c["h"], np.array(c["cam"], np.float32), order=order)
        col, z = r.trace_rays(rays, seeds, c["sec"])
        st = r.stats()
        pre, zz = _plane(col, z, xy, c["w"], c["h"])
        assert oracle_lib.fnv64(pre) == c["pre"], (c["name"], order)
        assert oracle_lib.fnv64(zz) == c["z"], (c["name"], order)
        assert HS.stats5(st) == tuple(c[k] for k in ("rays", "steps", "portals", "sphere_tests", "exhausted")), c["name"]
        assert st["trace_ms"] > 0 and st["total_ms"] >= st["trace_ms"]
        done += 1
    assert done >= 20
    for r in ctxs.values():
        r.close()


# ---------------------------------------------------------------- hard scenes ----

@pytest.mark.parametrize("variant", ["plain", "force_hasw", "inline", "indexed", "global"])
@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_hard_scenes_as_rays(oracle_lib, sc, variant):
    """all 42 hard scenes: every pixel's ray against the oracle's pre-blur frame, colour, depth and counters, carrying the
    depth of a first frame into a second (rays that run out of steps keep it); global: the sphere lists in device memory
    (tables.h PWN_LF_GLOBAL), forced on these small scenes"""
    import pwnfps_amd
    env = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "inline": {"PWN_SPHERE_LISTS": "inline"},
           "indexed": {"PWN_SPHERE_LISTS": "indexed"}, "global": {"PWN_SPHERE_LISTS": "global"}}[variant]
    O = HS.oracle(oracle_lib, sc)
    plane = HS.Plane(O, sc.w, sc.h)
    with _env(**env):
        r = pwnfps_amd.Renderer(8, 8)
    HS.load_renderer(r, sc)
    if variant == "global":
        assert r.sphere_tables()["form"] == 2, (sc.name, r.sphere_tables())
    r.set_counters(True)
    for k, (cam, sec) in enumerate(((sc.cam, sc.sec), (pwnfps_amd.mat4_roty(sc.cam, 0.4), sc.sec + 0.5))):
        rays, seeds, xy = pwnfps_amd.pixel_rays(sc.w, sc.h, cam, order="units" if k else "rows")
        zin = plane.z[xy[:, 1], xy[:, 0]]
        col, zout = r.trace_rays(rays, seeds, sec, depth=zin)
        want, wz, st = plane.frame(cam, sec, 0)
        got, gz = _plane(col, zout, xy, sc.w, sc.h)
        bad = got != want
        assert not bad.any(), (sc.name, variant, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert (_bits(gz) == _bits(wz)).all(), (sc.name, variant, k)
        assert HS.stats5(r.stats()) == HS.stats5(st), (sc.name, variant, k)
    r.close()


# ---------------------------------------------------------------- the oracle trick ----

TRICK_W = 8


def _trick(O, rec, seed_xy, zin, sec):
    """the oracle on ray (O, D) with pixel (x, y)'s seed of a TRICK_W-wide frame and entry depth zin: colour and depth"""
    x, y = seed_xy
    cam = np.zeros((4, 4), np.float32)
    cam[2] = rec[4:]
    cam[3] = rec[:4]
    zb = np.zeros((y + 1, TRICK_W), np.float32)
    zb[y, x] = zin
    sb, zb, st = O.trace_rows(TRICK_W, y + 1, y, y + 1, cam, sec=np.float32(sec), threads=1, zb=zb)
    return sb[y, x], zb[y, x]


def _ftz(a):
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < np.float32(1.17549435e-38), np.float32(0), a).astype(np.float32)


def _odd(rec):
    """rays whose direction normalises to non-finite lanes (no NaN component: those are NaN throughout, like the reference's)"""
    d = rec[:, 4:8].astype(np.float32)
    with np.errstate(all="ignore"):
        sq = _ftz(d * d)
        dot3 = _ftz(_ftz(sq[:, 0] + sq[:, 2]) + sq[:, 1])
        dot4 = _ftz(_ftz(sq[:, 0] + sq[:, 2]) + _ftz(sq[:, 1] + sq[:, 3]))
    bad = (dot3 == 0) | (dot4 == 0) | np.isinf(dot3) | np.isinf(dot4) | np.isinf(d[:, :3]).any(1)
    return bad & ~np.isnan(d).any(1)


def _frame_kernel(level, key, rec, sxy, zin, sec, which, force_hasw):
    """{i: (colour, depth)} of the trick camera of ray i through the frame kernel (pwn_trace_rows_device, row y of a TRICK_W-wide
    frame), for i in which; force_hasw: the 4-lane variants"""
    import torch
    r = _renderer(level, key, TRICK_W, 3000, env={"PWN_DBG_FORCE_HASW": "1"} if force_hasw else None)
    sb = torch.zeros((3000, TRICK_W), dtype=torch.int32, device="cuda")
    zb = torch.zeros((3000, TRICK_W), dtype=torch.float32, device="cuda")
    out = {}
    for i in which:
        x, y = (int(v) for v in sxy[i])
        cam = np.zeros((4, 4), np.float32)
        cam[2] = rec[i, 4:]
        cam[3] = rec[i, :4]
        zb[y, x] = float(zin[i])
        torch.cuda.synchronize()
        r.trace_rows_device(cam, sec, y, y + 1, sb.data_ptr(), zb.data_ptr())
        torch.cuda.synchronize()
        out[i] = (np.uint32(sb[y, x].item() & 0xffffffff), np.float32(zb[y, x].item()))
    r.close()
    return out


def _hostile_rays(rng, n, w_lanes):
    """origins and directions of every kind: ordinary ones inside the grid, far outside it, non-finite, huge, zero"""
    o = np.zeros((n, 4), np.float32)
    d = np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform(0, 64, (n, 3))
    o[:, 1] = rng.uniform(0.05, 0.95, n)
    o[:, 3] = 1.0
    d[:, :3] = rng.normal(size=(n, 3))
    specials = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 3e4, -2e5, 1e-30, 65.0, -1.0], np.float32)
    for i in range(n):
        kind = i % 8
        if kind == 1:
            d[i, rng.integers(3)] = specials[rng.integers(len(specials))]
        elif kind == 2:
            o[i, rng.integers(3)] = specials[rng.integers(len(specials))]
        elif kind == 3:
            d[i, :3] = 0.0
        elif kind == 4:
            o[i, :3] = rng.uniform(-1e6, 1e6, 3)
        elif kind == 5:
            d[i, :3] = specials[rng.integers(len(specials), size=3)]
            o[i, :3] = specials[rng.integers(len(specials), size=3)]
        elif kind == 6:
            d[i, :3] *= np.float32(1e-20)
    if w_lanes:
        o[::3, 3] = rng.uniform(-2, 2, len(o[::3]))
        d[1::3, 3] = rng.uniform(-1, 1, len(d[1::3]))
    rec = np.concatenate([o, d], 1).astype(np.float32)
    rec[rec == 0] = 0.0                      # (the trick turns a -0 component of D into +0: the batch gets +0 too)
    return rec


@pytest.mark.parametrize("level,key", [("pwnfps_level", "t0"), ("synth256", "synth256"), ("synth64", "synth64")])
@pytest.mark.parametrize("w_lanes", [False, True], ids=["w01", "w_lanes"])
def test_random_and_hostile_rays_against_the_oracle(oracle_lib, level, key, w_lanes):
    """random and hostile (O, D) with pixel seeds and random entry depths, host form and device form: against the oracle trick.
    Without PWN_RAYS_HAS_W the device form takes the w lanes as 1 and 0 -- the oracle on those rays."""
    import torch
    rng = np.random.default_rng(9100 + 10 * len(level) + w_lanes)
    n = 400
    rec = _hostile_rays(rng, n, w_lanes)
    sxy = np.stack([rng.integers(0, TRICK_W, n), rng.integers(0, 3000, n)], 1)
    seeds = np.array([oracle_lib.lib().pwno_pixel_seed(int(x), int(y), TRICK_W) for x, y in sxy], np.uint32)
    zin = rng.uniform(-5, 5, n).astype(np.float32)
    sec = 3.25
    O = oracle_lib.Oracle()
    O.load_level(level_path(level))
    O.set_spheres(load_spheres(key))
    plain = rec.copy()
    plain[:, 3], plain[:, 7] = 1.0, 0.0
    want = [_trick(O, rec[i], sxy[i], zin[i], sec) for i in range(n)]
    want01 = want if not w_lanes else [_trick(O, plain[i], sxy[i], zin[i], sec) for i in range(n)]
    r = _renderer(level, key)
    col, z = r.trace_rays(rec, seeds, sec, depth=zin)
    # A direction whose normalised form is not finite -- an infinite component, or a squared length that flushes to 0 or
    # overflows -- gets NaN or infinite lanes (rsqrt of 0 or inf): there the trace kernel, the frame kernel's too, is known to
    # leave the reference.  Such rays are held to the frame kernel on the same camera and kernel variant instead:
    # the ray mode adds no divergence of its own.
    odd = _odd(rec)
    frame = _frame_kernel(level, key, rec, sxy, zin, sec, np.flatnonzero(odd), force_hasw=w_lanes)
    exp_w = [frame[i] if odd[i] else want[i] for i in range(n)]
    for i in range(n):
        assert col[i] == exp_w[i][0] and _bits(z[i]) == _bits(exp_w[i][1]), (level, w_lanes, i, rec[i].tolist())
    dev = torch.device("cuda", 0)
    for has_w in (False, True):
        t_rec = torch.from_numpy(rec).to(dev)
        t_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        t_col = torch.zeros(n, dtype=torch.int32, device=dev)
        t_z = torch.from_numpy(zin).to(dev)
        r.trace_rays_device(t_rec, t_col, t_z, seeds=t_seeds, sec_current=sec, has_w=has_w)
        torch.cuda.synchronize()
        dcol = t_col.cpu().numpy().view(np.uint32)
        dz = t_z.cpu().numpy()
        if has_w:
            frame4 = frame if w_lanes else _frame_kernel(level, key, rec, sxy, zin, sec, np.flatnonzero(odd), force_hasw=True)
            exp = [frame4[i] if odd[i] else want[i] for i in range(n)]
        else:
            frame3 = _frame_kernel(level, key, plain, sxy, zin, sec, np.flatnonzero(odd), force_hasw=False)
            exp = [frame3[i] if odd[i] else want01[i] for i in range(n)]
        for i in range(n):
            assert dcol[i] == exp[i][0] and _bits(dz[i]) == _bits(exp[i][1]), (level, w_lanes, has_w, i, rec[i].tolist())
    r.close()


def test_exhausted_rays_keep_their_entry_depth(oracle_lib, cases):
    """synth256 cam0: rays that run out of steps keep the sentinel depth they came in with"""
    import pwnfps_amd
    c = next(x for x in cases if x["name"] == "synth256_cam0_480x272")
    w, h = c["w"], c["h"]
    cam = np.array(c["cam"], np.float32)
    rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, cam)
    sentinel = np.float32(-12345.5)
    r = _renderer("synth256", "synth256")
    r.set_counters(True)
    col, z = r.trace_rays(rays, seeds, c["sec"], depth=np.full(len(rays), sentinel, np.float32))
    assert r.stats()["exhausted"] == c["exhausted"] == 1
    O = oracle_lib.Oracle()
    O.load_level(level_path("synth256"))
    O.set_spheres(load_spheres("synth256"))
    sb, zb, st = O.trace_rows(w, h, 0, h, cam, sec=np.float32(c["sec"]), zb=np.full((h, w), sentinel, np.float32))
    assert st.exhausted == 1
    assert (col == sb.ravel()).all() and (_bits(z) == _bits(zb.ravel())).all()
    assert (z == sentinel).sum() >= 1
    r.close()


# ---------------------------------------------------------------- batch sizes and the device form ----

def test_batch_sizes_host_and_device(oracle_lib, cases):
    """n = 0, 1, 63, 64, 65, 1000 and 2^20 through both forms: the first n rays of a golden 1080p frame (pinned by its hash);
    the device form on torch tensors made on a non-default stream that the call then runs on"""
    import torch
    import pwnfps_amd
    c = next(x for x in cases if x["name"] == "level_spawn_1920x1080")
    rays, seeds, xy = pwnfps_amd.pixel_rays(c["w"], c["h"], np.array(c["cam"], np.float32), order="units")
    r = _renderer("pwnfps_level", "t0")
    col, z = r.trace_rays(rays, seeds, c["sec"])
    pre, zz = _plane(col, z, xy, c["w"], c["h"])
    assert oracle_lib.fnv64(pre) == c["pre"] and oracle_lib.fnv64(zz) == c["z"]
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    for n in (0, 1, 63, 64, 65, 1000, 1 << 20):
        a, za = r.trace_rays(rays[:n], seeds[:n], c["sec"])
        assert a.shape == (n,) and (a == col[:n]).all() and (_bits(za) == _bits(z[:n])).all(), n
        # (col only, depth only, no seeds)
        only_col = np.empty(n, np.uint32)
        assert r._chk(pwnfps_amd._lib.lib.pwn_trace_rays(r._ctx, n, rays[:n].ctypes.data, seeds[:n].ctypes.data, c["sec"],
                                                          only_col.ctypes.data, None), "t") == 0
        assert (only_col == col[:n]).all(), n
        with torch.cuda.stream(s):
            t_rec = torch.from_numpy(rays[:n].copy()).to(dev, non_blocking=True)
            t_seeds = torch.from_numpy(seeds[:n].view(np.int32).copy()).to(dev, non_blocking=True)
            t_col = torch.full((n,), -1, dtype=torch.int32, device=dev)
            t_z = torch.zeros(n, dtype=torch.float32, device=dev)
            r.trace_rays_device(t_rec, t_col, t_z, seeds=t_seeds, sec_current=c["sec"])
            got_col = t_col.cpu().numpy().view(np.uint32)
            got_z = t_z.cpu().numpy()
        s.synchronize()
        assert (got_col == col[:n]).all() and (_bits(got_z) == _bits(z[:n])).all(), n
    # seeds NULL: every seed 0 (the trick, seed of pixel (0, 0))
    a0, z0 = r.trace_rays(rays[:64], None, c["sec"])
    a1, z1 = r.trace_rays(rays[:64], np.zeros(64, np.uint32), c["sec"])
    assert (a0 == a1).all() and (_bits(z0) == _bits(z1)).all()
    r.close()


# ---------------------------------------------------------------- no disturbance ----

def _sequence(r, cams, rays_between, rays=None, seeds=None):
    """blocking frames (depth persistence on synth256), views, frames in flight and upscale; ray calls in between when asked"""
    import torch
    out = []

    def rays_call():
        if rays_between:
            r.trace_rays(rays, seeds, 0.5, depth=np.full(len(rays), 7.0, np.float32))
            t = torch.from_numpy(rays).cuda()
            r.trace_rays_device(t, torch.zeros(len(rays), dtype=torch.int32, device="cuda"),
                                torch.zeros(len(rays), device="cuda"), sec_current=0.5)
            torch.cuda.synchronize()

    rays_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    rays_call()
    out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32)))
    rays_call()
    out.append(r.screen_upscale(None, 2))
    out += list(r.trace_screen_centred(cams[0], 0.0))          # rays of cams[0] run out of steps: depth of cams[1] stays
    rays_call()
    out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32)))
    r.frames_config(2, sbuf=True, zbuf=True)
    r.submit_frame(cams[3], 0.25, 0)
    r.submit_frame(cams[2], 0.5, 1)
    rays_call()
    for i in range(2):
        fr = r.wait_frame(i)
        out += [fr["sbuf"].copy(), fr["zbuf"].copy()]
    r.frames_config(0)
    rays_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    return out


def test_other_calls_are_not_disturbed(oracle_lib):
    """blocking frames, frames in flight and batches of views, interleaved with ray calls, stay bit-identical to the same
    sequence without them, depth persistence and pwn_screen_upscale(NULL, ...) included"""
    import pwnfps_amd
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    w, h = 480, 272
    rays, seeds, _ = pwnfps_amd.pixel_rays(w, h, cams[0])
    for blur in (0, 1):
        res = []
        for between in (False, True):
            r = _renderer("synth256", "synth256", w, h)
            r.set_blur_passes(blur)
            res.append(_sequence(r, cams, between, rays, seeds))
            r.close()
        assert len(res[0]) == len(res[1])
        for i, (a, b) in enumerate(zip(*res)):
            assert a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(), (blur, i)


# ---------------------------------------------------------------- moving objects ----

def test_moving_sphere_between_ray_calls(oracle_lib):
    """pwn_obj_set_sphere + pwn_prepare_render between ray calls: each call sees the current object table"""
    import pwnfps_amd
    r = _renderer("pwnfps_level", "none")
    O = oracle_lib.Oracle()
    O.load_level(level_path("pwnfps_level"))
    _, _, spawn = r.get_level()
    w, h = 160, 120
    cam = pwnfps_amd.spawn_camera(spawn)                    # looking along +z from the spawn cell's centre
    rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, cam, order="units")
    obj = r.obj_new()
    hits = []
    for k in range(4):
        r.obj_set(obj, "sphere", 0.08, 0.4, spawn[0] + 0.5 + 0.04 * k, 0.5, spawn[1] + 0.85, 0.2, 0.6, 0.9)
        r.level_prepare_render()
        col, z = r.trace_rays(rays, seeds, 1.0 + k)
        O.set_spheres(r.get_objects())
        sb, zb, _ = O.trace_rows(w, h, 0, h, cam, sec=np.float32(1.0 + k))
        got, gz = _plane(col, z, xy, w, h)
        assert (got == sb).all() and (_bits(gz) == _bits(zb)).all(), k
        hits.append(got)
    assert not (hits[0] == hits[3]).all()           # the sphere moved in view
    r.close()


# ---------------------------------------------------------------- refusals ----

def test_refusals(oracle_lib):
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    rays = np.zeros((4, 8), np.float32)
    rays[:, 3] = 1.0
    rays[:, 4] = 1.0
    col = np.zeros(4, np.uint32)
    z = np.zeros(4, np.float32)
    # before a level
    nl = _renderer()
    assert L.pwn_trace_rays(nl._ctx, 4, rays.ctypes.data, None, 0.0, col.ctypes.data, z.ctypes.data) == PWN_ENOLEVEL
    nl.close()
    r = _renderer("pwnfps_level", "t0")
    ctx = r._ctx
    assert L.pwn_trace_rays(ctx, 0, None, None, 0.0, col.ctypes.data, None) == 0
    assert L.pwn_trace_rays(ctx, -1, rays.ctypes.data, None, 0.0, col.ctypes.data, None) == PWN_EINVAL
    assert L.pwn_trace_rays(ctx, 4, None, None, 0.0, col.ctypes.data, None) == PWN_EINVAL
    assert L.pwn_trace_rays(ctx, 4, rays.ctypes.data, None, 0.0, None, None) == PWN_EINVAL
    assert L.pwn_trace_rays(ctx, (1 << 28) + 1, rays.ctypes.data, None, 0.0, col.ctypes.data, None) == PWN_EINVAL
    import torch
    t = torch.zeros((5, 8), dtype=torch.float32, device="cuda")
    tc = torch.zeros(5, dtype=torch.int32, device="cuda")
    tz = torch.zeros(5, device="cuda")
    p = t.data_ptr()
    assert L.pwn_trace_rays_device(ctx, 4, p, None, 0.0, 2, tc.data_ptr(), tz.data_ptr(), None) == PWN_EINVAL     # unknown flag
    assert L.pwn_trace_rays_device(ctx, 4, p + 4, None, 0.0, 0, tc.data_ptr(), tz.data_ptr(), None) == PWN_EINVAL  # misaligned
    assert L.pwn_trace_rays_device(ctx, 4, p, tc.data_ptr() + 2, 0.0, 0, tc.data_ptr(), tz.data_ptr(), None) == PWN_EINVAL
    assert L.pwn_trace_rays_device(ctx, 4, p, None, 0.0, 0, tc.data_ptr() + 1, tz.data_ptr(), None) == PWN_EINVAL
    assert L.pwn_trace_rays_device(ctx, 4, p, None, 0.0, 0, None, tz.data_ptr(), None) == PWN_EINVAL
    assert L.pwn_trace_rays_device(ctx, 0, None, None, 0.0, 0, None, None, None) == 0
    with pytest.raises(ValueError):
        r.trace_rays_device(t[:, :7].contiguous(), tc, tz)
    with pytest.raises(ValueError):
        r.trace_rays_device(t, tc.float(), tz)
    with pytest.raises(ValueError):
        r.trace_rays_device(t.view(-1)[1:33].view(4, 8), tc[:4], tz[:4])      # 4 B past an aligned start
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(64, 64, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert L.pwn_trace_rays(g._ctx, 4, rays.ctypes.data, None, 0.0, col.ctypes.data, z.ctypes.data) == PWN_ENOTSUP
    assert L.pwn_trace_rays_device(g._ctx, 4, p, None, 0.0, 0, tc.data_ptr(), tz.data_ptr(), None) == PWN_ENOTSUP
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert L.pwn_trace_rays(ctx, 4, rays.ctypes.data, None, 0.0, col.ctypes.data, z.ctypes.data) == PWN_EBUSY
    assert L.pwn_trace_rays_device(ctx, 4, p, None, 0.0, 0, tc.data_ptr(), tz.data_ptr(), None) == PWN_EBUSY
    r.tiled_shutdown()
    a, za = r.trace_rays(rays, None, 0.0)
    assert a.shape == (4,)
    r.close()
