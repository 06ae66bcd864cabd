"""pwn_trace_hits: first-hit records of caller-supplied rays.  A record is the state of trace_ray's primary walk (trace.h:186) at
its return; the reference is the oracle's event chain of the same ray, read by tests/hit_chain.py (pinned on the oracle alone in
tests/test_hits_oracle.py), and the oracle's depth plane for `kind` and `dist` of whole frames.  Every check runs the kernel
variants a context can pick: 3-lane and 4-lane (PWN_DBG_FORCE_HASW), and the sphere lists inline, indexed or in device memory
(PWN_SPHERE_LISTS; global: tables.h PWN_LF_GLOBAL, forced on scenes that would fit on chip).
"""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
import hit_chain as HC
from conftest import GOLD, level_path, load_spheres
from oracle import SPHERE_DTYPE

pytestmark = pytest.mark.gpu

SCENES = HS.scenes(SPHERE_DTYPE)
IDS = [s.name for s in SCENES]
PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
VARIANTS = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "inline": {"PWN_SPHERE_LISTS": "inline"},
            "indexed": {"PWN_SPHERE_LISTS": "indexed"}, "global": {"PWN_SPHERE_LISTS": "global"}}
ON_CHIP = ("plain", "force_hasw", "inline", "indexed")
SENTINEL = np.uint32(0x7fc12345)          # a NaN pattern no computation makes


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


def _renderer(variant="plain", w=8, h=8):
    import pwnfps_amd
    with _env(**VARIANTS[variant]):
        r = pwnfps_amd.Renderer(w, h)
    r.set_blur_passes(0)
    return r


def _level_renderer(variant="plain", level="pwnfps_level", spheres="t0", w=8, h=8):
    r = _renderer(variant, w, h)
    r.level_load(level_path(level))
    r.set_objects(HC.mark_spheres(load_spheres(spheres)))
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _form_is_forced(r, variant, what):
    """global: the context really holds its tables in device memory (a misspelt variable would leave them on chip)"""
    if variant == "global":
        assert r.sphere_tables()["form"] == 2, (what, r.sphere_tables())


def _report(got, want, bad, rays=None):
    return [(int(i), got[i].tolist(), want[i].tolist(), None if rays is None else rays[i].tolist()) for i in bad[:3]]


# ---------------------------------------------------------------- 1. depth on the hard scenes ----

_depth_planes = {}


def _depth_plane(oracle_lib, sc):
    """the oracle's depth plane of the scene's frame, pre-filled with the sentinel: computed once, shared by the variants"""
    if sc.name not in _depth_planes:
        O = HS.oracle(oracle_lib, sc)
        zb = np.full((sc.h, sc.w), SENTINEL, np.uint32).view(np.float32)
        _, zb, _ = O.trace_rows(sc.w, sc.h, 0, sc.h, sc.cam, sec=np.float32(sc.sec), zb=zb)
        _depth_planes[sc.name] = _bits(zb).copy()
    return _depth_planes[sc.name]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_hard_scene_depths(oracle_lib, sc, variant):
    """every pixel of all 42 hard scenes: kind == 0 exactly where the oracle's depth keeps its sentinel, elsewhere dist is its bits"""
    import pwnfps_amd
    zb = _depth_plane(oracle_lib, sc)
    r = _renderer(variant)
    HS.load_renderer(r, sc)
    _form_is_forced(r, variant, sc.name)
    rays, _, xy = pwnfps_amd.pixel_rays(sc.w, sc.h, sc.cam)
    hits = r.trace_hits(rays)
    r.close()
    want = zb[xy[:, 1], xy[:, 0]]
    none = hits["kind"] == 0
    assert (none == (want == SENTINEL)).all(), (sc.name, variant, int((none != (want == SENTINEL)).sum()))
    bad = np.flatnonzero(~none & (_bits(hits["dist"]) != want))
    assert len(bad) == 0, (sc.name, variant, len(bad), xy[bad[:4]].tolist())
    assert np.isin(hits["kind"], (0, 1, 2)).all()


# ---------------------------------------------------------------- 2. every field against the reader ----

_record_refs = {}


def _record_ref(oracle_lib, sc):
    """(the pixels, their rays, what hit_chain.Reader reads off the oracle with marked spheres): computed once per scene, shared"""
    import pwnfps_amd
    if sc.name not in _record_refs:
        O = oracle_lib.Oracle()
        HS.load_oracle(O, sc._replace(spheres=HC.mark_spheres(sc.spheres)))
        n = sc.w * sc.h
        if n <= 516:
            xy = HC.all_pixels(sc.w, sc.h)
        else:
            rng = np.random.default_rng(1000 + len(sc.name))
            pick = rng.choice(n, 512, replace=False)
            xy = np.stack([pick % sc.w, pick // sc.w], 1).astype(np.int32)
            xy = np.concatenate([xy, np.array([[0, 0], [sc.w - 1, 0], [0, sc.h - 1], [sc.w - 1, sc.h - 1]], np.int32)])
        ref = HC.Reader(O).pixels(sc.w, sc.h, sc.cam, xy)
        rays, _, _ = pwnfps_amd.pixel_rays(sc.w, sc.h, sc.cam, xy)
        _record_refs[sc.name] = (xy, rays, ref)
    return _record_refs[sc.name]


# (the case without a suffix is the one this test has always had: the contexts whose tables lie on chip)
RECORD_CASES = [pytest.param(sc, lists, id=sc.name if lists == "plain" else sc.name + "-" + lists)
                for sc in SCENES for lists in ("plain", "global")]


@pytest.mark.parametrize("sc,lists", RECORD_CASES)
def test_hard_scene_records(oracle_lib, sc, lists):
    """512 seeded pixels and the four corners of each hard scene (all pixels of a smaller one): every field of every record
    against hit_chain.Reader.  plain: the four variants of a context with the lists on chip; global: the lists in device
    memory (`object` then comes out of the device buffer's which[])"""
    marked = sc._replace(spheres=HC.mark_spheres(sc.spheres))
    xy, rays, ref = _record_ref(oracle_lib, sc)
    for variant in (ON_CHIP if lists == "plain" else ("global",)):
        r = _renderer(variant)
        HS.load_renderer(r, marked)
        _form_is_forced(r, variant, sc.name)
        hits = r.trace_hits(rays)
        r.close()
        bad = HC.mismatches(hits, ref.want, ref.cmp_dy)
        assert len(bad) == 0, (sc.name, variant, len(bad), _report(hits, ref.want, bad, xy))


# ---------------------------------------------------------------- 3. the level.txt frames ----

def test_level_frames_records_and_counters(oracle_lib):
    """level.txt with spheres_t0, 32 x 24 from the spawn cell's centre at yaw 0, 0.8 and 5.6: every pixel, every field, `object`
    the index read from the reflectivity; the counters of the primary segments"""
    import pwnfps_amd
    O, sph, cams, refs = HC.level_frames(oracle_lib)
    w, h = HC.LEVEL_W, HC.LEVEL_H
    tests = {}
    for variant in VARIANTS:
        r = _level_renderer(variant)
        r.set_counters(True)
        for yaw, cam, ref in zip(HC.LEVEL_YAWS, cams, refs):
            rays, _, xy = pwnfps_amd.pixel_rays(w, h, cam)
            assert (xy == HC.all_pixels(w, h)).all()
            hits = r.trace_hits(rays)
            st = r.stats()
            bad = HC.mismatches(hits, ref.want, ref.cmp_dy)
            assert len(bad) == 0, (variant, yaw, len(bad), _report(hits, ref.want, bad, xy))
            assert st["rays"] == w * h
            assert st["steps"] == int(ref.steps.sum()), (variant, yaw)
            assert st["portals"] == int(ref.want["portals"].sum()), (variant, yaw)
            assert st["exhausted"] == int((ref.want["kind"] == HC.NONE).sum()), (variant, yaw)
            assert st["trace_ms"] > 0 and st["total_ms"] >= st["trace_ms"]
            tests.setdefault(yaw, []).append(st["sphere_tests"])
        r.close()
    for yaw, v in tests.items():
        # (the oracle counts sphere tests per frame, not per segment: the four variants against one another)
        assert len(set(v)) == 1 and v[0] > 0, (yaw, v)


# ---------------------------------------------------------------- 4. the loop corridor ----

CORRIDOR = ".........\n.A;;*;;A.\n.........\n"
CORRIDOR_DIRS = [(1, 0, 0), (-1, 0, 0), (1, 1e-5, 0), (1, -2e-4, 0), (-1, 3e-4, 1e-4), (1, 0, 2e-4), (1, 1e-3, 0), (1, 0.01, 0),
                 (0, 0, 1), (0.3, 0.2, 1)]


def test_loop_corridor(oracle_lib):
    """a corridor closed on itself by a portal pair: rays that run out of steps after hundreds of crossings, rays that reach the
    ceiling after 100 and after 10, rays that leave sideways"""
    O = oracle_lib.Oracle()
    O.load_level_text(CORRIDOR)
    O.set_spheres(np.zeros(0, SPHERE_DTYPE))
    starts = [(2.25, 0.5, 1.5), (4.5, 0.5, 1.25), (6.75, 0.5, 1.5), (3.5, 0.5, 1.75), (5.125, 0.5, 1.5)]
    rec = np.zeros((len(starts) * len(CORRIDOR_DIRS), 8), np.float32)
    rec[:, 3] = 1.0
    for i, s in enumerate(starts):
        for j, d in enumerate(CORRIDOR_DIRS):
            rec[i * len(CORRIDOR_DIRS) + j, :3] = s
            rec[i * len(CORRIDOR_DIRS) + j, 4:7] = d
    ref = HC.Reader(O).rays(rec)
    assert (ref.want["kind"] == HC.NONE).any() and (ref.want["portals"] >= 100).any()
    for variant in VARIANTS:
        r = _renderer(variant)
        r.level_load_text(CORRIDOR)
        r.set_objects(np.zeros(0, SPHERE_DTYPE))
        r.set_counters(True)
        hits = r.trace_hits(rec)
        st = r.stats()
        r.close()
        bad = HC.mismatches(hits, ref.want, ref.cmp_dy)
        assert len(bad) == 0, (variant, len(bad), _report(hits, ref.want, bad, rec))
        none = ref.want["kind"] == HC.NONE
        assert st["exhausted"] == int(none.sum()) and st["steps"] == int(ref.steps.sum())
        assert (ref.steps[none] == 1000).all()


# ---------------------------------------------------------------- 5. hostile records ----

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("w_lanes", [False, True], ids=["w01", "w_lanes"])
def test_hostile_records(variant, w_lanes):
    """NaN, +-inf, 1e30, zero directions, origins at +-16384 and beyond: kind and dist are what pwn_trace_rays leaves in a
    sentinel-filled depth array for the same rays and variant.  global: the walk reads its sphere records from device memory at
    indices that come out of the packed tables alone (trace_walk.inc), so these rays end as cleanly as on the other four"""
    from test_gpu_rays import _hostile_rays
    rng = np.random.default_rng(5150 + w_lanes)
    n = 512
    rec = _hostile_rays(rng, n, w_lanes)
    far = np.array([16383.5, -16384.5, 16384.0, -16385.0, 16500.25, -40000.0, 2.0 ** 31, -2.0 ** 31, 3e9, -1e12], np.float32)
    for k, v in enumerate(far):
        rec[8 * k + 7, k % 3 if k % 3 != 1 else 0] = v
        rec[8 * k + 7 + 80, 2] = v
        rec[8 * k + 7 + 80, 0] = -v
    r = _level_renderer(variant)
    _form_is_forced(r, variant, w_lanes)
    zin = np.full(n, SENTINEL, np.uint32).view(np.float32)
    _, z = r.trace_rays(rec, None, 0.0, depth=zin)
    hits = r.trace_hits(rec)
    r.close()
    zb = _bits(z)
    none = hits["kind"] == 0
    assert (none == (zb == SENTINEL)).all(), (variant, w_lanes, np.flatnonzero(none != (zb == SENTINEL))[:4].tolist())
    bad = np.flatnonzero(~none & (_bits(hits["dist"]) != zb))
    assert len(bad) == 0, (variant, w_lanes, len(bad), rec[bad[:3]].tolist())
    assert np.isin(hits["kind"], (0, 1, 2)).all()
    sp = hits["kind"] == 2
    assert ((hits["object"][sp] >= 0) & (hits["object"][sp] < len(load_spheres("t0")))).all() and (hits["object"][~sp] == -1).all()


# ---------------------------------------------------------------- 6. batch sizes and both forms ----

def test_batch_sizes_host_and_device(oracle_lib):
    """n = 0, 1, 63, 64, 65, 4097 through both forms; the device form on a non-default stream with torch tensors, guard words
    behind d_hits untouched; the host form's buffers grow at 4097 and give the same records afterwards"""
    import torch
    import pwnfps_amd
    O, sph, cams, _ = HC.level_frames(oracle_lib)
    rays, _, xy = pwnfps_amd.pixel_rays(96, 48, cams[1], order="units")
    keep = ~(np.signbit(rays[:, 4:]) & (rays[:, 4:] == 0)).any(1)       # (the trick gives +0 where the frame's ray has -0)
    rays = np.ascontiguousarray(rays[keep][:4097])
    assert len(rays) == 4097
    ref = HC.Reader(O).rays(rays)
    r = _level_renderer()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    guard = 8
    for n in (0, 1, 63, 64, 65, 4097, 65, 1):
        hits = r.trace_hits(rays[:n])
        assert hits.shape == (n,) and hits.dtype == pwnfps_amd.HIT_DTYPE
        bad = HC.mismatches(hits, ref.want[:n], ref.cmp_dy[:n])
        assert len(bad) == 0, (n, "host", _report(hits, ref.want, bad, rays))
        with torch.cuda.stream(s):
            t_rec = torch.from_numpy(rays[:n].copy()).to(dev, non_blocking=True)
            t_hits = torch.full((n + guard, 12), 0x5a5a5a5a, dtype=torch.int32, device=dev)
            r.trace_hits_device(t_rec, t_hits[:n])
            got = t_hits.cpu().numpy()
        s.synchronize()
        assert (got[n:] == 0x5a5a5a5a).all(), n
        dhits = np.ascontiguousarray(got[:n]).view(pwnfps_amd.HIT_DTYPE).reshape(n)
        bad = HC.mismatches(dhits, ref.want[:n], ref.cmp_dy[:n])
        assert len(bad) == 0, (n, "device", _report(dhits, ref.want, bad, rays))
    # the pair form, and the 4-lane variants told by the flag: the same records for rays with w lanes 1 and 0
    a = r.trace_hits((rays[:65, :3], rays[:65, 4:7]))
    assert len(HC.mismatches(a, ref.want[:65], ref.cmp_dy[:65])) == 0
    t_rec = torch.from_numpy(rays[:65].copy()).to(dev)
    t_hits = torch.zeros((65, 48), dtype=torch.uint8, device=dev)
    r.trace_hits_device(t_rec, t_hits, has_w=True)
    torch.cuda.synchronize()
    b = t_hits.cpu().numpy().view(pwnfps_amd.HIT_DTYPE).reshape(65)
    assert len(HC.mismatches(b, ref.want[:65], ref.cmp_dy[:65])) == 0
    r.close()


# ---------------------------------------------------------------- 7. left alone, refusals ----

def _sequence(r, cams, hits_between, rays):
    import torch
    out = []

    def hits_call():
        if hits_between:
            r.trace_hits(rays)
            t = torch.from_numpy(rays).cuda()
            r.trace_hits_device(t, torch.zeros((len(rays), 12), dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()

    hits_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    hits_call()
    out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32)))
    hits_call()
    out += list(r.trace_screen_centred(cams[0], 0.0))          # rays of cams[0] run out of steps: depth of cams[1] stays
    hits_call()
    out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32)))
    hits_call()
    out += list(r.trace_screen_centred(cams[1], 0.0))
    return out


def test_other_calls_are_not_disturbed():
    """blocking frames and batches of views interleaved with hit calls stay bit-identical to the same sequence without them,
    the depth that exhausted rays keep (the blocking call's plane, the view slots) included"""
    import pwnfps_amd
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    w, h = 240, 136
    rays, _, _ = pwnfps_amd.pixel_rays(w, h, cams[0])
    res = []
    for between in (False, True):
        r = _renderer("plain", w, h)
        r.level_load(level_path("synth256"))
        r.set_objects(load_spheres("synth256"))
        r.set_blur_passes(1)
        res.append(_sequence(r, cams, between, rays))
        r.close()
    assert len(res[0]) == len(res[1]) == 10
    for i, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(), i


def test_refusals():
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    rays = np.zeros((4, 8), np.float32)
    rays[:, 3] = 1.0
    rays[:, 4] = 1.0
    hits = np.zeros(4, pwnfps_amd.HIT_DTYPE)
    t = torch.zeros((5, 8), dtype=torch.float32, device="cuda")
    th = torch.zeros((5, 12), dtype=torch.int32, device="cuda")
    p, ph = t.data_ptr(), th.data_ptr()
    # before a level
    nl = _renderer()
    assert L.pwn_trace_hits(nl._ctx, 4, rays.ctypes.data, hits.ctypes.data) == PWN_ENOLEVEL
    assert L.pwn_trace_hits_device(nl._ctx, 4, p, 0, ph, None) == PWN_ENOLEVEL
    nl.close()
    r = _level_renderer()
    ctx = r._ctx
    assert L.pwn_trace_hits(ctx, 0, None, None) == 0
    assert L.pwn_trace_hits(ctx, -1, rays.ctypes.data, hits.ctypes.data) == PWN_EINVAL
    assert L.pwn_trace_hits(ctx, 4, None, hits.ctypes.data) == PWN_EINVAL
    assert L.pwn_trace_hits(ctx, 4, rays.ctypes.data, None) == PWN_EINVAL
    assert L.pwn_trace_hits(ctx, (1 << 28) + 1, rays.ctypes.data, hits.ctypes.data) == PWN_EINVAL
    assert L.pwn_trace_hits_device(ctx, 4, p, 2, ph, None) == PWN_EINVAL          # unknown flag
    assert L.pwn_trace_hits_device(ctx, 4, p + 4, 0, ph, None) == PWN_EINVAL      # misaligned rays
    assert L.pwn_trace_hits_device(ctx, 4, p, 0, ph + 4, None) == PWN_EINVAL      # misaligned hits: 4 B
    assert L.pwn_trace_hits_device(ctx, 4, p, 0, ph + 8, None) == PWN_EINVAL      # ... 8 B
    assert L.pwn_trace_hits_device(ctx, 4, p, 0, None, None) == PWN_EINVAL
    assert L.pwn_trace_hits_device(ctx, 4, None, 0, ph, None) == PWN_EINVAL
    assert L.pwn_trace_hits_device(ctx, 0, None, 0, None, None) == 0
    with pytest.raises(ValueError):
        r.trace_hits_device(t[:, :7].contiguous(), th)
    with pytest.raises(ValueError):
        r.trace_hits_device(t, th[:, :11].contiguous())
    with pytest.raises(ValueError):
        r.trace_hits_device(t[:4], th.view(-1)[1:49].view(4, 12))             # 4 B past an aligned start
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(64, 64, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert L.pwn_trace_hits(g._ctx, 4, rays.ctypes.data, hits.ctypes.data) == PWN_ENOTSUP
    assert L.pwn_trace_hits_device(g._ctx, 4, p, 0, ph, None) == PWN_ENOTSUP
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert L.pwn_trace_hits(ctx, 4, rays.ctypes.data, hits.ctypes.data) == PWN_EBUSY
    assert L.pwn_trace_hits_device(ctx, 4, p, 0, ph, None) == PWN_EBUSY
    r.tiled_shutdown()
    assert r.trace_hits(rays).shape == (4,)
    r.close()


# ---------------------------------------------------------------- 8. pwn_get_object_ids ----

def test_object_ids(oracle_lib):
    """`object` indexes the live table; pwn_get_object_ids maps it to the pwn_obj_new handle through new / set / free / new.
    Every handle's sphere carries the reflectivity (handle + 1) / 32, so the reader's `object` IS the handle of the sphere hit."""
    import pwnfps_amd
    r = _renderer()
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(np.zeros(0, SPHERE_DTYPE))
    assert r.object_ids().shape == (0,)
    O = oracle_lib.Oracle()
    O.load_level(level_path("pwnfps_level"))
    rd = HC.Reader(O)
    _, _, spawn = r.get_level()
    cam = pwnfps_amd.spawn_camera(spawn)                    # looking along +z from the spawn cell's centre
    w, h = 64, 48
    rays, _, xy = pwnfps_amd.pixel_rays(w, h, cam)
    where = {}

    def put(handle, dx, dy):
        where[handle] = (spawn[0] + 0.5 + dx, 0.5 + dy, spawn[1] + 0.9)
        r.obj_set(handle, "sphere", 0.05, (handle + 1) / 32.0, *where[handle], 0.2, 0.6, 0.9)

    def check(live_handles):
        r.level_prepare_render()
        ids = r.object_ids()
        assert ids.tolist() == live_handles
        objs = r.get_objects()
        assert len(objs) == len(ids)
        for k, hnd in enumerate(ids):
            assert (objs[k]["x"], objs[k]["y"], objs[k]["z"]) == tuple(np.float32(v) for v in where[hnd])
        hits = r.trace_hits(rays)
        O.set_spheres(objs)
        ref = rd.pixels(w, h, cam, xy)
        sp = ref.want["kind"] == HC.SPHERE
        assert (hits["kind"] == ref.want["kind"]).all()
        assert (ids[hits["object"][sp]] == ref.want["object"][sp]).all()           # the handle of the sphere the oracle hit
        assert set(ref.want["object"][sp].tolist()) == set(live_handles)             # every live sphere is hit
        # (and every other field: the reader's `object` turned from handle to index)
        want = ref.want.copy()
        want["object"][sp] = [live_handles.index(v) for v in ref.want["object"][sp]]
        assert len(HC.mismatches(hits, want, ref.cmp_dy)) == 0
        return ids

    a, b, c = r.obj_new(), r.obj_new(), r.obj_new()
    assert (a, b, c) == (0, 1, 2)
    put(a, -0.2, 0.0)
    put(b, 0.0, 0.15)
    put(c, 0.2, 0.0)
    check([0, 1, 2])
    r.obj_free(b)
    del where[b]
    check([0, 2])
    d = r.obj_new()
    assert d == b                       # (the freed slot is handed out again)
    e = r.obj_new()
    assert e == 3
    put(e, 0.0, -0.15)
    with pytest.raises(pwnfps_amd.PwnError):
        r.object_ids()                  # d was created but never set
    put(d, 0.0, 0.15)
    check([0, 1, 2, 3])
    r.obj_free(a)
    del where[a]
    check([1, 2, 3])                    # (no index is its own handle any more)
    put(a, -0.2, 0.0)                   # obj_set on a freed slot makes it a sphere again
    check([0, 1, 2, 3])
    # cap smaller than the count: the count comes back, the first entries are written
    from pwnfps_amd import _lib
    two = np.full(3, -7, np.int32)
    assert _lib.lib.pwn_get_object_ids(r._ctx, two.ctypes.data, 2) == 4 and two.tolist() == [0, 1, -7]
    # after pwn_upload_spheres: 0 .. n-1, in the array's order
    sph = load_spheres("t0")
    r.set_objects(sph)
    assert r.object_ids().tolist() == list(range(len(sph)))
    r.close()
