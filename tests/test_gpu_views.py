"""pwn_trace_views: a batch of views of one level in one call.  Every view is bit-identical, colour and depth, to the
blocking call with the same camera on a context whose earlier frames were that view slot's earlier cameras."""
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu


def _renderer(w, h, level=None, spheres=None, blur=1):
    import pwnfps_amd
    r = pwnfps_amd.Renderer(w, h)
    if level is not None:
        r.level_load(level_path(level))
        r.set_objects(load_spheres(spheres))
    r.set_blur_passes(blur)
    return r


def _stats5(st):
    return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])


GROUPS = [("pwnfps_level", "t0", 320, 240), ("synth64", "synth64", 480, 272), ("synth256", "synth256", 480, 272),
          ("synth64", "synth64", 1920, 1080)]


def _group(cases, level, spheres, w, h):
    return [c for c in cases if c["level"] == level and c["spheres"] == spheres and c["w"] == w and c["h"] == h]


@pytest.mark.parametrize("force_hasw", [False, True], ids=["plain", "force_hasw"])
def test_golden_cases_in_batches(oracle_lib, cases, monkeypatch, force_hasw):
    """Each group of golden cases that share a size, level and spheres as ONE batch: pre (blur 0), post (blur 1) and depth
    hashes per view, and the counters summed over the views"""
    if force_hasw:
        monkeypatch.setenv("PWN_DBG_FORCE_HASW", "1")       # (read when a context is created)
    for level, key, w, h in GROUPS:
        cs = _group(cases, level, key, w, h)
        assert len(cs) == (5 if level == "pwnfps_level" else 4), (level, w, h)
        if level == "pwnfps_level":
            assert sorted({c["sec"] for c in cs}) == [0.0, 1.5, 12.25, 1000.5]
        cams = np.array([c["cam"] for c in cs], np.float32)
        secs = np.array([c["sec"] for c in cs], np.float32)
        r = _renderer(w, h, level, key, blur=0)
        r.set_counters(True)
        pre, z = r.trace_views(cams, secs)
        st = r.stats()
        for i, c in enumerate(cs):
            assert oracle_lib.fnv64(pre[i]) == c["pre"], c["name"]
            assert oracle_lib.fnv64(z[i]) == c["z"], c["name"]       # (a fresh context: every slot's depth starts at 0 as the goldens')
        want = tuple(sum(c[k] for c in cs) for k in ("rays", "steps", "portals", "sphere_tests", "exhausted"))
        assert _stats5(st) == want, (level, w, h)
        r.set_counters(False)
        if any(c["exhausted"] > 0 for c in cs):
            r.close()
            r = _renderer(w, h, level, key)
        r.set_blur_passes(1)
        post, z = r.trace_views(cams.reshape(-1, 4, 4), secs)
        for i, c in enumerate(cs):
            assert oracle_lib.fnv64(post[i]) == c["post"], c["name"]
            assert oracle_lib.fnv64(z[i]) == c["z"], c["name"]
        r.close()


def _random_cams(rng, oracle_lib, level, n, w_frac=0.0):
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


def _check_against_single_calls(batch, cams, secs, w, h, level, key, blur):
    """view i of the batch (a fresh context's first batch) against the blocking call with cams[i]: on one second context
    where that view has no exhausted primary ray (depth then does not depend on the frames before), else on a fresh one"""
    sb, zb = batch
    single = _renderer(w, h, level, key, blur=blur)
    single.set_counters(True)
    for i in range(len(cams)):
        a, za = single.trace_screen_centred(cams[i], secs[i])
        if single.stats()["exhausted"] > 0:
            fresh = _renderer(w, h, level, key, blur=blur)
            a, za = fresh.trace_screen_centred(cams[i], secs[i])
            fresh.close()
        assert (sb[i] == a).all(), (level, w, h, blur, i, int((sb[i] != a).sum()))
        assert (zb[i].view(np.uint32) == za.view(np.uint32)).all(), (level, w, h, blur, i)
    single.close()


@pytest.mark.parametrize("level,key", [("pwnfps_level", "t0"), ("synth64", "synth64")])
def test_batch_equals_single_calls(oracle_lib, level, key):
    rng = np.random.default_rng(20261016 + len(level))
    for (w, h), n in (((332, 202), 1), ((332, 202), 3), ((320, 240), 64), ((332, 202), 300), ((100, 38), 64)):
        cams, secs = _random_cams(rng, oracle_lib, level, n)
        for blur in (0, 1, 2):
            r = _renderer(w, h, level, key, blur=blur)
            out = r.trace_views(cams, secs)
            assert out[0].shape == (n, h, w) and out[1].shape == (n, h, w)
            _check_against_single_calls(out, cams, secs, w, h, level, key, blur)
            r.close()


def test_cameras_with_w_components_in_a_batch(oracle_lib):
    """one camera with w components sends the whole batch through the general 4-lane variant: the plain cameras stay bit-exact"""
    rng = np.random.default_rng(77)
    w, h = 320, 240
    cams, secs = _random_cams(rng, oracle_lib, "pwnfps_level", 6)
    cams[2, :, 3] = (0.03, -0.01, 0.05, 0.8)
    for blur in (0, 1):
        r = _renderer(w, h, "pwnfps_level", "t0", blur=blur)
        out = r.trace_views(cams, secs)
        _check_against_single_calls(out, cams, secs, w, h, "pwnfps_level", "t0", blur)
        r.close()


def test_depth_persists_per_view_slot(oracle_lib):
    """slot k renders synth256 cams[1] and then cams[0] (rays of cams[0] run out of steps: the depth there stays cams[1]'s),
    while the other slots render other cameras; the second call has more views, which start from zero depth"""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    sph = load_spheres("synth256")
    O = oracle_lib.Oracle()
    O.load_level(level_path("synth256"))
    O.set_spheres(sph)
    w, h, k = 480, 272, 1
    sb, zb, _ = O.trace_rows(w, h, 0, h, cams[1])
    sb, zb, st = O.trace_rows(w, h, 0, h, cams[0], sb=sb, zb=zb)
    assert st.exhausted > 0
    fsb, fzb, _ = O.trace_rows(w, h, 0, h, cams[0])          # cams[0] on a slot that starts from zero depth
    assert (fzb.view(np.uint32) != zb.view(np.uint32)).any()
    for blur in (0, 1):
        r = _renderer(w, h, "synth256", "synth256", blur=blur)
        first = np.stack([cams[2], cams[1], cams[3]])
        r.trace_views(first, np.zeros(3, np.float32))
        second = np.stack([cams[3], cams[0], cams[2], cams[0], cams[1]])
        a, z = r.trace_views(second, np.zeros(5, np.float32))
        assert (z[k].view(np.uint32) == zb.view(np.uint32)).all()
        assert (a[k] == (O.blur_rows(0, h, sb, zb) if blur else sb)).all()
        assert (z[3].view(np.uint32) == fzb.view(np.uint32)).all()            # a new slot: zero depth behind it
        assert (a[3] == (O.blur_rows(0, h, fsb, fzb) if blur else fsb)).all()
        r.close()


def test_blocking_frame_state_is_left_alone(oracle_lib):
    """a batch between two blocking frames changes neither the blocking call's depth persistence nor what
    pwn_screen_upscale(NULL, ...) upscales"""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    sph = load_spheres("synth256")
    O = oracle_lib.Oracle()
    O.load_level(level_path("synth256"))
    O.set_spheres(sph)
    w, h = 480, 272
    r = _renderer(w, h, "synth256", "synth256", blur=0)
    s1, _ = r.trace_screen_centred(cams[1], 0.0)
    r.trace_views(np.stack([cams[2], cams[0], cams[3]]), np.zeros(3, np.float32))
    assert (r.screen_upscale(None, 2) == O.upscale(s1, 2)).all()
    a, z2 = r.trace_screen_centred(cams[0], 0.0)
    sb, zb, _ = O.trace_rows(w, h, 0, h, cams[1])
    sb, zb, st = O.trace_rows(w, h, 0, h, cams[0], sb=sb, zb=zb)
    assert st.exhausted > 0
    assert (a == sb).all() and (z2.view(np.uint32) == zb.view(np.uint32)).all()
    r.close()


def test_frames_in_flight_before_a_batch(oracle_lib, cases):
    c = next(x for x in cases if x["name"] == "level_pose1_320x240")
    w, h = c["w"], c["h"]
    rng = np.random.default_rng(5)
    fcams, fsecs = _random_cams(rng, oracle_lib, "pwnfps_level", 3)
    r = _renderer(w, h, "pwnfps_level", "t0")
    ref = _renderer(w, h, "pwnfps_level", "t0")
    want = [ref.trace_screen_centred(fcams[i], fsecs[i])[0].copy() for i in range(3)]
    ref.close()
    r.frames_config(3, sbuf=True)
    for i in range(3):
        r.submit_frame(fcams[i], fsecs[i], i)
    vc = np.array([c["cam"], fcams[0].ravel(), c["cam"]], np.float32)
    post, z = r.trace_views(vc, np.array([c["sec"], fsecs[0], c["sec"]], np.float32))
    assert oracle_lib.fnv64(post[0]) == c["post"] and oracle_lib.fnv64(post[2]) == c["post"]
    assert oracle_lib.fnv64(z[0]) == c["z"]
    assert (post[1] == want[0]).all()
    for i in range(3):
        fr = r.wait_frame(i)
        assert (fr["sbuf"] == want[i]).all(), i
    r.frames_config(0)
    r.close()


def _call(r, n, cams, secs, sbuf, zbuf=None):
    from pwnfps_amd._lib import lib
    p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    return lib.pwn_trace_views(r._ctx if r is not None else None, n, p(cams), p(secs), p(sbuf), p(zbuf))


def _ok_after(r, cams, secs, n=1):
    sb = np.zeros((n, r.h, r.w), np.uint32)
    assert _call(r, n, cams[:n], secs[:n], sb) == 0
    assert sb.any()


def test_errors(cases):
    import pwnfps_amd
    from pwnfps_amd import _lib
    c = next(x for x in cases if x["name"] == "level_spawn_320x240")
    w, h = c["w"], c["h"]
    cams = np.tile(np.array(c["cam"], np.float32), (4, 1))
    secs = np.zeros(4, np.float32)
    sb = np.zeros((4, h, w), np.uint32)
    assert _call(None, 1, cams, secs, sb) == _lib.PWN_EINVAL
    r = _renderer(w, h, "pwnfps_level", "t0")
    for args in ((1, None, secs, sb), (1, cams, None, sb), (1, cams, secs, None), (0, cams, secs, sb), (-3, cams, secs, sb),
                 (_lib.PWN_VIEWS_MAX + 1, cams, secs, sb)):
        assert _call(r, *args) == _lib.PWN_EINVAL, args[0]
        _ok_after(r, cams, secs)
    # more than 2^28 pixels in the batch
    big = _renderer(4096, 4096, "pwnfps_level", "t0", blur=0)
    assert _call(big, 17, cams, secs, sb) == _lib.PWN_EINVAL
    _ok_after(big, cams, secs)
    big.close()
    # w % 4 != 0 with blur on
    odd = _renderer(322, 200, "pwnfps_level", "t0", blur=1)
    assert _call(odd, 2, cams, secs, sb) == _lib.PWN_EINVAL
    odd.set_blur_passes(0)
    _ok_after(odd, cams, secs, 2)
    odd.close()
    # before a level
    nl = _renderer(w, h)
    assert _call(nl, 2, cams, secs, sb) == _lib.PWN_ENOLEVEL
    nl.level_load(level_path("pwnfps_level"))
    nl.set_objects(load_spheres("t0"))
    _ok_after(nl, cams, secs, 2)
    nl.close()
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(w, h, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    g.set_objects(load_spheres("t0"))
    assert _call(g, 2, cams, secs, sb) == _lib.PWN_ENOTSUP
    with pytest.raises(pwnfps_amd.PwnError):
        g.trace_views(cams[:2], secs[:2])
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert _call(r, 2, cams, secs, sb) == _lib.PWN_EBUSY
    r.tiled_shutdown()
    _ok_after(r, cams, secs, 4)
    r.close()
