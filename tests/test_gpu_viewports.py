"""pwn_trace_viewports: views of their own sizes composited into one frame in one call.  Rectangle i is bit-identical, colour
and depth, to the blocking call with cams[i] on a context of w_i x h_i; the depth plane persists by destination pixel; colour
outside the rectangles reads 0."""
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu

# Layout L1: context 336 x 208, full cover, every rectangle blur-legal -- 11 units wide off a 32-pixel tile, a width that is no
# multiple of 16, a rectangle across one 32-pixel tile with a height that is no multiple of 4, one smaller than a unit, a sliver
L1 = (336, 208, [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
                 (100, 138, 36, 70), (140, 100, 196, 108)])
# Layout L2: context 333 x 201, gaps, blur 0 only
L2 = (333, 201, [(1, 1, 1, 1), (3, 0, 17, 5), (21, 2, 33, 3), (55, 7, 277, 193), (0, 10, 50, 190)])


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _random_cams(rng, oracle_lib, level, n):
    """(the pattern of test_gpu_views._random_cams: a free cell, any heading, a pitch up to 1.2)"""
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
_SINGLE = {}


def _cams_for(oracle_lib, level, n, seed):
    """the cameras of a layout, the same for every test that uses it (neighbouring rectangles look at different places)"""
    k = (level, n, seed)
    if k not in _CAMS:
        _CAMS[k] = _random_cams(np.random.default_rng(seed), oracle_lib, level, n)
    return _CAMS[k]


def _single(level, key, w, h, blur, cam, sec):
    """(colour, depth, counters) of the blocking call on a FRESH context of w x h: computed once per process, never changed"""
    k = (level, key, w, h, blur, np.asarray(cam, np.float32).tobytes(), float(sec))
    if k not in _SINGLE:
        assert not os.environ.get("PWN_DBG_FORCE_HASW") and not os.environ.get("PWN_SPHERE_LISTS")
        r = _renderer(w, h, level, key, blur=blur)
        r.set_counters(True)
        sb, zb = r.trace_screen_centred(cam, sec)
        _SINGLE[k] = (sb.copy(), zb.copy(), _stats5(r.stats()))
        r.close()
    return _SINGLE[k]


def _check_rects(out, rects, cams, secs, level, key, blur, skip=()):
    """every rectangle of a fresh context's first viewport frame against the blocking call on a fresh context of its size"""
    sb, zb = out
    for i, (x, y, w, h) in enumerate(rects):
        if i in skip:
            continue
        a, za, _ = _single(level, key, w, h, blur, cams[i], secs[i])
        bad = int((sb[y:y + h, x:x + w] != a).sum())
        assert bad == 0, (level, blur, i, (x, y, w, h), bad)
        assert (_bits(zb[y:y + h, x:x + w]) == _bits(za)).all(), (level, blur, i, (x, y, w, h))


def _outside(W, H, rects):
    m = np.ones((H, W), bool)
    for x, y, w, h in rects:
        m[y:y + h, x:x + w] = False
    return m


@pytest.mark.parametrize("level,key", [("pwnfps_level", "t0"), ("synth64", "synth64")])
@pytest.mark.parametrize("layout,blur", [("L1", 0), ("L1", 1), ("L1", 2), ("L2", 0)])
def test_each_rectangle_equals_the_blocking_call_at_its_size(oracle_lib, level, key, layout, blur):
    W, H, rects = L1 if layout == "L1" else L2
    cams, secs = _cams_for(oracle_lib, level, len(rects), 20261018 + len(level) + len(rects))
    r = _renderer(W, H, level, key, blur=blur)
    sb, zb = r.trace_viewports(rects, cams, secs)
    r.close()
    assert sb.shape == (H, W) and zb.shape == (H, W) and sb.dtype == np.uint32 and zb.dtype == np.float32
    _check_rects((sb, zb), rects, cams, secs, level, key, blur)
    out = _outside(W, H, rects)
    assert out.any() == (layout == "L2")
    # outside the rectangles: colour 0, depth the plane as it stands (zero on a fresh context)
    assert (sb[out] == 0).all() and (_bits(zb)[out] == 0).all()


def test_goldens_of_two_sizes_in_one_call(oracle_lib, cases):
    names = ["level_spawn_320x200", "level_spawn_320x240", "level_pose1_320x240"]
    rects = [(0, 0, 320, 200), (320, 0, 320, 240), (0, 208, 320, 240)]
    cs = [next(c for c in cases if c["name"] == n) for n in names]
    assert all(c["level"] == "pwnfps_level" and c["spheres"] == "t0" and (c["w"], c["h"]) == r[2:] for c, r in zip(cs, rects))
    cams = np.array([c["cam"] for c in cs], np.float32)
    secs = np.array([c["sec"] for c in cs], np.float32)
    r = _renderer(640, 448, "pwnfps_level", "t0", blur=0)
    r.set_counters(True)
    pre, z = r.trace_viewports(rects, cams, secs)
    st = r.stats()
    for c, (x, y, w, h) in zip(cs, rects):
        assert oracle_lib.fnv64(np.ascontiguousarray(pre[y:y + h, x:x + w])) == c["pre"], c["name"]
        assert oracle_lib.fnv64(np.ascontiguousarray(z[y:y + h, x:x + w])) == c["z"], c["name"]
    assert _stats5(st) == tuple(sum(c[k] for c in cs) for k in ("rays", "steps", "portals", "sphere_tests", "exhausted"))
    r.set_counters(False)
    assert all(c["exhausted"] == 0 for c in cs)          # (depth then does not depend on the frame before)
    r.set_blur_passes(1)
    post, z = r.trace_viewports(rects, cams, secs)
    for c, (x, y, w, h) in zip(cs, rects):
        assert oracle_lib.fnv64(np.ascontiguousarray(post[y:y + h, x:x + w])) == c["post"], c["name"]
        assert oracle_lib.fnv64(np.ascontiguousarray(z[y:y + h, x:x + w])) == c["z"], c["name"]
    out = _outside(640, 448, rects)
    assert (post[out] == 0).all() and (pre[out] == 0).all()
    r.close()


@pytest.mark.parametrize("variant", ["force_hasw", "cam_w", "lists_indexed", "lists_inline", "lists_global", "counters"])
def test_every_variant_gives_the_plain_pixels(oracle_lib, monkeypatch, variant):
    """L1 at blur 1 through the 4-lane kernels, every form of the sphere lists and the counting kernels: the plain run's pixels
    (which test_each_rectangle... ties to the per-size contexts), and the counters summed over the per-size contexts'"""
    level, key, blur = "pwnfps_level", "t0", 1
    W, H, rects = L1
    cams, secs = _cams_for(oracle_lib, level, len(rects), 20261018 + len(level) + len(rects))
    singles = [_single(level, key, w, h, blur, cams[i], secs[i]) for i, (x, y, w, h) in enumerate(rects)]      # (before the environment changes)
    r = _renderer(W, H, level, key, blur=blur)
    plain = r.trace_viewports(rects, cams, secs)
    r.close()
    _check_rects(plain, rects, cams, secs, level, key, blur)
    cams = cams.copy()
    skip = ()
    if variant == "force_hasw":
        monkeypatch.setenv("PWN_DBG_FORCE_HASW", "1")           # (read when a context is created)
    elif variant.startswith("lists_"):
        monkeypatch.setenv("PWN_SPHERE_LISTS", variant[6:])     # (set before the context is created)
    elif variant == "cam_w":
        cams[3, :, 3] = (0.03, -0.01, 0.05, 0.8)                # the whole launch runs the 4-lane variant; the plain cameras stay exact
        skip = (3,)
    r = _renderer(W, H, level, key, blur=blur)
    if variant.startswith("lists_"):
        assert r.sphere_tables()["form"] == {"indexed": 0, "inline": 1, "global": 2}[variant[6:]]
    if variant == "counters":
        r.set_counters(True)
    sb, zb = r.trace_viewports(rects, cams, secs)
    st = r.stats()
    r.close()
    monkeypatch.delenv("PWN_DBG_FORCE_HASW", raising=False)
    monkeypatch.delenv("PWN_SPHERE_LISTS", raising=False)
    for i, (x, y, w, h) in enumerate(rects):
        if i in skip:
            a, za, _ = _single(level, key, w, h, blur, cams[i], secs[i])
            assert (sb[y:y + h, x:x + w] == a).all() and (_bits(zb[y:y + h, x:x + w]) == _bits(za)).all()
            continue
        assert (sb[y:y + h, x:x + w] == plain[0][y:y + h, x:x + w]).all(), (variant, i)
        assert (_bits(zb[y:y + h, x:x + w]) == _bits(plain[1][y:y + h, x:x + w])).all(), (variant, i)
    if variant == "counters":
        assert _stats5(st) == tuple(sum(s[2][k] for s in singles) for k in range(5))


def test_hostile_depths_in_touching_viewports():
    """a scene whose -inf depths send the blur's taps far outside (tests/hard_scenes.py, the non-finite lattice), twice in one
    frame side by side: no tap crosses the shared edge -- each half equals its own context's blurred frame"""
    import hard_scenes
    import pwnfps_amd
    from oracle import SPHERE_DTYPE
    sc = next(s for s in hard_scenes.scenes(SPHERE_DTYPE) if s.name == "nonfinite_lattice_77_698")
    assert sc.blur_ok and (sc.w, sc.h) == (128, 72)
    # (the second view: the scene's camera turned by half a radian about its y axis, a moment later)
    turned = sc.cam.copy()
    co, si = np.float32(np.cos(0.5)), np.float32(np.sin(0.5))
    turned[0], turned[2] = co * sc.cam[0] + si * sc.cam[2], co * sc.cam[2] - si * sc.cam[0]
    cams = np.stack([sc.cam, turned])
    secs = np.array([sc.sec, sc.sec + 1.0], np.float32)
    rects = [(0, 0, sc.w, sc.h), (sc.w, 0, sc.w, sc.h)]
    for blur in (1, 2):
        want = []
        for i in range(2):
            s = pwnfps_amd.Renderer(sc.w, sc.h)
            hard_scenes.load_renderer(s, sc)
            s.set_blur_passes(blur)
            want.append(tuple(a.copy() for a in s.trace_screen_centred(cams[i], secs[i])))
            s.close()
        assert (~np.isfinite(want[0][1])).any()
        r = pwnfps_amd.Renderer(2 * sc.w, sc.h)
        hard_scenes.load_renderer(r, sc)
        r.set_blur_passes(blur)
        sb, zb = r.trace_viewports(rects, cams, secs)
        r.close()
        for i, (x, y, w, h) in enumerate(rects):
            assert (sb[y:y + h, x:x + w] == want[i][0]).all(), (blur, i, int((sb[y:y + h, x:x + w] != want[i][0]).sum()))
            assert (_bits(zb[y:y + h, x:x + w]) == _bits(want[i][1])).all(), (blur, i)


_CHAIN = {}


def _synth256_chain(oracle_lib):
    """the oracle chain of test_gpu_views.test_depth_persists_per_view_slot, once: synth256 cams[1], then cams[0] over its depth
    (rays of cams[0] run out of steps: the depth there stays cams[1]'s), and cams[0] from zero depth"""
    if not _CHAIN:
        cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
        O = oracle_lib.Oracle()
        O.load_level(level_path("synth256"))
        O.set_spheres(load_spheres("synth256"))
        w, h = 480, 272
        sb1, zb1, _ = O.trace_rows(w, h, 0, h, cams[1])
        sb, zb, st = O.trace_rows(w, h, 0, h, cams[0], sb=sb1.copy(), zb=zb1.copy())
        assert st.exhausted > 0
        fsb, fzb, _ = O.trace_rows(w, h, 0, h, cams[0])
        assert (_bits(fzb) != _bits(zb)).any()
        _CHAIN.update(O=O, cams=cams, w=w, h=h, sb1=sb1, sb=sb, zb=zb, post=O.blur_rows(0, h, sb, zb))
    return _CHAIN


def test_depth_persists_by_destination_pixel(oracle_lib):
    ch = _synth256_chain(oracle_lib)
    cams, w, h = ch["cams"], ch["w"], ch["h"]
    W, H, rect = 512, 288, (16, 8, 480, 272)
    x, y = rect[:2]
    side = (496, 0, 16, 288)                    # fresh ground beside it, in the second call only
    for blur in (0, 1):
        r = _renderer(W, H, "synth256", "synth256", blur=blur)
        r.trace_viewports([rect], cams[1:2], [0.0])
        a, z = r.trace_viewports([side, rect], np.stack([cams[0], cams[0]]), [0.0, 0.0])
        r.close()
        assert (_bits(z[y:y + h, x:x + w]) == _bits(ch["zb"])).all(), blur
        assert (a[y:y + h, x:x + w] == (ch["post"] if blur else ch["sb"])).all(), blur
        # the new rectangle starts from zero depth: a fresh context of its size
        sa, sz, _ = _single("synth256", "synth256", side[2], side[3], blur, cams[0], 0.0)
        assert (a[:, 496:] == sa).all() and (_bits(z[:, 496:]) == _bits(sz)).all(), blur
        out = _outside(W, H, [side, rect])
        assert (a[out] == 0).all() and (_bits(z)[out] == 0).all()


def test_blocking_frames_and_view_slots_are_left_alone(oracle_lib):
    """a viewport call between two blocking frames and between two batches of views changes neither the blocking call's depth
    persistence, nor what pwn_screen_upscale(NULL, ...) upscales, nor the view slots' depth"""
    ch = _synth256_chain(oracle_lib)
    cams, w, h, O = ch["cams"], ch["w"], ch["h"], ch["O"]
    r = _renderer(w, h, "synth256", "synth256", blur=0)
    s1, _ = r.trace_screen_centred(cams[1], 0.0)
    assert (s1 == ch["sb1"]).all()
    r.trace_views(np.stack([cams[2], cams[1], cams[3]]), np.zeros(3, np.float32))
    vp, vz = r.trace_viewports([(0, 0, 240, 272), (240, 0, 240, 136)], np.stack([cams[0], cams[3]]), [0.0, 0.0])
    assert vp[:, :240].any() and (vp[136:, 240:] == 0).all()
    assert (r.screen_upscale(None, 2) == O.upscale(s1, 2)).all()
    a, z = r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32))
    assert (a[1] == ch["sb"]).all() and (_bits(z[1]) == _bits(ch["zb"])).all()
    a, z2 = r.trace_screen_centred(cams[0], 0.0)
    assert (a == ch["sb"]).all() and (_bits(z2) == _bits(ch["zb"])).all()
    r.close()


def test_frames_in_flight_before_a_viewport_call(oracle_lib, cases):
    c = next(x for x in cases if x["name"] == "level_pose1_320x240")
    w, h = c["w"], c["h"]
    fcams, fsecs = _random_cams(np.random.default_rng(5), oracle_lib, "pwnfps_level", 3)
    r = _renderer(w, h, "pwnfps_level", "t0")
    want = [_single("pwnfps_level", "t0", w, h, 1, fcams[i], fsecs[i])[0] for i in range(3)]
    r.frames_config(3, sbuf=True)
    for i in range(3):
        r.submit_frame(fcams[i], fsecs[i], i)
    post, z = r.trace_viewports([(0, 0, w, h)], np.array([c["cam"]], np.float32), [c["sec"]])
    assert oracle_lib.fnv64(post) == c["post"] and oracle_lib.fnv64(z) == c["z"]
    for i in range(3):
        fr = r.wait_frame(i)
        assert (fr["sbuf"] == want[i]).all(), i
    r.frames_config(0)
    r.close()


def _call(r, n, vp, cams, secs, sbuf, zbuf=None):
    from pwnfps_amd._lib import lib
    p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    return lib.pwn_trace_viewports(r._ctx if r is not None else None, n, p(vp), p(cams), p(secs), p(sbuf), p(zbuf))


def _ok_after(r, cams, secs):
    vp = np.array([(0, 0, r.w // 2 // 4 * 4, r.h), (r.w // 2 // 4 * 4, 0, 4, 1)], np.int32)
    sb = np.zeros((r.h, r.w), np.uint32)
    assert _call(r, 2, vp, cams, secs, sb) == 0
    assert sb[:, :vp[0, 2]].any()


def test_errors(cases):
    import pwnfps_amd
    from pwnfps_amd import _lib
    c = next(x for x in cases if x["name"] == "level_spawn_320x240")
    w, h = c["w"], c["h"]
    cams = np.tile(np.array(c["cam"], np.float32), (4, 1))
    secs = np.zeros(4, np.float32)
    sb = np.zeros((h, w), np.uint32)
    good = np.array([(0, 0, 160, 240), (160, 0, 160, 120), (160, 120, 160, 120)], np.int32)
    assert _call(None, 3, good, cams, secs, sb) == _lib.PWN_EINVAL
    r = _renderer(w, h, "pwnfps_level", "t0")
    many = np.zeros((_lib.PWN_VIEWS_MAX + 1, 4), np.int32)
    many[:, 0] = np.arange(len(many)) % 80 * 4
    many[:, 1] = np.arange(len(many)) // 80 * 4
    many[:, 2:] = 4
    mcams = np.tile(cams[:1], (len(many), 1))
    msecs = np.zeros(len(many), np.float32)

    def rects(*rs):
        return np.array(rs, np.int32)

    refused = [
        (3, None, cams, secs, sb), (3, good, None, secs, sb), (3, good, cams, None, sb), (3, good, cams, secs, None),
        (0, good, cams, secs, sb), (-3, good, cams, secs, sb), (len(many), many, mcams, msecs, sb),
        (2, rects((0, 0, 160, 240), (160, 0, 0, 240)), cams, secs, sb),                  # w < 1
        (2, rects((0, 0, 160, 240), (160, 0, 160, -1)), cams, secs, sb),                 # h < 1
        (2, rects((0, 0, 160, 240), (164, 0, 160, 240)), cams, secs, sb),                # one group outside
        (2, rects((0, 0, 160, 240), (160, 1, 160, 240)), cams, secs, sb),                # one row outside
        (1, rects((-4, 0, 160, 240)), cams, secs, sb),
        (2, rects((0, 0, 164, 240), (160, 0, 160, 240)), cams, secs, sb),                # overlap
        (2, rects((0, 0, 160, 240), (156, 239, 160, 1)), cams, secs, sb),                # overlap by one group of one row
        (2, rects((0, 0, 160, 240), (162, 0, 156, 240)), cams, secs, sb),                # x % 4 with blur on
        (2, rects((0, 0, 158, 240), (160, 0, 160, 240)), cams, secs, sb),                # w % 4 with blur on
    ]
    for args in refused:
        assert _call(r, *args) == _lib.PWN_EINVAL, args[:2]
        _ok_after(r, cams, secs)
    assert _call(r, _lib.PWN_VIEWS_MAX, many, mcams, msecs, sb) == 0          # (the limit itself is fine)
    # the blur-only rules go with the blur
    r.set_blur_passes(0)
    for vp in (rects((0, 0, 160, 240), (162, 0, 156, 240)), rects((0, 0, 158, 240), (160, 0, 160, 240)), rects((1, 1, 1, 1), (3, 0, 17, 5))):
        assert _call(r, 2, vp, cams, secs, sb) == 0
    r.set_blur_passes(1)
    # W % 4 != 0 with blur on
    odd = _renderer(322, 200, "pwnfps_level", "t0", blur=1)
    osb = np.zeros((200, 322), np.uint32)
    assert _call(odd, 1, rects((0, 0, 160, 200)), cams, secs, osb) == _lib.PWN_EINVAL
    odd.set_blur_passes(0)
    assert _call(odd, 2, rects((0, 0, 161, 200), (161, 0, 161, 200)), cams, secs, osb) == 0 and osb[:, :161].any() and osb[:, 161:].any()
    odd.close()
    # before a level
    nl = _renderer(w, h)
    assert _call(nl, 3, good, cams, secs, sb) == _lib.PWN_ENOLEVEL
    nl.level_load(level_path("pwnfps_level"))
    nl.set_objects(load_spheres("t0"))
    _ok_after(nl, cams, secs)
    nl.close()
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(w, h, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    g.set_objects(load_spheres("t0"))
    assert _call(g, 3, good, cams, secs, sb) == _lib.PWN_ENOTSUP
    with pytest.raises(pwnfps_amd.PwnError):
        g.trace_viewports(good, cams[:3], secs[:3])
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert _call(r, 3, good, cams, secs, sb) == _lib.PWN_EBUSY
    r.tiled_shutdown()
    _ok_after(r, cams, secs)
    r.close()


@pytest.mark.parametrize("w,h,blur", [(332, 202, 0), (320, 240, 1)])
def test_full_frame_viewport_equals_trace_views(oracle_lib, w, h, blur):
    cams, secs = _random_cams(np.random.default_rng(8 + w), oracle_lib, "pwnfps_level", 1)
    r = _renderer(w, h, "pwnfps_level", "t0", blur=blur)
    a, za = r.trace_viewports([(0, 0, w, h)], cams, secs)
    r.close()
    r = _renderer(w, h, "pwnfps_level", "t0", blur=blur)
    b, zb = r.trace_views(cams, secs)
    r.close()
    assert a.any() and (a == b[0]).all() and (_bits(za) == _bits(zb[0])).all()
