"""Every shipped kernel variant and call path on the hard scenes (tests/hard_scenes.py) and on hostile depths.

The default blocking call already runs the hard scenes (test_gpu_parity.py, test_nonfinite.py).  Here the same scenes go
through the other compiled variants of the trace kernel (COUNT, HAS_W, all three sphere-list forms -- indexed, inline, and the
records in device memory --, ORDER with a sorted hand-out, VIEWS) and of the blur (the 32x32 tile, the CHECK forms of row strips and groups, the VIEWS tiles), and through the other
entry points: pwn_trace_views, forced call strips, frames in flight on two streams, a three-member group, the refill
scheduler.  Colour and depth are compared bit for bit with the oracle, counters where they are on; a path that cannot take a
scene must refuse it with its documented error.

The blur differential matrix at the end drives pwn_blur_rows_device[_bounded] directly with random pre-blur words and
chosen depth planes, on both tiles, against the oracle's blur and a NumPy model of the taps' rows.
"""
import contextlib
import os

import numpy as np
import pytest

import hard_scenes as HS
from oracle import SPHERE_DTYPE

pytestmark = pytest.mark.gpu

SCENES = HS.scenes(SPHERE_DTYPE)
IDS = [s.name for s in SCENES]
PWN_EINVAL = -1
ROOM = 256                         # PWN_OPT_TRACE_ROOM: any room > 0 selects the 32x32 blur tile on narrow frames


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


def _ctx(sc, w=None, h=None, env=None, devices=None):
    """a context with the scene's level and spheres (env: variables read when the context is created)"""
    import pwnfps_amd
    with _env(**(env or {})):
        r = pwnfps_amd.Renderer(w or sc.w, h or sc.h, devices=devices)
    HS.load_renderer(r, sc)
    return r


def _blur(sc):
    return 1 if sc.blur_ok else 0


def _same(what, got, gz, want, wz):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (HS.bits(gz) == HS.bits(wz)).all(), (what, "depth", np.argwhere(HS.bits(gz) != HS.bits(wz))[:4].tolist())


def _blocking(r, plane, sc, what, cam=None, sec=None, counters=False):
    cam = sc.cam if cam is None else cam
    sec = sc.sec if sec is None else sec
    a, za = r.trace_screen_centred(cam, sec)
    b, zb, st = plane.frame(cam, sec, r._blur)
    _same((sc.name, what), a, za, b, zb)
    if counters:
        assert HS.stats5(r.stats()) == HS.stats5(st), (sc.name, what)


def _set_blur(r, n):
    r.set_blur_passes(n)
    r._blur = n


def _refuses_blur(r, sc, call):
    """w % 4 != 0: a blur of whole 4-pixel groups cannot run (screen.h:88); the call says so"""
    import pwnfps_amd
    _set_blur(r, 1)
    with pytest.raises(pwnfps_amd.PwnError) as e:
        call()
    assert e.value.code == PWN_EINVAL, (sc.name, e.value)
    _set_blur(r, 0)


def _view_cams(sc):
    """three views: the scene's camera at sec and at sec + 0.5, and a camera of another scene on the same level (else the
    scene's camera turned)"""
    import pwnfps_amd
    other = next((s.cam for s in SCENES if s.level == sc.level and s.name != sc.name and
                  not np.array_equal(s.cam, sc.cam)), None)
    if other is None:
        other = pwnfps_amd.mat4_roty(sc.cam, 0.5)
    cams = np.stack([sc.cam, sc.cam, other]).astype(np.float32)
    secs = np.array([sc.sec, sc.sec + 0.5, sc.sec], np.float32)
    return cams, secs


def _views(r, planes, sc, what, counters=False, cams=None, secs=None):
    if cams is None:
        cams, secs = _view_cams(sc)
    a, za = r.trace_views(cams, secs)
    want = [0] * 5
    for i in range(len(cams)):
        b, zb, st = planes[i].frame(cams[i], secs[i], r._blur)
        _same((sc.name, what, "view %d" % i), a[i], za[i], b, zb)
        want = [x + y for x, y in zip(want, HS.stats5(st))]
    if counters:
        assert HS.stats5(r.stats()) == tuple(want), (sc.name, what)


# ---------------------------------------------------------------- the blocking call ----

def _strips(h, k):
    """PWN_OPT_CALL_STRIPS = k: strips of whole 32-row blur tiles (pwn_calls.cpp strip_cuts); a frame of one strip runs in one piece"""
    per = ((h + k - 1) // k + 31) // 32 * 32
    return (h + per - 1) // per


@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_blocking_call_variants(sc, oracle_lib):
    """One context, options changed between calls (the depth plane carries over): the 32x32 blur tile on a narrow frame,
    the COUNT variants with their counters, the refill scheduler, forced call strips on either CHECK tile."""
    O = HS.oracle(oracle_lib, sc)
    plane = HS.Plane(O, sc.w, sc.h)
    r = _ctx(sc)
    if not sc.blur_ok:
        _refuses_blur(r, sc, lambda: r.trace_screen_centred(sc.cam, sc.sec))
    _set_blur(r, _blur(sc))
    assert r.trace_room_state()["room_now"] == 0
    _blocking(r, plane, sc, "default")
    r.set_trace_room(ROOM)
    assert r.trace_room_state()["room_now"] == ROOM
    _blocking(r, plane, sc, "room")
    r.set_counters(True)
    _blocking(r, plane, sc, "counters", counters=True)
    _blocking(r, plane, sc, "counters sec+0.5", sec=sc.sec + 0.5, counters=True)
    r.set_scheduler("refill")
    _blocking(r, plane, sc, "refill counters", counters=True)
    r.set_counters(False)
    _blocking(r, plane, sc, "refill")
    r.set_scheduler("units")
    if sc.h >= 16:
        assert sc.h <= 32 or _strips(sc.h, 2) >= 2
        for room in (0, ROOM):
            r.set_trace_room(room)
            for k in (2, 7):
                r.set_call_strips(k)
                _blocking(r, plane, sc, "call strips %d room %d" % (k, room))
                st = r.call_strips_state()
                assert st["strips_last"] == _strips(sc.h, k) and st["redone"] <= st["calls_in_strips"], (sc.name, k, st)
        r.set_call_strips(-1)
    r.close()


@pytest.mark.parametrize("variant", ["force_hasw", "indexed", "inline", "global"])
@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_context_variants(sc, variant, oracle_lib):
    """Variants chosen when the context is created: HAS_W forced (PWN_DBG_FORCE_HASW), and each sphere-list form
    (PWN_SPHERE_LISTS, the LISTS template parameter; global: the records in device memory, tables.h PWN_LF_GLOBAL, which
    every scene plans when forced, one whose spheres bin into no cell too): the blocking call with and without counters,
    the 32x32 tile, a batch of views."""
    env = {"force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "indexed": {"PWN_SPHERE_LISTS": "indexed"},
           "inline": {"PWN_SPHERE_LISTS": "inline"}, "global": {"PWN_SPHERE_LISTS": "global"}}[variant]
    O = HS.oracle(oracle_lib, sc)
    plane = HS.Plane(O, sc.w, sc.h)
    r = _ctx(sc, env=env)
    if variant == "global":
        assert r.sphere_tables()["form"] == 2, (sc.name, r.sphere_tables())
        if not sc.blur_ok:
            _refuses_blur(r, sc, lambda: r.trace_screen_centred(sc.cam, sc.sec))
    _set_blur(r, _blur(sc))
    _blocking(r, plane, sc, variant)
    r.set_counters(True)
    _blocking(r, plane, sc, variant + " counters", counters=True)
    views = [HS.Plane(O, sc.w, sc.h) for _ in range(3)]
    _views(r, views, sc, variant + " views counters", counters=True)
    r.set_counters(False)
    r.set_trace_room(ROOM)
    _blocking(r, plane, sc, variant + " room")
    _views(r, views, sc, variant + " views room")
    r.close()


# ---------------------------------------------------------------- pwn_trace_views ----

@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_views(sc, oracle_lib):
    """A batch of three views, again and again on one context (each slot's depth carries over): the plain VIEWS variants
    with the 128x16 VIEWS blur, with counters, with room (the 32x32 VIEWS blur)"""
    O = HS.oracle(oracle_lib, sc)
    r = _ctx(sc)
    cams, secs = _view_cams(sc)
    if not sc.blur_ok:
        _refuses_blur(r, sc, lambda: r.trace_views(cams, secs))
    _set_blur(r, _blur(sc))
    planes = [HS.Plane(O, sc.w, sc.h) for _ in range(3)]
    _views(r, planes, sc, "views")
    r.set_counters(True)
    _views(r, planes, sc, "views counters", counters=True)
    r.set_counters(False)
    r.set_trace_room(ROOM)
    assert r.trace_room_state()["room_now"] == ROOM
    _views(r, planes, sc, "views room")
    # the blocking call's plane is left alone by the batches
    _blocking(r, HS.Plane(O, sc.w, sc.h), sc, "blocking after views")
    r.close()


def test_views_and_blocking_call_on_a_wide_frame(oracle_lib):
    """w >= 2560: the 32x32 tiles are chosen without any option, for the blocking call and the VIEWS blur"""
    far = [s for s in SCENES if s.kind == "far"]
    for sc in far[:2]:
        w, h = 2560, 64
        O = HS.oracle(oracle_lib, sc)
        r = _ctx(sc, w, h)
        _set_blur(r, 1)
        assert r.trace_room_state()["room_now"] == 0
        planes = [HS.Plane(O, w, h) for _ in range(3)]
        cams, secs = _view_cams(sc)
        _views(r, planes, sc, "wide views", cams=cams, secs=secs)
        r.set_counters(True)
        _views(r, planes, sc, "wide views counters", counters=True, cams=cams[::-1].copy(), secs=secs[::-1].copy())
        r.set_counters(False)
        _blocking(r, HS.Plane(O, w, h), sc, "wide blocking")
        r.close()


# ---------------------------------------------------------------- ORDER ----

def _order_size(sc):
    """the sort needs at least 256 16x4 units (4 per queue): the scene's own size where it has them, else 320x208"""
    units = ((sc.w + 15) // 16) * ((sc.h + 3) // 4)
    return (sc.w, sc.h) if units >= 256 else (320, 208)


@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_sorted_unit_order(sc, oracle_lib):
    """PWN_OPT_UNIT_ORDER: the second frame of a camera is traced in the order the first one's costs sorted (the ORDER
    variant); it is the oracle's frame on the depth the first frame left.  That second frame is the one the planes hold already,
    so the frame follows twice as device rows into planes of poison (tests/handout.py), a moment later: the second of those
    launches runs in the order sorted from the first, and a unit it did not trace keeps the poison"""
    import torch
    import handout as H
    w, h = _order_size(sc)
    O = HS.oracle(oracle_lib, sc)
    plane = HS.Plane(O, w, h)
    r = _ctx(sc, w, h)
    _set_blur(r, 1 if w % 4 == 0 else 0)
    r.set_unit_order(True)
    _blocking(r, plane, sc, "order frame 1 at %dx%d" % (w, h))
    assert r.unit_order_state()["launches_in_sorted_order"] == 0
    _blocking(r, plane, sc, "order frame 2 at %dx%d" % (w, h))
    st = r.unit_order_state()
    assert st["launches_in_sorted_order"] >= 1 and st["sorts"] >= 1, (sc.name, st)
    assert w % 4 == 0          # (the blur behind a strip's trace is what sorts its costs)
    sec = np.float32(sc.sec + 0.5)
    poison_z = np.full((h, w), H.POISON_Z, np.uint32).view(np.float32)
    want_sb, want_z, _ = O.trace_rows(w, h, 0, h, sc.cam, sec=sec, sb=np.full((h, w), H.POISON_S, np.uint32), zb=poison_z)
    assert not (want_sb == H.POISON_S).any(), sc.name
    d_out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for k in range(2):
        d_sb = torch.full((h, w), H.POISON_S, dtype=torch.int32, device="cuda")
        d_zb = torch.full((h, w), H.POISON_Z, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.trace_rows_device(sc.cam, sec, 0, h, d_sb.data_ptr(), d_zb.data_ptr())
        r.blur_rows_device(0, h, d_sb.data_ptr(), d_zb.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        H.same((sc.name, "device rows", k), d_sb.cpu().numpy(), d_zb.cpu().numpy(), want_sb, want_z)
        now = r.unit_order_state()
        assert now["launches_in_sorted_order"] == st["launches_in_sorted_order"] + k and now["sorts"] == st["sorts"] + k + 1, (sc.name, k, st, now)
    r.close()


# ---------------------------------------------------------------- frames in flight, groups ----

@pytest.mark.parametrize("sc", SCENES, ids=IDS)
def test_frames_in_flight_on_two_streams(sc, oracle_lib):
    """Two slots on two streams with room beside the trace grid (the 32x32 tile): both slots start from zero depth, so
    either delivered frame is the fresh oracle frame of its submit"""
    O = HS.oracle(oracle_lib, sc)
    r = _ctx(sc)
    _set_blur(r, _blur(sc))
    r.set_trace_room(ROOM)
    r.frames_config(2, sbuf=True, zbuf=True)
    secs = (sc.sec, sc.sec + 0.5)
    for slot in (0, 1):
        r.submit_frame(sc.cam, secs[slot], slot)
    for slot in (0, 1):
        fr = r.wait_frame(slot)
        b, zb, _ = HS.fresh(O, sc.w, sc.h, sc.cam, np.float32(secs[slot]), r._blur)
        _same((sc.name, "frames in flight slot %d" % slot), fr["sbuf"], fr["zbuf"], b, zb)
    assert r.trace_room_state()["room_now"] == ROOM
    r.frames_config(0)
    r.close()


GROUP_SCENES = [s for s in SCENES if s.h >= 24]


@pytest.mark.parametrize("sc", GROUP_SCENES, ids=[s.name for s in GROUP_SCENES])
def test_group_of_three_on_one_device(sc, oracle_lib):
    """pwn_init_multi with three members on device 0: the frame is cut in row strips, each member blurs its strip with the
    CHECK blur over the rows it holds and repeats what leaves them"""
    O = HS.oracle(oracle_lib, sc)
    r = _ctx(sc, devices=[0, 0, 0])
    assert r.group_info()["members"] == 3
    _set_blur(r, _blur(sc))
    plane = HS.Plane(O, sc.w, sc.h)
    _blocking(r, plane, sc, "group")
    _blocking(r, plane, sc, "group sec+0.5", sec=sc.sec + 0.5)
    r.close()


# ---------------------------------------------------------------- the blur, differential ----
#
# Tile shapes: pwn_i_launch_blur takes 128x16 while w < 2560 with no room beside the trace grid, else 32x32.  The tame fast
# path runs for a wave while every |z - 1| of its lanes is below 1e6; one lane above sends the whole wave to the general path.

TILES = {0: (128, 16), ROOM: (32, 32)}
SIZES = [(w, h) for w in (4, 28, 36, 132, 2564) for h in (1, 3, 17, 33)] + [(8, 4320), (32, 8640)]
HOSTILE = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1.2e10, -1.2e10, 2.4e10, 1e30, -1e30, 1e38, -1e38,
                    1.1184e10, -1.1184e10, 5.5e9, 0.0, -0.0, 1.0, 1e-40,
                    # above the tame bound, below 2^31 / fstr on small frames, beyond it on tall ones
                    1000001.0, -999999.0, 4.0e8, -4.0e8, 9.0e8, 2.5e8], np.float32)
NOT_TAME = HOSTILE[~(np.abs(HOSTILE - np.float32(1.0)) < np.float32(1e6))]
# |z - 1| just below and at / above 1e6: on tall frames the tame path's tap coordinates pass 2^24
NEAR_BELOW = np.float32(1.0) + np.array([999999.94, -999999.94, 999999.0, -999999.0, 999998.0, 524288.0], np.float32)
NEAR_ABOVE = np.float32(1.0) + np.array([1e6, -1e6, 1000064.0, -1000064.0], np.float32)
# above the tame bound and far enough that fstr * |z - 1| passes 2^31 on tall frames: only the general path converts these
# as cvttss2si does
BIG = np.array([2.5e8, -2.5e8, 4.0e8, -4.0e8, 9.0e8, -9.0e8], np.float32)
SENTINEL = np.uint32(0xA5C3E1F7)


def _fstr(h):
    return np.float32(0.002) * np.float32(h)


def _tame(rng, w, h):
    """taps up to ~40 pixels away: inside the staged halo (16), beyond it, and off every edge"""
    span = min(40.0 / float(_fstr(h)), 9.0e5)
    z = np.float32(1.0) + (rng.uniform(-1, 1, (h, w)) * span).astype(np.float32)
    z.reshape(-1)[rng.integers(0, h * w, max(1, h * w // 16))] = 1.0
    assert (np.abs(z - np.float32(1.0)) < np.float32(1e6)).all()
    return z


def _waves(w, h, y0, y1, tile):
    """the 4-pixel groups (g, cy) of every wave64 of a launch over rows [y0, y1), in lane order (post_kernels.hip:
    tile t at x0 = (t % tiles_x) * TW, y0 + (t / tiles_x) * TH; thread i of it takes group x0 / 4 + i % (TW / 4), row
    i / (TW / 4); lanes without a group in the frame leave before the ballot)"""
    tw, th = tile
    out = []
    for ty in range((y1 - y0 + th - 1) // th):
        for tx in range((w + tw - 1) // tw):
            t = np.arange(tw // 4 * th)
            g = tx * tw // 4 + t % (tw // 4)
            cy = y0 + ty * th + t // (tw // 4)
            for k in range(0, len(t), 64):
                gg, yy = g[k:k + 64], cy[k:k + 64]
                ok = (gg < w // 4) & (yy < y1)
                if ok.any():
                    out.append((gg[ok], yy[ok]))
    return out


def _one_per_wave(rng, z, y0, y1, tile, lane, values):
    """one non-tame pixel in exactly one 4-pixel group of every wave: the wave's first or last lane"""
    h, w = z.shape
    z = z.copy()
    for gg, yy in _waves(w, h, y0, y1, tile):
        i = 0 if lane == "first" else -1
        z[yy[i], 4 * gg[i] + rng.integers(0, 4)] = values[rng.integers(0, len(values))]
    return z


def _depths(rng, cls, w, h, y0, y1, tile):
    if cls == "tame":
        return _tame(rng, w, h)
    if cls in ("wave_first", "wave_last"):
        return _one_per_wave(rng, _tame(rng, w, h), y0, y1, tile, cls[5:], NOT_TAME)
    if cls in ("big_first", "big_last"):
        return _one_per_wave(rng, _tame(rng, w, h), y0, y1, tile, cls[4:], BIG)
    if cls == "hostile":
        z = (1.0 + rng.standard_normal((h, w)) * 8.0).astype(np.float32)
        idx = rng.integers(0, h * w, max(1, h * w // 4))
        z.reshape(-1)[idx] = HOSTILE[rng.integers(0, len(HOSTILE), len(idx))]
        return z
    if cls == "near_below":
        return NEAR_BELOW[rng.integers(0, len(NEAR_BELOW), (h, w))]
    if cls == "near_mixed":
        z = NEAR_BELOW[rng.integers(0, len(NEAR_BELOW), (h, w))]
        idx = rng.integers(0, h * w, max(1, h * w // 512))
        z.reshape(-1)[idx] = NEAR_ABOVE[rng.integers(0, len(NEAR_ABOVE), len(idx))]
        return z
    raise ValueError(cls)


def _classes(h):
    return ["tame", "wave_first", "wave_last", "hostile"] + (["near_below", "near_mixed", "big_first", "big_last"] if h >= 4096 else [])


def _windows(rng, h):
    """row windows [y0, y1) aligned to neither tile height: the whole frame, a random one, single rows"""
    out = [(0, h), (h - 1, h)]
    if h >= 3:
        out.append((1, 2))
        y0 = int(rng.integers(1, h - 1))
        out.append((y0, int(rng.integers(y0 + 1, h))))
    if h >= 4096:
        out.append((h // 2 + 5, h // 2 + 42))
    return out


_SKIP = {}


def _skip(n):
    """(A_d, C_d) for d = 1..n: the row LCG after d draws is (A_d * s + C_d) mod 2^31"""
    if n not in _SKIP:
        a, c = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        x, y = 1, 0
        for d in range(n):
            x, y = (x * 25739) & 0x7FFFFFFF, (y * 25739 + 4) & 0x7FFFFFFF
            a[d], c[d] = x, y
        _SKIP[n] = (a, c)
    return _SKIP[n]


def _tap_rows(z, y0, y1):
    """the row every tap of every 4-pixel group of rows [y0, y1) reads (screen.h:101-106, float32 op by op: cvttss2si, INT_MIN
    for NaN and out of range, then the clamp) -> [rows, groups, 16]"""
    h, w = z.shape
    groups = w // 4
    a, c = _skip(32 * groups)
    cy = np.arange(y0, y1, dtype=np.uint64)
    seed0 = (cy * cy + 415135) & 0x7FFFFFFF
    # draw 2 (4 i + j) + 1 of group g is tap (i, j)'s x, the next one its y
    seeds = ((a[None, :] * seed0[:, None] + c[None, :]) & 0x7FFFFFFF).reshape(y1 - y0, groups, 4, 4, 2)[..., 1]
    fs = (seeds % 3759).astype(np.float32) * (np.float32(1.0) / np.float32(3759.0)) * np.float32(2.0) - np.float32(1.0)
    zm = (z[y0:y1, :groups * 4] - np.float32(1.0)).astype(np.float32).reshape(y1 - y0, groups, 1, 4)
    with np.errstate(all="ignore"):
        fy = cy.astype(np.float32)[:, None, None, None] + (fs * _fstr(h)) * zm
        ok = (fy >= np.float32(-2147483648.0)) & (fy < np.float32(2147483648.0))
        y = np.where(ok, np.trunc(np.where(ok, fy, np.float32(0))), np.float32(-2147483648.0)).astype(np.int64)
    return np.clip(y, 0, h - 1).reshape(y1 - y0, groups, 16)


class _Blur:
    """one context of the frame's size, device buffers, and the room option that picks the tile"""

    def __init__(self, w, h):
        import pwnfps_amd
        import torch
        self.w, self.h, self.torch = w, h, torch
        self.r = pwnfps_amd.Renderer(w, h)
        dev = torch.device("cuda:0")
        self.pre = torch.zeros((h, w), dtype=torch.int32, device=dev)
        self.z = torch.zeros((h, w), dtype=torch.float32, device=dev)
        self.out = torch.zeros((h, w), dtype=torch.int32, device=dev)
        self.miss = torch.zeros(1, dtype=torch.int32, device=dev)
        self.s = torch.cuda.current_stream().cuda_stream

    def room(self, room):
        self.r.set_trace_room(room)
        assert self.r.trace_room_state()["room_now"] == room

    def run(self, pre, z, y0, y1, avail=None):
        t = self.torch
        self.pre.copy_(t.from_numpy(pre.view(np.int32)))
        self.z.copy_(t.from_numpy(z))
        self.out.fill_(int(SENTINEL.view(np.int32)))
        self.miss.zero_()
        if avail is None:
            self.r.blur_rows_device(y0, y1, self.pre.data_ptr(), self.z.data_ptr(), self.out.data_ptr(), self.s)
        else:
            self.r.blur_rows_device_bounded(y0, y1, self.pre.data_ptr(), self.z.data_ptr(), self.out.data_ptr(),
                                            avail[0], avail[1], self.miss.data_ptr(), self.s)
        t.cuda.synchronize()
        out = self.out.cpu().numpy().view(np.uint32)
        assert (out[:y0] == SENTINEL).all() and (out[y1:] == SENTINEL).all(), "rows outside [y0, y1) written"
        return out, int(self.miss.item())

    def close(self):
        self.r.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_blur_matrix(size, oracle_lib):
    """pwn_blur_rows_device on both tiles, every depth class, unaligned row windows: the oracle's blur bit for bit"""
    w, h = size
    rng = np.random.default_rng(w * 100003 + h)
    O = oracle_lib.Oracle()
    B = _Blur(w, h)
    for room, tile in TILES.items():
        B.room(room)
        tile = (32, 32) if w >= 2560 else tile
        for cls in _classes(h):
            for y0, y1 in _windows(rng, h):
                pre = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
                z = _depths(rng, cls, w, h, y0, y1, tile)
                got, _ = B.run(pre, z, y0, y1)
                want = O.blur_rows(y0, y1, pre, z)
                bad = got[y0:y1] != want[y0:y1]
                assert not bad.any(), (w, h, tile, cls, (y0, y1), int(bad.sum()), (np.argwhere(bad)[:4] + [y0, 0]).tolist())
    B.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_bounded_blur_matrix(size, oracle_lib):
    """pwn_blur_rows_device_bounded (the CHECK variants of row strips, call strips and groups): rows outside the available
    window [a0, a1) hold another frame.  The strip is what the oracle blurs from the memory as it stands; a tap outside the
    window is counted once per 4-pixel group, exactly as a NumPy model of the taps' rows says; so a miss count of 0 means
    the strip is the clean frame's, and a strip that the poison changed has a count above 0."""
    w, h = size
    rng = np.random.default_rng(w * 7919 + h)
    O = oracle_lib.Oracle()
    B = _Blur(w, h)
    checked = 0
    for room, tile in TILES.items():
        B.room(room)
        tile = (32, 32) if w >= 2560 else tile
        for cls in _classes(h):
            for y0, y1 in _windows(rng, h):
                for tight in (True, False):
                    a0 = y0 if tight else int(rng.integers(0, y0 + 1))
                    a1 = y1 if tight else int(rng.integers(y1, h + 1))
                    clean = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
                    z = _depths(rng, cls, w, h, y0, y1, tile)
                    poisoned = clean.copy()
                    poisoned[:a0] = rng.integers(0, 2 ** 32, (a0, w), dtype=np.uint64).astype(np.uint32)
                    poisoned[a1:] = rng.integers(0, 2 ** 32, (h - a1, w), dtype=np.uint64).astype(np.uint32)
                    got, miss = B.run(poisoned, z, y0, y1, avail=(a0, a1))
                    want_clean = O.blur_rows(y0, y1, clean, z)[y0:y1]
                    want_poisoned = O.blur_rows(y0, y1, poisoned, z)[y0:y1]
                    what = (w, h, tile, cls, (y0, y1), (a0, a1), miss)
                    assert (got[y0:y1] == want_poisoned).all(), what
                    rows = _tap_rows(z, y0, y1)
                    assert miss == int(((rows < a0) | (rows >= a1)).any(axis=2).sum()), what
                    if miss == 0:
                        assert (got[y0:y1] == want_clean).all(), what
                    if (want_poisoned != want_clean).any():
                        assert miss > 0, what
                        checked += 1
    assert checked > 0 or h == 1          # (one row: nothing outside the window to poison)
    B.close()
