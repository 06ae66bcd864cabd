"""pwn_trace_view_hits: first-hit planes of a batch of views.  Pixel (x, y) of view i is the record pwn_trace_hits returns for
pwn_pixel_rays' ray of that pixel, packed (pwnhip.h PWN_LABEL_*): the ray form on the same context is the reference for every pixel
and every field that has a place, hit_chain.Reader on the oracle for sampled pixels straight against the reference's event chain.
Floats compare as bits.  Contexts are the scenes' own small sizes.
"""
import contextlib
import os

import numpy as np
import pytest

import big_scenes as BS
import hard_scenes as HS
import hit_chain as HC
from conftest import GOLD, level_path, load_spheres
from oracle import SPHERE_DTYPE

pytestmark = pytest.mark.gpu

SCENES = HS.scenes(SPHERE_DTYPE)
BY_NAME = {s.name: s for s in SCENES}
PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
VARIANTS = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}, "inline": {"PWN_SPHERE_LISTS": "inline"},
            "indexed": {"PWN_SPHERE_LISTS": "indexed"}, "global": {"PWN_SPHERE_LISTS": "global"}}
# the other three variants run these eight.  By the oracle, of 516 sampled pixels: sec_3e7 has 108 behind portals, open_inside 163
# that end in a ramp cell, sphere_r_big 125 on its sphere; a non-finite scene; odd sizes; spheres behind portals; a far start
SUBSET = ("sec_3e7", "open_inside", "sphere_r_big", "nonfinite_lattice_77_458", "level_33x7", "level_68x40", "sphere_refl_gt1_axis",
          "far_fuzz_9004_544")
SENTINEL = 0x7fc12345                     # a NaN pattern no computation makes
GUARD = 64
PLANE_FIELDS = ("kind", "face", "object", "portals", "dist", "cell_x", "cell_z")


def _level_text(sc):
    return open(sc.level).read() if HS.is_path(sc.level) else sc.level


assert len(SCENES) == 42 and len(set(SUBSET)) == 8 and set(SUBSET) <= set(BY_NAME)
assert any(c in _level_text(BY_NAME["open_inside"]) for c in "<>^,") and "A" in _level_text(BY_NAME["sec_3e7"])
assert len(BY_NAME["sphere_r_big"].spheres) > 0 and BY_NAME["nonfinite_lattice_77_458"].kind == "nonfinite"


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


def _renderer(variant, w, h):
    import pwnfps_amd
    with _env(**VARIANTS[variant]):
        r = pwnfps_amd.Renderer(w, h)
    r.set_blur_passes(0)
    return r


def _level_renderer(w, h, variant="plain"):
    r = _renderer(variant, w, h)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(HC.mark_spheres(load_spheres("t0")))
    return r


def _form_is_forced(r, variant, what):
    """global: the context really holds its tables in device memory (a misspelt variable would leave them on chip)"""
    if variant == "global":
        assert r.sphere_tables()["form"] == 2, (what, r.sphere_tables())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _planes_of_hits(hits, shape):
    """(label, cell word, dist bits), uint32 of `shape`, of HIT_DTYPE records: what the planes must hold"""
    import pwnfps_amd
    hits = np.ascontiguousarray(hits)
    words = hits.view(np.uint32).reshape(len(hits), 12)
    return pwnfps_amd.pack_labels(hits).reshape(shape), words[:, 11].reshape(shape).copy(), words[:, 4].reshape(shape).copy()


def _ray_form(r, cams):
    """the reference planes of views `cams` on context r, by the ray form: (n,h,w) uint32 each"""
    import pwnfps_amd
    out = []
    for cam in cams:
        rays, _, xy = pwnfps_amd.pixel_rays(r.w, r.h, cam)
        assert (xy == HC.all_pixels(r.w, r.h)).all()
        out.append(_planes_of_hits(r.trace_hits(rays), (r.h, r.w)))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def _host_form(r, cams):
    """trace_view_hits' three planes as uint32 words"""
    label, cell, dist = r.trace_view_hits(np.asarray(cams, np.float32))
    n = len(cams)
    assert label.shape == (n, r.h, r.w) and label.dtype == np.uint32
    assert cell.shape == (n, r.h, r.w, 2) and cell.dtype == np.int16 and dist.shape == (n, r.h, r.w) and dist.dtype == np.float32
    return label, cell.view(np.uint32).reshape(n, r.h, r.w), _bits(dist)


def _same(got, want, what):
    for name, g, w in zip(("label", "cell", "dist"), got, want):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:3].tolist(), [hex(int(g[tuple(b)])) for b in bad[:3]], [hex(int(w[tuple(b)])) for b in bad[:3]])


def _device_form(r, cams, want=("label", "cell", "dist"), has_w=False, stream=None):
    """the device form into planes with GUARD words on each side, all filled with the sentinel first: (the buffers by name, the
    camera tensor).  Everything is enqueued on `stream` (None: torch's current one) and nothing is waited for."""
    import torch
    dev = torch.device("cuda", 0)
    cams = np.ascontiguousarray(np.asarray(cams, np.float32).reshape(len(cams), 16))
    n, N = len(cams), len(cams) * r.h * r.w
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx:
        t_cams = torch.from_numpy(cams).to(dev)
        bufs = {k: torch.full((N + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev) for k in want}
        pl = {k: b[GUARD:GUARD + N].view(n, r.h, r.w) for k, b in bufs.items()}
        dist = pl["dist"].view(torch.float32) if "dist" in pl else None
        r.trace_view_hits_device(t_cams, pl["label"], pl.get("cell"), dist, has_w=has_w, stream=stream)
    return bufs, t_cams


def _read_guarded(r, bufs, n):
    """(planes as uint32 (n,h,w) by name) of _device_form's buffers, once the stream is through: every guard word still the
    sentinel, no plane word the sentinel"""
    N = n * r.h * r.w
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy().view(np.uint32)
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + N:] == SENTINEL).all(), (k, "guard words written")
        assert len(a) == N + 2 * GUARD
        p = a[GUARD:GUARD + N].reshape(n, r.h, r.w)
        assert not (p == SENTINEL).any(), (k, "pixels not written", np.argwhere(p == SENTINEL)[:4].tolist())
        out[k] = p
    return out


def _cams_at_spawn(r, n, tilt=0.0):
    import pwnfps_amd
    _, _, spawn = r.get_level()
    return np.stack([pwnfps_amd.spawn_camera(spawn, ang_y=0.35 + 0.9 * i, ang_x=tilt * (i % 3 - 1)) for i in range(n)]).astype(np.float32)


# ---------------------------------------------------------------- 1. equal to the ray form, every pixel, every field ----

CASES = [pytest.param(sc, v, id=sc.name + "-" + v) for sc in SCENES for v in VARIANTS if v in ("plain", "global") or sc.name in SUBSET]
assert len(CASES) == 42 * 2 + 8 * 3


@pytest.mark.parametrize("sc,variant", CASES)
def test_hard_scenes_equal_the_ray_form(sc, variant):
    """each hard scene as a one-view batch: label, cell and dist are pack_labels, the cell word and the dist bits of
    trace_hits(pixel_rays(w, h, cam)) on the same context"""
    r = _renderer(variant, sc.w, sc.h)
    HS.load_renderer(r, sc)
    _form_is_forced(r, variant, sc.name)
    want = _ray_form(r, [sc.cam])
    got = _host_form(r, [sc.cam])
    r.close()
    _same(got, want, (sc.name, variant))
    assert np.isin(got[0] & 3, (0, 1, 2)).all()
    none = got[0] == 0
    assert (got[1][none] == 0).all() and (got[2][none] == 0).all()


# ---------------------------------------------------------------- 2. straight against the reference ----

def _sample(w, h, seed):
    n = w * h
    if n <= 516:
        return HC.all_pixels(w, h)
    pick = np.random.default_rng(seed).choice(n, 512, replace=False)
    xy = np.stack([pick % w, pick // w], 1).astype(np.int32)
    return np.concatenate([xy, np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.int32)])


@pytest.mark.parametrize("which", ["level", "sec_3e7", "open_inside"])
def test_against_the_oracles_event_chain(oracle_lib, which):
    """level.txt with the t0 spheres marked (every pixel of 32 x 24), a portal scene and a ramp scene (512 seeded pixels and the
    corners): kind, face, object, portals, dist and the cell against hit_chain.Reader -- not through pwn_pixel_rays"""
    import pwnfps_amd
    if which == "level":
        O, sph, cams, refs = HC.level_frames(oracle_lib)
        w, h, cam, ref, xy = HC.LEVEL_W, HC.LEVEL_H, cams[1], refs[1], HC.all_pixels(HC.LEVEL_W, HC.LEVEL_H)
        r = _level_renderer(w, h)
    else:
        sc = BY_NAME[which]
        sc = sc._replace(spheres=HC.mark_spheres(sc.spheres))
        O = oracle_lib.Oracle()
        HS.load_oracle(O, sc)
        w, h, cam = sc.w, sc.h, sc.cam
        xy = _sample(w, h, 77)
        ref = HC.Reader(O).pixels(w, h, cam, xy)
        r = _renderer("plain", w, h)
        HS.load_renderer(r, sc)
    if which == "sec_3e7":
        assert (ref.want["portals"] > 0).sum() >= 100
    if which == "open_inside":
        assert np.isin(ref.last_ch, [ord(c) for c in "<>^,"]).sum() >= 100
    if which == "level":
        assert (ref.want["kind"] == HC.SPHERE).any() and (ref.want["kind"] == HC.WALL).any()
    label, cell, dist = r.trace_view_hits(np.asarray(cam, np.float32).reshape(1, 16))
    r.close()
    x, y = xy[:, 0], xy[:, 1]
    got = ref.want.copy()               # (x y z and dx dy dz have no plane)
    got["kind"], got["face"], got["object"], got["portals"] = (a[0][y, x] for a in pwnfps_amd.unpack_labels(label))
    got["cell_x"], got["cell_z"] = cell[0, y, x, 0], cell[0, y, x, 1]
    got["dist"] = dist[0][y, x]
    bad = HC.mismatches(got, ref.want, fields=PLANE_FIELDS)
    assert len(bad) == 0, (which, len(bad), [(xy[i].tolist(), got[i].tolist(), ref.want[i].tolist()) for i in bad[:3]])


# ---------------------------------------------------------------- 3. geometry the hand-out can get wrong ----

@pytest.mark.parametrize("w,h", [(1, 1), (17, 5), (33, 3), (40, 10), (64, 8)])
def test_sizes_and_view_counts(w, h):
    """n = 1, 2, 3, 5 views (3 and 5: division by views_magic) of frames that end in half a tile, a partial unit row, one pixel:
    view i of the batch is the one-view call with camera i; planes with 64 guard words on each side, filled with a sentinel first,
    are written completely and nowhere else"""
    import torch
    r = _level_renderer(w, h)
    cams = _cams_at_spawn(r, 5, tilt=0.2)
    one = [_host_form(r, cams[i:i + 1]) for i in range(5)]
    want1 = _ray_form(r, cams[:1])
    _same(one[0], want1, (w, h, "one view against the ray form"))
    for n in (1, 2, 3, 5):
        bufs, _ = _device_form(r, cams[:n])
        torch.cuda.synchronize()
        got = _read_guarded(r, bufs, n)
        for i in range(n):
            _same([got[k][i:i + 1] for k in ("label", "cell", "dist")], one[i], (w, h, n, i))
        _same(_host_form(r, cams[:n]), [got[k] for k in ("label", "cell", "dist")], (w, h, n, "host form"))
    r.close()


# ---------------------------------------------------------------- 4. a sequence of launches ----

def test_sequence_of_device_calls_on_one_and_two_streams():
    """seven calls on one stream, then seven alternating strictly between two: round the counter sets (and the view records
    that go with them) more than once; every call's freshly poisoned planes are complete and equal the first call's"""
    import torch
    w, h, n = 40, 10, 3
    r = _level_renderer(w, h)
    cams = _cams_at_spawn(r, n, tilt=0.2)
    dev = torch.device("cuda", 0)
    s = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    calls = []
    for k in range(7):
        calls.append(_device_form(r, cams, stream=s[0]))
    for k in range(7):
        calls.append(_device_form(r, cams, stream=s[(k + 1) & 1]))
    torch.cuda.synchronize()
    first = _read_guarded(r, calls[0][0], n)
    _same([first[k] for k in ("label", "cell", "dist")], _ray_form(r, cams), "the first call against the ray form")
    for i, (bufs, _) in enumerate(calls[1:]):
        got = _read_guarded(r, bufs, n)
        _same([got[k] for k in ("label", "cell", "dist")], [first[k] for k in ("label", "cell", "dist")], ("call", i + 1))
    r.close()


# ---------------------------------------------------------------- 5. the portal field ----

CORRIDOR = ".........\n.A;;*;;A.\n.........\n"


def _corridor_cam(sign, eps, pos):
    """looking along +-x from pos, the middle row's rays climbing by eps per unit: pixel (w/2 - 1, h/2) is (sign, eps, 0) exactly"""
    cam = np.zeros((4, 4), np.float32)
    cam[0, :3] = (0, 0, 1)
    cam[1, :3] = (0, 1, 0)
    cam[2, :3] = (sign, eps, 0)
    cam[3] = (*pos, 1)
    return cam


def test_loop_corridor_portal_counts():
    """a corridor closed on itself by a portal pair.  A view's pixel (w/2 - 1, h/2) runs along it: with a climb of 5.5e-4 .. 1e-3
    per unit it reaches the ceiling or the floor after 100 crossings and more, with less it runs out of its 1000 steps (all three
    planes 0); portals and kind are the ray form's"""
    import pwnfps_amd
    w, h = 16, 8
    cams = np.stack([_corridor_cam(s, e, p) for s, e, p in [
        (1, 0.0, (2.25, 0.5, 1.5)), (-1, 0.0, (4.5, 0.5, 1.25)), (1, 1e-5, (6.75, 0.5, 1.5)), (1, -2e-4, (3.5, 0.5, 1.75)),
        (-1, 6e-4, (5.125, 0.5, 1.5)), (1, 5.5e-4, (4.5, 0.5, 1.25)), (1, -6.5e-4, (2.25, 0.5, 1.5)), (1, 1e-3, (2.25, 0.5, 1.5)),
        (1, 0.01, (2.25, 0.5, 1.5))]])
    r = _renderer("plain", w, h)
    r.level_load_text(CORRIDOR)
    r.set_objects(np.zeros(0, SPHERE_DTYPE))
    want = _ray_form(r, cams)
    got = _host_form(r, cams)
    r.close()
    _same(got, want, "corridor")
    kind, _, _, portals = pwnfps_amd.unpack_labels(got[0])
    wk, _, _, wp = pwnfps_amd.unpack_labels(want[0])
    assert (kind == wk).all() and (portals == wp).all()
    assert ((portals >= 100) & (kind != 0)).sum() >= 2, portals.max()
    none = kind == 0
    assert none.sum() >= 2 and (got[0][none] == 0).all() and (got[1][none] == 0).all() and (got[2][none] == 0).all()
    assert portals.max() <= 1000


# ---------------------------------------------------------------- 6. the object field beyond 11 bits ----

def test_objects_beyond_2047(oracle_lib):
    """swarm_near, 2100 live spheres (lists in device memory): a camera placed by the oracle in front of a sphere with an index
    above 2047; the planes are the ray form's and that index comes back through the 14-bit field"""
    import pwnfps_amd
    sc = BS.scene("swarm_near", oracle_lib)
    assert len(sc.spheres) == 2100            # (of big_scenes' tables with more than 2047 spheres the smaller; swarm_all has 10000)
    O = BS.oracle_for(sc, oracle_lib)
    rd = HC.Reader(O)
    w, h = 32, 24
    centre = np.array([[w // 2 - 1, h // 2]], np.int32)         # the pixel whose ray is the camera's z row exactly
    cam = None
    for i in range(2048, len(sc.spheres)):
        s = sc.spheres[i]
        c = np.eye(4, dtype=np.float32)
        c[3, :3] = (s["x"], s["y"], s["z"] - s["r"] - np.float32(0.15))
        ref = rd.pixels(w, h, c, centre)
        if ref.want["kind"][0] == HC.SPHERE and ref.want["object"][0] > 2047:
            cam, obj = c, int(ref.want["object"][0])
            break
    assert cam is not None, "no camera sees a sphere above 2047 at its centre pixel"
    r = _renderer("plain", w, h)
    r.level_load(BS.level_path(sc.level))
    r.set_objects(sc.spheres)
    assert r.sphere_tables()["form"] == 2
    want = _ray_form(r, [cam])
    got = _host_form(r, [cam])
    r.close()
    _same(got, want, "swarm_near")
    kind, _, objects, _ = pwnfps_amd.unpack_labels(got[0])
    assert (objects > 2047).any()
    assert kind[0, centre[0, 1], centre[0, 0]] == HC.SPHERE and objects[0, centre[0, 1], centre[0, 0]] == obj


# ---------------------------------------------------------------- 7. the device form ----

def test_device_form():
    """tensors in: planes equal to the host form's; cell and / or dist left out leave the others identical; PWN_VIEWS_HAS_W with
    cameras that have w components equals the host form on them, without the flag the cameras with w = 0, 0, 0, 1"""
    import torch
    w, h, n = 40, 10, 3
    r = _level_renderer(w, h)
    cams = _cams_at_spawn(r, n, tilt=0.2)
    host = _host_form(r, cams)
    names = ("label", "cell", "dist")
    for want in (names, ("label", "cell"), ("label", "dist"), ("label",)):
        bufs, _ = _device_form(r, cams, want=want)
        torch.cuda.synchronize()
        got = _read_guarded(r, bufs, n)
        assert set(got) == set(want)
        for k in want:
            assert (got[k] == host[names.index(k)]).all(), (want, k)
    # the host form without the optional planes
    label, cell, dist = r.trace_view_hits(cams, want_cell=False, want_dist=False)
    assert cell is None and dist is None and (label == host[0]).all()
    # w lanes
    wcams = cams.copy()
    wcams[:, 0, 3], wcams[:, 1, 3], wcams[:, 2, 3], wcams[:, 3, 3] = 0.015, -0.02, 0.01, 1.25
    plain = wcams.copy()
    plain[:, :3, 3], plain[:, 3, 3] = 0.0, 1.0
    host_w, host_plain = _host_form(r, wcams), _host_form(r, plain)
    assert any((a != b).any() for a, b in zip(host_w, host_plain)), "the w lanes change nothing: the check below would be empty"
    for flag, ref in ((True, host_w), (False, host_plain)):
        bufs, _ = _device_form(r, wcams, has_w=flag)
        torch.cuda.synchronize()
        got = _read_guarded(r, bufs, n)
        _same([got[k] for k in names], ref, ("has_w", flag))
    # int16 pairs for the cell plane, a (n,4,4) camera tensor
    dev = torch.device("cuda", 0)
    t_cams = torch.from_numpy(cams.reshape(n, 4, 4).copy()).to(dev)
    t_label = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    t_cell = torch.zeros((n, h, w, 2), dtype=torch.int16, device=dev)
    r.trace_view_hits_device(t_cams, t_label, cell=t_cell)
    torch.cuda.synchronize()
    assert (t_label.cpu().numpy().view(np.uint32) == host[0]).all()
    assert (t_cell.cpu().numpy().view(np.uint32).reshape(n, h, w) == host[1]).all()
    with pytest.raises(ValueError):
        r.trace_view_hits_device(t_cams, t_label[:, :, :-1].contiguous())
    with pytest.raises(ValueError):
        r.trace_view_hits_device(t_cams, torch.zeros(n * h * w + 4, dtype=torch.int32, device=dev)[1:1 + n * h * w].view(n, h, w))      # 4 B past an aligned start
    r.close()


# ---------------------------------------------------------------- 8. counters ----

def test_counters():
    """PWN_OPT_COUNTERS: rays = n w h; steps, portals, sphere tests and exhausted are the sums of trace_hits' counters over the
    views' pixel rays; the planes are those of the call without counting"""
    import pwnfps_amd
    w, h, n = 40, 10, 3
    r = _level_renderer(w, h)
    cams = _cams_at_spawn(r, n, tilt=0.2)
    plain = _host_form(r, cams)
    r.set_counters(True)
    keys = ("rays", "steps", "portals", "sphere_tests", "exhausted")
    total = dict.fromkeys(keys, 0)
    for cam in cams:
        rays, _, _ = pwnfps_amd.pixel_rays(w, h, cam)
        r.trace_hits(rays)
        st = r.stats()
        for k in keys:
            total[k] += st[k]
    counted = _host_form(r, cams)
    st = r.stats()
    r.close()
    _same(counted, plain, "counting against plain")
    assert st["rays"] == n * w * h
    assert {k: st[k] for k in keys} == total
    assert st["steps"] > st["rays"] and st["sphere_tests"] > 0
    assert st["exhausted"] == int((counted[0] == 0).sum())
    assert st["trace_ms"] > 0 and st["total_ms"] >= st["trace_ms"] and st["blur_ms"] == 0


# ---------------------------------------------------------------- 9. nothing else moves ----

def _sequence(r, cams, between):
    import torch
    out = []
    rects = [(0, 0, 120, 136), (120, 0, 120, 68)]

    def view_hits_call():
        if between:
            r.trace_view_hits(np.stack([cams[0], cams[2], cams[1]]))
            bufs, _ = _device_form(r, np.stack([cams[3], cams[0]]))
            torch.cuda.synchronize()

    def others(a, b):
        res = list(r.trace_screen_centred(cams[a], 0.0))
        res += list(r.trace_views(np.stack([cams[b], cams[a]]), np.zeros(2, np.float32)))
        res += list(r.trace_viewports(rects, np.stack([cams[a], cams[b]]), [0.0, 0.0]))
        return res

    out += others(1, 2)
    view_hits_call()
    out += others(0, 0)                 # rays of cams[0] run out of steps: the depth of the frames before stays where they do
    view_hits_call()
    out += others(1, 3)
    return out


def test_other_calls_are_not_disturbed():
    """a blocking frame, a batch of views (blur on) and a frame of viewports, then their repeats with other cameras, with
    trace_view_hits calls of both forms between them: bit-identical to the same sequence without, the depth that exhausted rays
    keep (the blocking call's plane, the view slots, the viewports' plane) included"""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    w, h = 240, 136
    res = []
    for between in (False, True):
        r = _renderer("plain", w, h)
        r.level_load(level_path("synth256"))
        r.set_objects(load_spheres("synth256"))
        r.set_blur_passes(1)
        if between:
            label, _, _ = r.trace_view_hits(cams[:1])
            assert (label == 0).any(), "no pixel of cams[0] runs out of steps: the depth persistence is not exercised"
        res.append(_sequence(r, cams, between))
        r.close()
    assert len(res[0]) == len(res[1]) == 18
    for i, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and (_bits(a) == _bits(b)).all(), i


# ---------------------------------------------------------------- 10. refusals ----

def test_refusals():
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    w, h, n = 40, 10, 3
    N = n * w * h
    dev = torch.device("cuda", 0)
    cams = np.tile(np.eye(4, dtype=np.float32).ravel(), (n, 1))
    t_cams = torch.from_numpy(np.concatenate([cams, cams[:1]])).to(dev)
    bufs = [torch.full((N + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
    pc = t_cams.data_ptr()
    pl, pe, pd = (b.data_ptr() + 4 * GUARD for b in bufs)
    hl, he, hd = (np.full(N, SENTINEL, np.uint32) for _ in range(3))

    def host(ctx, n_, cams_=cams, label=hl, cell=he, dist=hd):
        p = lambda a: None if a is None else a.ctypes.data
        return L.pwn_trace_view_hits(ctx, n_, p(cams_), p(label), p(cell), p(dist))

    def device(ctx, n_, c=pc, flags=0, a=pl, b=pe, d=pd):
        return L.pwn_trace_view_hits_device(ctx, n_, c, flags, a, b, d, None)

    # before a level
    nl = _renderer("plain", w, h)
    assert host(nl._ctx, n) == PWN_ENOLEVEL and device(nl._ctx, n) == PWN_ENOLEVEL
    nl.close()
    r = _level_renderer(w, h)
    ctx = r._ctx
    assert host(None, n) == PWN_EINVAL and device(None, n) == PWN_EINVAL
    assert host(ctx, n, cams_=None) == PWN_EINVAL and device(ctx, n, c=None) == PWN_EINVAL
    assert host(ctx, n, label=None) == PWN_EINVAL and device(ctx, n, a=None) == PWN_EINVAL
    for bad_n in (0, -1, 1025):
        assert host(ctx, bad_n) == PWN_EINVAL and device(ctx, bad_n) == PWN_EINVAL, bad_n
    assert device(ctx, n, flags=2) == PWN_EINVAL and device(ctx, n, flags=3) == PWN_EINVAL          # a flag other than PWN_VIEWS_HAS_W
    for off in (4, 8):                                                                                # a misaligned pointer
        assert device(ctx, n, c=pc + off) == PWN_EINVAL
        assert device(ctx, n, a=pl + off) == PWN_EINVAL
        assert device(ctx, n, b=pe + off) == PWN_EINVAL
        assert device(ctx, n, d=pd + off) == PWN_EINVAL
    # any two of the given plane ranges overlapping (16-byte aligned starts inside one another's N words)
    assert device(ctx, n, b=pl) == PWN_EINVAL and device(ctx, n, d=pl) == PWN_EINVAL and device(ctx, n, b=pd) == PWN_EINVAL
    assert device(ctx, n, b=pl + 4 * (N - 4)) == PWN_EINVAL and device(ctx, n, a=pd + 16, b=None) == PWN_EINVAL
    assert device(ctx, n, b=None, d=None) == 0                   # (and the label plane alone is in order)
    torch.cuda.synchronize()
    assert not (bufs[0][GUARD:GUARD + N] == SENTINEL).any() and (bufs[0][:GUARD] == SENTINEL).all() and (bufs[0][GUARD + N:] == SENTINEL).all()
    bufs[0].fill_(SENTINEL)
    # n x w x h > 2^28: 1024 views of 1024 x 512
    big = _renderer("plain", 1024, 512)
    big.level_load(level_path("pwnfps_level"))
    many = np.tile(np.eye(4, dtype=np.float32).ravel(), (1024, 1))
    t_many = torch.from_numpy(many).to(dev)
    assert host(big._ctx, 1024, cams_=many) == PWN_EINVAL
    assert device(big._ctx, 1024, c=t_many.data_ptr(), b=None, d=None) == PWN_EINVAL
    big.close()
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(w, h, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert host(g._ctx, n) == PWN_ENOTSUP and device(g._ctx, n) == PWN_ENOTSUP
    g.close()
    # while the context runs a row tiling
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert host(ctx, n) == PWN_EBUSY and device(ctx, n) == PWN_EBUSY
    r.tiled_shutdown()
    # every refused call left the sentinel-filled planes alone
    torch.cuda.synchronize()
    for b in bufs:
        assert (b == SENTINEL).all()
    for a in (hl, he, hd):
        assert (a == SENTINEL).all()
    assert host(ctx, n) == 0 and not (hl == SENTINEL).any() and not (he == SENTINEL).any() and not (hd == SENTINEL).any()
    r.close()
