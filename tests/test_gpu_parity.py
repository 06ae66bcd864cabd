"""Parity of the HIP path (through the C ABI) with the reference's pixels:
every golden case incl. the full BASELINE sizes (4K, 8K), bit-exact colour,
depth and work counters; strip forms; sink; error behaviour."""
import os

import numpy as np
import pytest

from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu


def _renderer(w, h):
    import pwnfps_amd
    return pwnfps_amd.Renderer(w, h)


def _fnv(oracle_lib, a):
    return oracle_lib.fnv64(a)


def test_library_is_loaded_in_tree():
    from pwnfps_amd import _lib
    assert os.path.samefile(os.path.dirname(_lib.LIB_PATH), os.path.join(os.path.dirname(GOLD), "..", "pwnfps_amd"))
    maps = open("/proc/self/maps").read()
    assert "libpwnhip.so" in maps


def test_level_loader_through_ctx():
    r = _renderer(64, 64)
    for name, key in (("pwnfps_level", "t0"), ("synth64", "synth64"), ("synth256", "synth256")):
        t = np.load(os.path.join(GOLD, "levels", name + "_tables.npz"))
        r.level_load(level_path(name))
        d, p, s = r.get_level()
        assert (d == t["data"]).all() and (p == t["pmap"]).all() and (s == t["spawn"]).all()
        r.set_objects(load_spheres(key))
        counts, idx = r.get_bins()
        assert (counts == t["bin_counts"]).all() and (idx == t["bin_idx"]).all()
    r.close()


def test_all_golden_cases(oracle_lib, cases):
    """pre-blur, post-blur, depth hashes and counters for every case, at every
    BASELINE resolution up to 7680x4320."""
    by_size = {}
    for c in cases:
        by_size.setdefault((c["w"], c["h"]), []).append(c)
    for (w, h), cs in sorted(by_size.items()):
        r = _renderer(w, h)
        for c in cs:
            r.level_load(level_path(c["level"]))
            r.set_objects(load_spheres(c["spheres"]))
            cam = np.array(c["cam"], np.float32)
            r.set_blur_passes(0)
            r.set_counters("steps" in c)
            pre, z = r.trace_screen_centred(cam, c["sec"])
            st = r.stats()
            # depth of never-hit pixels keeps its previous value (trace.h:677); the
            # goldens start from zero depth, and a fresh context does too, but this
            # context has rendered other cases: compare depth only where the golden
            # frame wrote it, i.e. through a fresh context when any ray exhausts
            assert _fnv(oracle_lib, pre) == c["pre"], c["name"]
            if c.get("exhausted", 0) == 0 and "exhausted" in c:
                assert _fnv(oracle_lib, z) == c["z"], c["name"]
            if "steps" in c:
                got = (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])
                want = (c["rays"], c["steps"], c["portals"], c["sphere_tests"], c["exhausted"])
                assert got == want, c["name"]
            r.set_counters(False)
            if c.get("exhausted", 1) > 0:
                # (cases without counters may exhaust too) stale depth from the previous case feeds the blur at the never-hit
                # pixels, as in the reference; these cases are checked through a
                # fresh context in test_depth_with_exhausted_rays_fresh_context
                r.close()
                r = _renderer(w, h)
                continue
            r.set_blur_passes(1)
            post, z2 = r.trace_screen_centred(cam, c["sec"])
            assert _fnv(oracle_lib, post) == c["post"], c["name"]
        r.close()


def test_golden_cases_through_the_general_four_lane_variant(oracle_lib, cases, monkeypatch):
    """The goldens' cameras carry no w components and take the 3-lane specialisation.  The general (HAS_W)
    kernel variants are only reached by unusual cameras -- and were the ones with the layout-dependent
    miscompile of round 1 (dev_math.h) -- so the fixed goldens are also rendered through them
    (PWN_DBG_FORCE_HASW, read when a context is created): both schedulers, sizes up to 4K."""
    monkeypatch.setenv("PWN_DBG_FORCE_HASW", "1")
    import pwnfps_amd
    names = ("level_spawn_320x240", "level_pose1_1280x720", "synth64_cam0_1920x1080", "level_spawn_3840x2160", "synth256_cam1_480x272")
    picked = [c for c in cases if c["name"] in names]
    assert len(picked) >= 3
    for sched in ("units", "refill"):
        for c in picked:
            r = _renderer(c["w"], c["h"])
            r.set_scheduler(sched)
            r.level_load(level_path(c["level"]))
            r.set_objects(load_spheres(c["spheres"]))
            post, z = r.trace_screen_centred(np.array(c["cam"], np.float32), c["sec"])
            assert _fnv(oracle_lib, post) == c["post"], (sched, c["name"])
            assert _fnv(oracle_lib, z) == c["z"], (sched, c["name"])
            r.close()


def test_depth_with_exhausted_rays_fresh_context(oracle_lib, cases):
    cs = [c for c in cases if c.get("exhausted", 0) > 0 or "exhausted" not in c]
    assert cs
    for c in cs:
        r = _renderer(c["w"], c["h"])
        r.level_load(level_path(c["level"]))
        r.set_objects(load_spheres(c["spheres"]))
        post, z = r.trace_screen_centred(np.array(c["cam"], np.float32), c["sec"])
        assert _fnv(oracle_lib, post) == c["post"], c["name"]
        assert _fnv(oracle_lib, z) == c["z"], c["name"]
        r.close()


def test_raw_frames_and_strips():
    raw = np.load(os.path.join(GOLD, "raw_320x240.npz"))
    r = _renderer(320, 240)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    cam = np.eye(4, dtype=np.float32)
    cam[3, :3] = (9.5, 0.5, 4.5)
    r.set_blur_passes(0)
    pre, z = r.trace_screen_centred(cam, 0.0)
    assert (pre == raw["pre"]).all()
    assert (z.view(np.uint32) == raw["z"].view(np.uint32)).all()
    r.set_blur_passes(1)
    post, _ = r.trace_screen_centred(cam, 0.0)
    assert (post == raw["post"]).all()
    r.close()
    s = np.load(os.path.join(GOLD, "strips.npz"))
    r = _renderer(3840, 2160)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    y0, y1 = (int(v) for v in s["c4_rows"])
    r.set_blur_passes(0)
    pre, z = r.trace_screen_centred(cam, 0.0)
    assert (pre[y0:y1] == s["c4_pre"]).all() and (z[y0:y1].view(np.uint32) == s["c4_z"].view(np.uint32)).all()
    r.set_blur_passes(1)
    post, _ = r.trace_screen_centred(cam, 0.0)
    assert (post[y0:y1] == s["c4_post"]).all()
    r.close()


def test_ragged_large_frames_vs_oracle(oracle_lib):
    """Frames long enough for the wave scheduler to draw its tickets in PAIRS (>= 16 units per resident wave, the
    4K and 8K goldens' regime) at sizes that are multiples of nothing: partial units at the right and bottom edges,
    queues of unequal length, a last pair whose second ticket is past the end.  Every pixel and depth against the
    oracle, twice through the same context (the second launch uses the ticket set the first one cleared); with the
    blur where the width is a multiple of 4 (the library takes POSTPROC_BLUR only then: 16-byte stores, screen.h:88)."""
    import pwnfps_amd
    from oracle import Oracle
    O = Oracle()
    O.load_level(level_path("pwnfps_level"))
    O.set_spheres(load_spheres("t0"))
    for (w, h), ang in (((3001, 2003), 0.4), ((4099, 1301), -1.1), ((3004, 2002), 2.3)):
        cam = pwnfps_amd.spawn_camera((9, 4), ang_y=ang, ang_x=0.05)
        ob0, oz0 = O.render(w, h, cam, sec=0.3, blur=0)
        r = _renderer(w, h)
        r.level_load(level_path("pwnfps_level"))
        r.set_objects(load_spheres("t0"))
        for rep in range(2):
            r.set_blur_passes(0)
            sb, zb = r.trace_screen_centred(cam, 0.3)
            assert (sb == ob0).all() and (zb.view(np.uint32) == oz0.view(np.uint32)).all(), (w, h, rep)
        if w % 4 == 0:
            ob1, _ = O.render(w, h, cam, sec=0.3, blur=1)
            r.set_blur_passes(1)
            sb, _ = r.trace_screen_centred(cam, 0.3)
            assert (sb == ob1).all(), (w, h)
        r.close()


def test_extreme_aspect_frames_vs_oracle(oracle_lib):
    """The widest and the tallest frame pwn_init takes (32768), one unit high / one unit wide, and widths whose units per
    row are 1, a power of two, and neither: the kernel turns a unit number into (row, column) with a reciprocal the host
    computes per launch (launch_plan.h pwn_unit_div_magic; frames one unit wide divide), the blur picks its tile shape by
    the width, and the pixel index is 32-bit arithmetic.  Every pixel and depth against the oracle, blur included."""
    import pwnfps_amd
    from oracle import Oracle
    O = Oracle()
    O.load_level(level_path("pwnfps_level"))
    O.set_spheres(load_spheres("t0"))
    for (w, h), ang in (((32768, 4), 0.3), ((4, 32768), 1.9), ((16, 2048), -0.7), ((2048, 12), 2.6), ((2064, 20), 0.9), ((4096, 36), -2.2)):
        cam = pwnfps_amd.spawn_camera((9, 4), ang_y=ang, ang_x=-0.04)
        r = _renderer(w, h)
        r.level_load(level_path("pwnfps_level"))
        r.set_objects(load_spheres("t0"))
        for blur in (0, 1):
            ob, oz = O.render(w, h, cam, sec=0.7, blur=blur)
            r.set_blur_passes(blur)
            sb, zb = r.trace_screen_centred(cam, 0.7)
            assert (sb == ob).all(), (w, h, blur, int((sb != ob).sum()))
            assert (zb.view(np.uint32) == oz.view(np.uint32)).all(), (w, h, blur)
        r.close()


def test_campaign(oracle_lib):
    c = np.load(os.path.join(GOLD, "campaign.npz"))
    ctxs = {}
    for i in range(len(c["cams"])):
        w, h = (int(v) for v in c["size"][i])
        r = _renderer(w, h)        # fresh: depth starts at zero like the goldens
        r.level_load(level_path(str(c["level"][i])))
        ns = int(c["hashes"][i][3])
        r.set_objects(c["spheres"][i][:ns])
        r.set_blur_passes(0)
        pre, z = r.trace_screen_centred(c["cams"][i], float(c["sec"][i]))
        r.set_blur_passes(1)
        post, _ = r.trace_screen_centred(c["cams"][i], float(c["sec"][i]))
        assert [_fnv(oracle_lib, pre), _fnv(oracle_lib, post), _fnv(oracle_lib, z)] == list(c["hashes"][i][:3]), i
        r.close()


def test_random_scenes_vs_oracle(oracle_lib):
    """Fresh random scenes (not in the goldens) against the oracle, incl.
    cameras with w components and odd frame sizes."""
    rng = np.random.default_rng(4242)
    for lvl in ("pwnfps_level", "synth64", "synth256"):
        O = oracle_lib.Oracle()
        O.load_level(level_path(lvl))
        data, _, _ = O.get_level()
        free = [(x, z) for z in range(64) for x in range(64) if chr(data[z, x]) in ';$"#&><,^']
        for it in range(14):
            # (frames one and two units wide: the kernel's unit -> (row, column) division has a path of its own for those)
            w, h = [(256, 128), (132, 75), (64, 8), (36, 33), (520, 260), (16, 24), (12, 40)][it % 7]
            x, z = free[rng.integers(len(free))]
            ay, ax = rng.uniform(0, 6.28), rng.uniform(-1.2, 1.2)
            cy, sy, cx, sx = np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
            cam = np.eye(4, dtype=np.float32)
            cam[:3, :3] = (np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])).astype(np.float32)
            cam[3, :3] = (x + rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95), z + rng.uniform(0.05, 0.95))
            if it % 4 == 3:
                cam[:, 3] = (0.03, -0.01, 0.05, 0.8)
            sph = np.zeros(int(rng.integers(0, 30)), oracle_lib.SPHERE_DTYPE)
            for i in range(len(sph)):
                sph[i] = (rng.uniform(0.03, 0.4), rng.choice([0.0, 0.3, 0.6]), np.clip(x + rng.uniform(-1, 2), 0.6, 62.4),
                          rng.uniform(0.1, 1.2), np.clip(z + rng.uniform(-1, 2), 0.6, 62.4), *rng.uniform(0, 1.2, 3))
            sec = float(np.float32(rng.uniform(0, 50)))
            O.set_spheres(sph)
            r = _renderer(w, h)
            r.level_load(level_path(lvl))
            r.set_objects(sph)
            blur = 1 if w % 4 == 0 else 0
            r.set_blur_passes(blur)
            a, za = r.trace_screen_centred(cam, sec)
            b, zb = O.render(w, h, cam, sec=sec, blur=blur)
            assert (a == b).all(), (lvl, it, int((a != b).sum()))
            assert (za.view(np.uint32) == zb.view(np.uint32)).all(), (lvl, it)
            r.close()


def test_strip_forms_equal_full_frame(oracle_lib, cases):
    """pwn_trace_rows_device / pwn_blur_rows_device on uneven strips reproduce
    the full frame (the multi-GPU building blocks), incl. stale-depth rows."""
    import torch
    c = next(x for x in cases if x["name"] == "level_pose1_1280x720")
    w, h = c["w"], c["h"]
    r = _renderer(w, h)
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    cam = np.array(c["cam"], np.float32)
    dev = torch.device("cuda:0")
    pre = torch.zeros((h, w), dtype=torch.int32, device=dev)
    z = torch.zeros((h, w), dtype=torch.float32, device=dev)
    out = torch.zeros((h, w), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cuts = [0, 8, 13, 300, 301, 640, h]
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        r.trace_rows_device(cam, c["sec"], y0, y1, pre.data_ptr(), z.data_ptr(), stream)
    r.trace_rows_device(cam, c["sec"], 5, 5, pre.data_ptr(), z.data_ptr(), stream)   # empty strip is a no-op
    torch.cuda.synchronize()
    assert _fnv(oracle_lib, pre.cpu().numpy()) == c["pre"]
    assert _fnv(oracle_lib, z.cpu().numpy()) == c["z"]
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        r.blur_rows_device(y0, y1, pre.data_ptr(), z.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert _fnv(oracle_lib, out.cpu().numpy()) == c["post"]
    r.close()


def test_single_rank_row_tiled_frame(oracle_lib, cases):
    """pwnfps_amd/dist.py's restatement of the tiling choreography over the HIP strip kernels
    (torch tensors, torch's stream), one rank: two frames in flight, alternating poses."""
    import torch
    from pwnfps_amd.dist import HipStripBackend, TiledFrames
    c = next(x for x in cases if x["name"] == "level_pose2_320x240")
    r = _renderer(c["w"], c["h"])
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    fr = TiledFrames(c["w"], c["h"], HipStripBackend(r), torch.device("cuda:0"), rank=0, world=1)
    cams = [np.array(c["cam"], np.float32).reshape(4, 4).copy() for _ in range(2)]
    cams[1][3, 0] += 0.25
    want = []
    for cam in cams:
        sb, _ = r.trace_screen_centred(cam, c["sec"])
        want.append(_fnv(oracle_lib, sb))
    assert want[0] == c["post"] and want[1] != want[0]
    got = []
    for i in range(6):
        fr.submit(cams[i & 1], c["sec"])
        if i >= 1:
            o, redone = fr.wait()
            torch.cuda.synchronize()
            got.append(_fnv(oracle_lib, fr.to_host(o)))
    o, _ = fr.wait()
    torch.cuda.synchronize()
    got.append(_fnv(oracle_lib, fr.to_host(o)))
    assert got == [want[i & 1] for i in range(6)]
    r.close()


def test_upscale_sink(oracle_lib):
    k = np.load(os.path.join(GOLD, "helpers_kat.npz"))
    src = k["up_src"]
    r = _renderer(src.shape[1], src.shape[0])
    assert (r.screen_upscale(src, 3, pitch_bytes=k["up3"].shape[1] * 4) == k["up3"]).all()
    assert (r.screen_upscale(src, 1) == k["up1"]).all()
    r.close()
    # the shipped default: 320x200 x3 into a 960x600 surface (defs.h:11-15), last frame on the device
    O = oracle_lib.Oracle()
    r = _renderer(320, 200)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    cam = np.eye(4, dtype=np.float32)
    cam[3, :3] = (9.5, 0.5, 4.5)
    sb, _ = r.trace_screen_centred(cam, 0.0)
    big = r.screen_upscale(None, 3)
    assert big.shape == (600, 960) and (big == O.upscale(sb, 3)).all()
    r.close()


def test_stale_depth_semantics(oracle_lib):
    """zbuf keeps its previous value where the primary ray exhausts maxsteps
    (trace.h:677): second frame from another pose leaves those pixels alone."""
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy"))
    sph = load_spheres("synth256")
    O = oracle_lib.Oracle()
    O.load_level(level_path("synth256"))
    O.set_spheres(sph)
    w, h = 480, 272
    r = _renderer(w, h)
    r.level_load(level_path("synth256"))
    r.set_objects(sph)
    r.set_blur_passes(0)
    _, z1 = r.trace_screen_centred(cams[1], 0.0)
    a, z2 = r.trace_screen_centred(cams[0], 0.0)
    sb, zb, st = O.trace_rows(w, h, 0, h, cams[1])
    sb, zb, st = O.trace_rows(w, h, 0, h, cams[0], sb=sb, zb=zb)
    assert st.exhausted > 0
    assert (a == sb).all() and (z2.view(np.uint32) == zb.view(np.uint32)).all()
    r.close()


def test_errors():
    import pwnfps_amd
    from pwnfps_amd import PwnError
    r = _renderer(322, 100)
    cam = np.eye(4, dtype=np.float32)
    with pytest.raises(PwnError) as e:       # blur needs w % 4 == 0 (screen.h:88)
        r.trace_screen_centred(cam, 0.0)
    assert e.value.code == -1
    r.set_blur_passes(0)
    with pytest.raises(PwnError) as e:       # no level yet
        r.trace_screen_centred(cam, 0.0)
    assert e.value.code == -6
    with pytest.raises(PwnError) as e:
        r.level_load("/nonexistent/level.txt")
    assert e.value.code == -4
    r.level_load(level_path("pwnfps_level"))
    big = np.zeros(5000, pwnfps_amd.SPHERE_DTYPE)
    big["r"] = 0.1; big["x"] = 9.5; big["y"] = 0.3; big["z"] = 5.5
    with pytest.raises(PwnError) as e:       # beyond the LDS budget
        r.set_objects(big)
    assert e.value.code == -7
    r.set_objects(load_spheres("t0"))        # the previous good state still renders
    r.trace_screen_centred(cam, 0.0)
    with pytest.raises(PwnError):
        pwnfps_amd.Renderer(0, 10)
    with pytest.raises(PwnError):
        pwnfps_amd.Renderer(64, 64, device=99)
    r.close()


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLD), "..", "oracle", "_ref", "libpwnref_tab.so")),
                    reason="oracle/_ref not shipped")
def test_full_size_vs_compiled_reference():
    """A pose that is in no fixture, at 3840x2160, against the reference's own
    code (table build, so the host CPU's rcpps does not matter)."""
    import refharness
    R = refharness.RefHarness("tab")
    R.load_level(level_path("pwnfps_level"))
    sph = load_spheres("t0")
    R.set_spheres(sph)
    cam = np.eye(4, dtype=np.float32)
    ay = 3.9
    cam[0, 0], cam[0, 2], cam[2, 0], cam[2, 2] = np.cos(ay), np.sin(ay), -np.sin(ay), np.cos(ay)
    cam[3, :3] = (12.4, 0.55, 14.3)
    want, wz = R.render(3840, 2160, cam, sec=7.5, blur=1)
    r = _renderer(3840, 2160)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(sph)
    got, gz = r.trace_screen_centred(cam, 7.5)
    assert (got == want).all() and (gz.view(np.uint32) == wz.view(np.uint32)).all()
    r.close()



def test_edge_scenes_vs_oracle(oracle_lib):
    """Inputs at the edges of the domain (tests/edge_scenes.py), each against the
    oracle bit for bit; the oracle itself is pinned on the same scenes against the
    compiled reference by tests/test_oracle_vs_ref.py::test_edge_scenes."""
    import edge_scenes
    for sc in edge_scenes.scenes(oracle_lib.SPHERE_DTYPE):
        O = oracle_lib.Oracle()
        r = _renderer(sc.w, sc.h)
        if sc.text is None:
            O.load_level(level_path("pwnfps_level"))
            r.level_load(level_path("pwnfps_level"))
        else:
            O.load_level_text(sc.text)
            r.level_load_text(sc.text)
        O.set_spheres(sc.spheres)
        r.set_objects(sc.spheres)
        blur = 1 if sc.w % 4 == 0 else 0
        r.set_blur_passes(blur)
        a, za = r.trace_screen_centred(sc.cam, sc.sec)
        b, zb = O.render(sc.w, sc.h, sc.cam, sec=sc.sec, blur=blur)
        assert (a == b).all(), (sc.name, sc.w, sc.h, int((a != b).sum()))
        assert (za.view(np.uint32) == zb.view(np.uint32)).all(), (sc.name, sc.w, sc.h)
        r.close()


def test_bounded_blur_reports_taps_outside_the_available_rows(oracle_lib, cases):
    """pwn_blur_rows_device_bounded: with enough rows available the strip equals the plain
    strip and the counter stays 0; with too few it counts.  (The multi-GPU halo exchange
    relies on exactly this to stay bit-exact.)"""
    import torch
    c = next(x for x in cases if x["name"] == "level_pose1_1280x720")
    w, h = c["w"], c["h"]
    r = _renderer(w, h)
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    cam = np.array(c["cam"], np.float32)
    dev = torch.device("cuda:0")
    pre = torch.zeros((h, w), dtype=torch.int32, device=dev)
    z = torch.zeros((h, w), dtype=torch.float32, device=dev)
    ref = torch.zeros((h, w), dtype=torch.int32, device=dev)
    out = torch.zeros((h, w), dtype=torch.int32, device=dev)
    miss = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    r.trace_rows_device(cam, c["sec"], 0, h, pre.data_ptr(), z.data_ptr(), s)
    r.blur_rows_device(0, h, pre.data_ptr(), z.data_ptr(), ref.data_ptr(), s)
    torch.cuda.synchronize()
    assert _fnv(oracle_lib, ref.cpu().numpy()) == c["post"]
    zmax = float((z[240:480] - 1.0).abs().max())
    need = int(np.floor(np.float32(0.002 * h) * zmax)) + 1
    # (a) a halo that covers the deepest pixel of the strip: exact, no miss, even with garbage outside it
    lo, hi = max(240 - need, 0), min(480 + need, h)
    poisoned = pre.clone()
    poisoned[:lo] = 0x5EADBEEF
    poisoned[hi:] = 0x5EADBEEF
    r.blur_rows_device_bounded(240, 480, poisoned.data_ptr(), z.data_ptr(), out.data_ptr(), lo, hi, miss.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(miss.item()) == 0
    assert (out[240:480] == ref[240:480]).all()
    # (b) only the strip itself: this scene's taps do leave it
    assert need > 1
    r.blur_rows_device_bounded(240, 480, pre.data_ptr(), z.data_ptr(), out.data_ptr(), 240, 480, miss.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(miss.item()) > 0
    r.close()


def test_sphere_uploads_between_launches_in_flight(oracle_lib):
    """level_prepare_render every frame (main.c:95) with the strip forms: six frames with six
    different sphere sets are queued back to back on the caller's stream with no synchronisation
    by the caller; an upload waits for the launch that still reads the tables (pwn_launch.cpp, pwn_tables.cpp).
    (A fully asynchronous double-buffered upload was measured: the cross-stream event waits cost
    7 % of a 4K frame, the blocking form 0.3 %.)"""
    import torch
    w, h = 1280, 720
    r = _renderer(w, h)
    r.level_load(level_path("pwnfps_level"))
    base = load_spheres("t0")
    _, _, spawn = r.get_level()
    import pwnfps_amd
    cam = pwnfps_amd.spawn_camera(spawn, ang_y=0.2)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    sets, pres, zs = [], [], []
    for i in range(6):
        sph = base.copy()
        sph["y"] += np.float32(0.05 * i)
        sph["x"] += np.float32(0.11 * (i % 3))
        if i == 4:
            sph = np.concatenate([sph, sph])[:23]      # another table size: the copy is re-allocated
        sets.append(sph)
        pres.append(torch.zeros((h, w), dtype=torch.int32, device=dev))
        zs.append(torch.zeros((h, w), dtype=torch.float32, device=dev))
    for i in range(6):
        r.set_objects(sets[i])
        r.trace_rows_device(cam, 0.5, 0, h, pres[i].data_ptr(), zs[i].data_ptr(), s)
    torch.cuda.synchronize()
    O = oracle_lib.Oracle()
    O.load_level(level_path("pwnfps_level"))
    for i in range(6):
        O.set_spheres(sets[i])
        b, zb = O.render(w, h, cam, sec=0.5, blur=0)
        assert (pres[i].cpu().numpy().view(np.uint32) == b).all(), i
        assert (zs[i].cpu().numpy().view(np.uint32) == zb.view(np.uint32)).all(), i
    r.close()


def test_two_contexts_interleaved(oracle_lib, cases):
    """Two live contexts of different sizes and levels, frames interleaved: nothing is shared
    between contexts but the per-device launch attributes."""
    a = next(x for x in cases if x["name"] == "level_pose1_320x240")
    b = next(x for x in cases if x["name"] == "synth64_cam1_1920x1080")
    ra, rb = _renderer(a["w"], a["h"]), _renderer(b["w"], b["h"])
    ra.level_load(level_path(a["level"])); ra.set_objects(load_spheres(a["spheres"]))
    rb.level_load(level_path(b["level"])); rb.set_objects(load_spheres(b["spheres"]))
    for _ in range(3):
        fa, _ = ra.trace_screen_centred(np.array(a["cam"], np.float32), a["sec"])
        fb, _ = rb.trace_screen_centred(np.array(b["cam"], np.float32), b["sec"])
        assert _fnv(oracle_lib, fa) == a["post"]
        assert _fnv(oracle_lib, fb) == b["post"]
    ra.close(); rb.close()


def test_wave_level_counters_are_consistent(cases):
    """pwn_stats.wave_steps / wave_paths (the divergence profile of the walk loop): bounded by
    the lane-level counters they summarise, and the same from run to run."""
    c = next(x for x in cases if x["name"] == "level_spawn_1280x720")
    r = _renderer(c["w"], c["h"])
    r.level_load(level_path(c["level"]))
    r.set_objects(load_spheres(c["spheres"]))
    r.set_blur_passes(0)
    r.set_counters(True)
    cam = np.array(c["cam"], np.float32)
    r.trace_screen_centred(cam, c["sec"], want_z=False)
    st = r.stats()
    assert (st["rays"], st["steps"], st["portals"]) == (c["rays"], c["steps"], c["portals"])
    ws, wp = st["wave_steps"], st["wave_paths"]
    assert st["steps"] / 64.0 <= ws <= st["steps"]             # 1..64 lanes per wave iteration
    assert all(0 <= v <= ws for v in wp[:7])
    assert wp[1] > 0.5 * ws                                     # most iterations walk a room cell
    assert wp[5] <= st["portals"] and wp[5] * 64 >= st["portals"]
    assert wp[0] * 64 >= 1 and wp[7] <= st["sphere_tests"]
    assert wp[4] > 0 and wp[2] > 0 and wp[3] > 0 and wp[6] > 0  # level.txt has ramps, fog, two-level rooms, walls
    r.trace_screen_centred(cam, c["sec"], want_z=False)
    st2 = r.stats()
    assert st2["wave_steps"] == ws and st2["wave_paths"] == wp
    r.set_counters(False)
    r.trace_screen_centred(cam, c["sec"], want_z=False)
    r.close()


def test_blur_tap_coordinates_with_hostile_depths(oracle_lib):
    """screen.h:101-106 turns a float tap coordinate into an int with cvttss2si (INT_MIN for NaN and
    anything outside int32) and clamps it; the kernel does it with a saturating convert and one
    median-of-three (post_kernels.hip blur_coord).  Depths chosen so that taps are NaN, +-inf, beyond
    +-2^31 and just inside it, on a random frame; the oracle's blur is the reference's loop."""
    import torch
    w, h = 256, 96
    rng = np.random.default_rng(11)
    pre = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
    z = (1.0 + rng.standard_normal((h, w)) * 8.0).astype(np.float32)
    hostile = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1.2e10, -1.2e10, 2.4e10, 1e30, -1e30, 1e38, -1e38,
                        1.1184e10, -1.1184e10, 5.5e9, 0.0, -0.0, 1.0, 1e-40], np.float32)
    idx = rng.integers(0, h * w, 6000)
    z.reshape(-1)[idx] = hostile[rng.integers(0, len(hostile), len(idx))]
    O = oracle_lib.Oracle()
    want = O.blur_rows(0, h, pre, z)
    r = _renderer(w, h)
    dev = torch.device("cuda:0")
    d_pre = torch.from_numpy(pre.view(np.int32)).to(dev)
    d_z = torch.from_numpy(z).to(dev)
    d_out = torch.zeros((h, w), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    r.blur_rows_device(0, h, d_pre.data_ptr(), d_z.data_ptr(), d_out.data_ptr(), s)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    assert (got == want).all(), int((got != want).sum())
    r.close()


def test_far_start_scenes(oracle_lib):
    """A bounced ray can start its next segment 10^13 cells away (horizon rays of axis-aligned cameras); the
    walk packs cell numbers in 16 bits and has to keep such a start outside the grid.  Frames, depths and the
    path counters (rays, steps, portals, sphere tests, exhausted) against the oracle, both schedulers."""
    k = np.load(os.path.join(GOLD, "far_starts.npz"))
    O = oracle_lib.Oracle()
    for i in range(len(k["names"])):
        text, cam, sph, sec = str(k["text_%d" % i]), k["cam_%d" % i], k["sph_%d" % i], float(k["sec_%d" % i])
        w, h = (int(v) for v in k["wh_%d" % i])
        O.load_level_text(text)
        O.set_spheres(sph)
        b, zb, ost = O.render(w, h, cam, sec=sec, blur=0, stats=True)
        for sched in ("units", "refill"):
            for counters in (False, True):
                r = _renderer(w, h)
                r.level_load_text(text)
                r.set_objects(sph)
                r.set_blur_passes(0)
                r.set_scheduler(sched)
                r.set_counters(counters)
                a, za = r.trace_screen_centred(cam, sec)
                assert (a == b).all(), (k["names"][i], sched, counters, int((a != b).sum()))
                assert (za.view(np.uint32) == zb.view(np.uint32)).all(), (k["names"][i], sched)
                if counters:
                    st = r.stats()
                    assert (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"]) == \
                        (ost.rays, ost.steps, ost.portals, ost.sphere_tests, ost.exhausted), (k["names"][i], sched)
                r.close()

