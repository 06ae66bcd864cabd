"""Sphere tables that outgrow LDS are traced from device memory (tables.h PWN_LF_GLOBAL, up to PWN_OBJ_MAX spheres): every call
path, bit for bit against the oracle, on the scenes of tests/big_scenes.py -- and the scenes that always loaded, sent through the
same kernels by PWN_SPHERE_LISTS=global, against the compiled reference's goldens.  Both lane variants of the kernels throughout
(PWN_DBG_FORCE_HASW)."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import big_scenes as BS
import hit_chain as HC
from conftest import ROOT, level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_ETOOBIG = -7
VARIANTS = {"plain": {}, "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}}
W, H = 160, 120


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


def _renderer(w, h, env=None, devices=None):
    import pwnfps_amd
    with _env(**(env or {})):
        return pwnfps_amd.Renderer(w, h, devices=devices)


def _scene_renderer(sc, w=W, h=H, variant="plain", blur=0):
    r = _renderer(w, h, VARIANTS[variant])
    r.level_load(level_path(sc.level))
    r.set_objects(sc.spheres)
    r.set_blur_passes(blur)
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_frames = {}


def _oracle_frame(oracle_lib, sc, ci, w, h, blur, level=None):
    """(colour, depth bits, stats) of camera ci of the scene's spawn: computed once, shared"""
    key = (sc.name, len(sc.spheres), ci, w, h, blur, level)
    if key not in _frames:
        if level is None:
            O = BS.oracle_for(sc, oracle_lib)
        else:
            O = oracle_lib.Oracle()
            O.load_level(level_path(level))
            O.set_spheres(sc.spheres)
        cam = BS.cameras(sc.spawn, oracle_lib)[ci]
        sb, zb, st = O.render(w, h, cam, sec=0.0, blur=blur, stats=True)
        _frames[key] = (sb, _bits(zb).copy(), (st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted))
    return _frames[key]


def _same(got, want, what):
    sb, zb = got
    assert (sb == want[0]).all(), (what, "colour", int((sb != want[0]).sum()))
    assert (_bits(zb) == want[1]).all(), (what, "depth", int((_bits(zb) != want[1]).sum()))


def _counters(r):
    st = r.stats()
    return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])


def _scenes5(oracle_lib):
    under, over = BS.one_over_pair(oracle_lib)
    return {"swarm_near": BS.scene("swarm_near", oracle_lib), "swarm_all": BS.scene("swarm_all", oracle_lib),
            "fat": BS.scene("fat", oracle_lib), "one_over_k": under, "one_over": over}


# ---------------------------------------------------------------- 1. the scenes that always loaded, through the new kernels ----

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", [(320, 240), (480, 272)])
def test_golden_cases_through_the_global_form(oracle_lib, cases, size, variant):
    """every golden case of the size: pre, post and depth hashes and the five counters with PWN_SPHERE_LISTS=global (form 2); the
    same context without the variable says form 0 or 1"""
    picked = [c for c in cases if (c["w"], c["h"]) == size]
    assert len(picked) >= 6
    env = dict(VARIANTS[variant])
    for c in picked:
        for forced in (True, False):
            r = _renderer(c["w"], c["h"], dict(env, PWN_SPHERE_LISTS="global") if forced else env)      # fresh: depth starts at zero like the goldens
            r.level_load(level_path(c["level"]))
            r.set_objects(load_spheres(c["spheres"]))
            form = r.sphere_tables()["form"]
            if not forced:
                assert form in (0, 1), (c["name"], form)
                r.close()
                continue
            assert form == 2, (c["name"], form)
            cam = np.array(c["cam"], np.float32)
            r.set_blur_passes(0)
            r.set_counters(True)
            pre, z = r.trace_screen_centred(cam, c["sec"])
            got = _counters(r)
            assert oracle_lib.fnv64(pre) == c["pre"], c["name"]
            assert oracle_lib.fnv64(z) == c["z"], c["name"]
            assert got == (c["rays"], c["steps"], c["portals"], c["sphere_tests"], c["exhausted"]), c["name"]
            r.set_counters(False)
            r.set_blur_passes(1)
            post, z = r.trace_screen_centred(cam, c["sec"])
            assert oracle_lib.fnv64(post) == c["post"], c["name"]
            assert oracle_lib.fnv64(z) == c["z"], c["name"]
            r.close()


# ---------------------------------------------------------------- 2. the big scenes against the oracle ----

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["swarm_near", "swarm_all", "fat", "one_over_k", "one_over"])
def test_big_scene_frames_and_counters(oracle_lib, name, variant):
    """three cameras: colour and depth without blur at 160 x 120, counting and not; the counters; with blur at 320 x 240"""
    sc = _scenes5(oracle_lib)[name]
    r = _scene_renderer(sc, W, H, variant, blur=0)
    assert (r.sphere_tables()["form"] == 2) == (name != "one_over_k")          # (the first k of one_over still load on chip)
    for ci, cam in enumerate(BS.cameras(sc.spawn, oracle_lib)):
        want = _oracle_frame(oracle_lib, sc, ci, W, H, 0)
        assert want[2][4] == 0                       # no ray runs out of steps: every depth is this frame's
        _same(r.trace_screen_centred(cam, 0.0), want, (name, variant, ci))
        r.set_counters(True)
        _same(r.trace_screen_centred(cam, 0.0), want, (name, variant, ci, "counting"))
        assert _counters(r) == want[2], (name, variant, ci)
        r.set_counters(False)
    r.close()
    r = _scene_renderer(sc, 320, 240, variant, blur=1)
    for ci, cam in enumerate(BS.cameras(sc.spawn, oracle_lib)):
        _same(r.trace_screen_centred(cam, 0.0), _oracle_frame(oracle_lib, sc, ci, 320, 240, 1), (name, variant, ci, "blur"))
    r.close()


# ---------------------------------------------------------------- 3. rays and hits ----

@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rays_reproduce_the_frame(oracle_lib, variant):
    """swarm_all: pwn_trace_rays of a 64 x 48 frame's pwn_pixel_rays = the blocking call's pre-blur colour and depth"""
    import pwnfps_amd
    sc = BS.scene("swarm_all", oracle_lib)
    w, h = 64, 48
    r = _scene_renderer(sc, w, h, variant, blur=0)
    for ci, cam in enumerate(BS.cameras(sc.spawn, oracle_lib)):
        sb, zb = r.trace_screen_centred(cam, 0.0)
        _same((sb, zb), _oracle_frame(oracle_lib, sc, ci, w, h, 0), (variant, ci))
        rays, seeds, xy = pwnfps_amd.pixel_rays(w, h, cam)
        col, z = r.trace_rays(rays, seeds, 0.0)
        assert (col == sb[xy[:, 1], xy[:, 0]]).all() and (_bits(z) == _bits(zb)[xy[:, 1], xy[:, 0]]).all(), (variant, ci)
    r.close()


_hit_refs = {}


def _hit_ref(oracle_lib, sc, ci):
    key = (sc.name, ci)
    if key not in _hit_refs:
        cam = BS.cameras(sc.spawn, oracle_lib)[ci]
        _hit_refs[key] = HC.Reader(BS.oracle_for(sc, oracle_lib)).pixels(32, 24, cam, HC.all_pixels(32, 24))
    return _hit_refs[key]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["swarm_all", "fat"])
def test_hits_equal_the_reader(oracle_lib, name, variant):
    """pwn_trace_hits of a 32 x 24 frame, host form and device form: every field of every record as hit_chain reads it off the
    oracle; swarm_all: objects >= 2048 among them (an index, where the on-chip lists hold 16-bit offsets)"""
    import torch
    import pwnfps_amd
    sc = BS.scene(name, oracle_lib)
    r = _scene_renderer(sc, 8, 8, variant, blur=0)
    assert r.sphere_tables()["form"] == 2
    high = 0
    for ci, cam in enumerate(BS.cameras(sc.spawn, oracle_lib)):
        ref = _hit_ref(oracle_lib, sc, ci)
        rays, _, xy = pwnfps_amd.pixel_rays(32, 24, cam)
        assert (xy == HC.all_pixels(32, 24)).all()
        hits = r.trace_hits(rays)
        bad = HC.mismatches(hits, ref.want, ref.cmp_dy)
        assert len(bad) == 0, (name, variant, ci, len(bad), [(int(i), hits[i].tolist(), ref.want[i].tolist()) for i in bad[:3]])
        d_rays = torch.from_numpy(rays).cuda()
        d_hits = torch.zeros((len(rays), 12), dtype=torch.int32, device=d_rays.device)
        r.trace_hits_device(d_rays, d_hits)
        torch.cuda.synchronize()
        dev = d_hits.cpu().numpy().view(HC.HIT_DTYPE).reshape(-1)
        assert dev.tobytes() == hits.tobytes(), (name, variant, ci)
        high += int((hits["object"] >= 2048).sum())
    if name == "swarm_all":
        assert high >= 1
    r.close()


# ---------------------------------------------------------------- 4. views ----

@pytest.mark.parametrize("variant", list(VARIANTS))
def test_views_equal_blocking_calls(oracle_lib, variant):
    sc = BS.scene("swarm_near", oracle_lib)
    r = _scene_renderer(sc, W, H, variant, blur=1)
    cams = BS.cameras(sc.spawn, oracle_lib)
    vs, vz = r.trace_views(np.stack(cams), np.zeros(3, np.float32))
    for ci, cam in enumerate(cams):
        sb, zb = r.trace_screen_centred(cam, 0.0)
        assert (vs[ci] == sb).all() and (_bits(vz[ci]) == _bits(zb)).all(), (variant, ci)
        _same((vs[ci], vz[ci]), _oracle_frame(oracle_lib, sc, ci, W, H, 1), (variant, ci))
    r.close()


# ---------------------------------------------------------------- 5. tables that change size under frames in flight ----

def _flight_tables(oracle_lib):
    """eight object tables in turn, all in level.txt: on chip -> device memory and back, growing and not growing"""
    from oracle import SPHERE_DTYPE
    t0 = HC.mark_spheres(np.ascontiguousarray(load_spheres("t0"), SPHERE_DTYPE))
    near, every, fat = (BS.scene(n, oracle_lib) for n in ("swarm_near", "swarm_all", "fat"))
    seq = [("t0", t0), ("swarm_near", near.spheres), ("t0", t0), ("swarm_all", every.spheres), ("fat", fat.spheres),
           ("swarm_near_1500", HC.mark_spheres(near.spheres[:1500])), ("swarm_all", every.spheres), ("t0", t0)]
    return near.spawn, [BS.Scene(n, "pwnfps_level", s, near.spawn) for n, s in seq]


def _via_upload(r, k, sc):
    r.set_objects(sc.spheres)


def _via_object_table(r, k, sc):
    """the same table through obj_new / obj_set / level_prepare_render: the live objects, in table order, are sc.spheres"""
    have = len(r.object_ids())
    handles = list(r.object_ids())
    while len(handles) < len(sc.spheres):
        handles.append(r.obj_new())
    for o, s in zip(handles, sc.spheres):
        r.obj_set(o, "sphere", *(float(s[f]) for f in ("r", "refl", "x", "y", "z", "cb", "cg", "cr")))
    for o in handles[len(sc.spheres):have]:
        r.obj_free(o)
    r.level_prepare_render()
    assert len(r.object_ids()) == len(sc.spheres)


@pytest.mark.parametrize("how,steps", [("upload", 8), ("object_table", 3)])
def test_tables_change_size_under_frames_in_flight(oracle_lib, how, steps):
    spawn, seq = _flight_tables(oracle_lib)
    seq = seq[:steps]
    slots = 3
    r = _renderer(W, H)
    r.level_load(level_path("pwnfps_level"))
    r.frames_config(slots, sbuf=True, zbuf=True)
    cams = BS.cameras(spawn, oracle_lib)
    forms, got = [], {}
    for f in range(len(seq) + slots - 1):
        if f >= slots - 1:
            k = f - (slots - 1)
            fr = r.wait_frame(k % slots)
            assert fr["seq"] == k + 1
            got[k] = (fr["sbuf"].copy(), fr["zbuf"].copy())
        if f < len(seq):
            (_via_upload if how == "upload" else _via_object_table)(r, f, seq[f])
            forms.append(r.sphere_tables()["form"])
            r.submit_frame(cams[f % 3], 0.0, f % slots)
    assert forms == [1, 2, 1, 2, 2, 2, 2, 1][:steps]
    for k, sc in enumerate(seq):
        _same(got[k], _oracle_frame(oracle_lib, sc, k % 3, W, H, 1, level="pwnfps_level"), (how, k, sc.name))
    r.frames_config(0)
    r.close()


# ---------------------------------------------------------------- 6. the other paths ----

def test_strips_and_call_strips(oracle_lib):
    """pwn_trace_rows_device in two strips + pwn_blur_rows_device = the frame; PWN_OPT_CALL_STRIPS 4 = one piece"""
    import torch
    sc = BS.scene("swarm_near", oracle_lib)
    cam = BS.cameras(sc.spawn, oracle_lib)[1]
    want = _oracle_frame(oracle_lib, sc, 1, W, H, 1)
    r = _scene_renderer(sc, W, H, blur=1)
    dev = torch.device("cuda:0")
    pre = torch.zeros((H, W), dtype=torch.int32, device=dev)
    z = torch.zeros((H, W), dtype=torch.float32, device=dev)
    out = torch.zeros((H, W), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for y0, y1 in ((0, 52), (52, H)):
        r.trace_rows_device(cam, 0.0, y0, y1, pre.data_ptr(), z.data_ptr(), stream)
    for y0, y1 in ((0, 52), (52, H)):
        r.blur_rows_device(y0, y1, pre.data_ptr(), z.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    _same((out.cpu().numpy().view(np.uint32), z.cpu().numpy()), want, "strips")
    r.set_call_strips(0)
    one = r.trace_screen_centred(cam, 0.0)
    r.set_call_strips(4)
    four = r.trace_screen_centred(cam, 0.0)
    assert r.call_strips_state()["strips_last"] == 4
    _same(one, want, "one piece")
    _same(four, want, "four strips")
    r.close()


@pytest.mark.parametrize("option", ["refill", "unit_order"])
def test_scheduler_and_unit_order_options_are_accepted(oracle_lib, option):
    """tables in device memory always run the units kernel, in arithmetic order: PWN_OK and the same frame"""
    sc = BS.scene("swarm_near", oracle_lib)
    cam = BS.cameras(sc.spawn, oracle_lib)[2]
    r = _scene_renderer(sc, W, H, blur=1)
    if option == "refill":
        r.set_scheduler("refill")
    else:
        r.set_unit_order(True)
    assert r.sphere_tables()["form"] == 2
    for _ in range(2):              # (twice: an ordered launch would use the first one's costs)
        _same(r.trace_screen_centred(cam, 0.0), _oracle_frame(oracle_lib, sc, 2, W, H, 1), option)
    if option == "unit_order":
        st = r.unit_order_state()
        assert st["option"] == 1 and st["launches_in_sorted_order"] == 0
    # back on chip the option holds again
    r.set_objects(HC.mark_spheres(load_spheres("t0")))
    assert r.sphere_tables()["form"] == (0 if option == "refill" else 1)
    sb, zb = r.trace_screen_centred(cam, 0.0)
    r.close()
    r = _renderer(W, H)
    r.level_load(level_path(sc.level))
    r.set_objects(HC.mark_spheres(load_spheres("t0")))
    sb2, zb2 = r.trace_screen_centred(cam, 0.0)
    r.close()
    assert (sb == sb2).all() and (_bits(zb) == _bits(zb2)).all()


def test_group_of_two_members(oracle_lib):
    """a pwn_init_multi handle, two members on device 0 over the in-process transport: the oracle's swarm_near frame at 320 x 240"""
    sc = BS.scene("swarm_near", oracle_lib)
    cam = BS.cameras(sc.spawn, oracle_lib)[1]
    r = _renderer(320, 240, {"PWN_GROUP_TRANSPORT": "local"}, devices=[0, 0])
    assert r.group_info()["members"] == 2 and r.group_info()["transport"] == "local"
    r.level_load(level_path(sc.level))
    r.set_objects(sc.spheres)
    assert r.sphere_tables()["form"] == 2
    sb = np.zeros((240, 320), np.uint32)
    zb = np.zeros((240, 320), np.float32)
    r.trace_screen_centred(cam, 0.0, sbuf=sb, zbuf=zb)
    _same((sb, zb), _oracle_frame(oracle_lib, sc, 1, 320, 240, 1), "group")
    r.close()


def test_two_rank_tiling_over_shared_memory(oracle_lib, tmp_path):
    """two ranks, fresh child processes, PWN_TRANSPORT_SHM (as tests/test_gpu_tiled.py): the oracle's swarm_near frame at 320 x 240"""
    sc = BS.scene("swarm_near", oracle_lib)
    want = oracle_lib.fnv64(_oracle_frame(oracle_lib, sc, 1, 320, 240, 1)[0])
    idfile = str(tmp_path / "id")
    prog = os.path.join(ROOT, "tests", "big_scenes.py")
    procs = [subprocess.Popen([sys.executable, prog, "rank", str(k), "2", idfile, "swarm_near", "320", "240"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in range(2)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, e[-3000:]
        outs.append(o)
    m = re.search(r"frame fnv64 ([0-9a-f]{16}) form (\d)", outs[0])
    assert m is not None, outs
    assert m.group(1) == want and m.group(2) == "2"


# ---------------------------------------------------------------- 7. refusal ----

def test_refused_tables_leave_the_previous_ones_in_force(oracle_lib):
    import pwnfps_amd
    sc = BS.scene("swarm_near", oracle_lib)
    cam = BS.cameras(sc.spawn, oracle_lib)[0]
    want = _oracle_frame(oracle_lib, sc, 0, W, H, 1)
    r = _scene_renderer(sc, W, H, blur=1)
    _same(r.trace_screen_centred(cam, 0.0), want, "before")
    before = r.sphere_tables()
    big = np.zeros(4096, BS.SPHERE_DTYPE)
    big["r"] = 100.0
    big["x"] = big["z"] = 32.0
    big["y"] = 0.5
    with pytest.raises(pwnfps_amd.PwnError) as e:
        r.set_objects(big)
    assert e.value.code == PWN_ETOOBIG
    assert r.sphere_tables() == before and before["form"] == 2
    _same(r.trace_screen_centred(cam, 0.0), want, "after")
    assert len(r.get_objects()) == len(sc.spheres)
    r.close()
