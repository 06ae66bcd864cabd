"""pwn_trace_reach: rays that stop after a given distance.  The reference is tests/reach_chain.py's model, which derives every record
from the oracle's event chain of the same ray (pinned on the CPU in tests/test_reach_corpus.py); the corpus is its ~6 000 rays in nine
batches of reaches.  Every check runs the kernel variants a context can pick: the sphere lists indexed, inline or in device memory
(PWN_SPHERE_LISTS) and the 4-lane variant (PWN_DBG_FORCE_HASW)."""
import contextlib
import os

import numpy as np
import pytest

import hit_chain as HC
import reach_chain as RC
from conftest import GOLD, level_path, load_spheres

pytestmark = pytest.mark.gpu

VARIANTS = {"indexed": {"PWN_SPHERE_LISTS": "indexed"}, "inline": {"PWN_SPHERE_LISTS": "inline"}, "global": {"PWN_SPHERE_LISTS": "global"},
            "force_hasw": {"PWN_DBG_FORCE_HASW": "1"}}
FORM = {"indexed": 0, "inline": 1, "global": 2}
POISON = 0x5a5a5a5a
COUNTERS = ("rays", "steps", "portals", "sphere_tests", "exhausted")
INF = np.float32(np.inf)


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


def _renderer(variant="indexed", w=8, h=8):
    import pwnfps_amd
    with _env(**VARIANTS[variant]):
        r = pwnfps_amd.Renderer(w, h)
    r.set_blur_passes(0)
    return r


def _device(r, rays, reach, hide=None, has_w=False, guard=8):
    """trace_reach_device on torch tensors in guarded, poisoned arrays: the records, as numpy"""
    import torch
    import pwnfps_amd
    n = len(rays)
    t_rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    t_reach = torch.from_numpy(np.ascontiguousarray(reach, np.float32)).cuda()
    t_hide = None if hide is None else torch.from_numpy(np.ascontiguousarray(hide, np.int32)).cuda()
    t_hits = torch.full((n + guard, 12), POISON, dtype=torch.int32, device="cuda")
    r.trace_reach_device(t_rays, t_reach, t_hits[:n], hide=t_hide, has_w=has_w)
    got = t_hits.cpu().numpy()
    assert (got[n:] == POISON).all(), "records were written behind the n-th"
    return np.ascontiguousarray(got[:n]).view(pwnfps_amd.HIT_DTYPE).reshape(n)


def _hits_device(r, rays, hide=None):
    import torch
    import pwnfps_amd
    n = len(rays)
    t_rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    t_hide = None if hide is None else torch.from_numpy(np.ascontiguousarray(hide, np.int32)).cuda()
    t_hits = torch.full((n, 12), POISON, dtype=torch.int32, device="cuda")
    r.trace_hits_device(t_rays, t_hits, hide=t_hide)
    return t_hits.cpu().numpy().view(pwnfps_amd.HIT_DTYPE).reshape(n)


def _report(got, w, bad, reach):
    return [(int(i), float(reach[i]), str(w.arm[i]), got[i].tolist(), w.want[i].tolist()) for i in bad[:3]]


def _same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


# ---------------------------------------------------------------- 1. the corpus against the model ----

@pytest.mark.parametrize("variant", list(VARIANTS))
def test_corpus_against_the_model(oracle_lib, variant):
    """both forms, every batch of every part: every field of every record the model decides, at most 1 % left out; with the counters
    on, `steps` is the model's count, never above the unlimited call's and strictly below it on the reach-0.25 batch"""
    for pi, part in enumerate(RC.corpus(oracle_lib)):
        r = _renderer(variant)
        RC.load_renderer(r, part)
        if variant in FORM:
            assert r.sphere_tables()["form"] == FORM[variant], (variant, r.sphere_tables())
        r.set_counters(True)
        n = len(part.rays)
        r.trace_hits(part.rays)
        unlimited = r.stats()["steps"]
        for bi, reach in enumerate(RC.reaches(pi, part)):
            w = RC.model(part.chains, reach)
            assert int(w.left_out.sum()) * 100 <= n, (part.name, bi, int(w.left_out.sum()))
            got = _device(r, part.rays, reach)
            st = r.stats()
            bad = RC.mismatches(got, w)
            assert len(bad) == 0, (variant, part.name, bi, "device", len(bad), _report(got, w, bad, reach))
            assert st["rays"] == n
            if not w.left_out.any():
                assert st["steps"] == int(w.steps.sum()), (variant, part.name, bi, st["steps"], int(w.steps.sum()))
                assert st["exhausted"] == int((w.want["kind"] == HC.NONE).sum())
            assert st["steps"] <= unlimited, (variant, part.name, bi)
            if bi == 1:
                assert reach[0] == np.float32(0.25) and st["steps"] < unlimited, (variant, part.name, st["steps"], unlimited)
            host = r.trace_reach(part.rays, reach)
            bad = RC.mismatches(host, w)
            assert len(bad) == 0, (variant, part.name, bi, "host", len(bad), _report(host, w, bad, reach))
            assert r.stats()["steps"] == st["steps"]
        r.close()


# ---------------------------------------------------------------- 2. batch sizes ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_in_guarded_arrays(oracle_lib, n):
    """n rays of the hand-made level under their random reaches, both device forms and the host form: the first n records and none
    behind them (_device asserts the guard)"""
    part = RC.corpus(oracle_lib)[1]
    pick = np.arange(n) * (len(part.rays) // n)
    rays = part.rays[pick]
    reach = RC.reaches(1, part)[6][pick]
    w = RC.model([part.chains[i] for i in pick], reach)
    r = _renderer()
    RC.load_renderer(r, part)
    for got in (_device(r, rays, reach), _device(r, rays, reach, hide=np.full(n, -1, np.int32)), _device(r, rays, reach, has_w=True),
                r.trace_reach(rays, reach)):
        bad = RC.mismatches(got, w)
        assert len(bad) == 0, (n, _report(got, w, bad, reach))
    assert r.trace_reach(rays[:0], reach[:0]).shape == (0,)
    r.close()


# ---------------------------------------------------------------- 3. +inf is pwn_trace_hits_device ----

@pytest.mark.parametrize("variant", list(VARIANTS))
def test_infinite_reach_is_trace_hits(oracle_lib, variant):
    """reach = +inf, and NaN: pwn_trace_hits_device's records bit for bit, the five counters included"""
    for part in RC.corpus(oracle_lib):
        r = _renderer(variant)
        RC.load_renderer(r, part)
        r.set_counters(True)
        want = _hits_device(r, part.rays)
        st_want = {k: r.stats()[k] for k in COUNTERS}
        n = len(part.rays)
        for value in (np.inf, np.nan):
            got = _device(r, part.rays, np.full(n, value, np.float32))
            assert got.tobytes() == want.tobytes(), (variant, part.name, value)
            assert {k: r.stats()[k] for k in COUNTERS} == st_want, (variant, part.name, value)
        r.close()


# ---------------------------------------------------------------- 4. hide ----

def _body_scene():
    """level.txt's 14 spheres with a body of r 0.3 around the camera put in at index 3; rays from a point inside the body"""
    import pwnfps_amd
    import edge_scenes
    r0 = _renderer()
    r0.level_load(level_path("pwnfps_level"))
    _, _, spawn = r0.get_level()
    r0.close()
    sph = HC.mark_spheres(load_spheres("t0"))
    body = np.zeros(1, sph.dtype)
    body[0] = (0.3, 0.5, spawn[0] + 0.5, 0.5, spawn[1] + 0.5, 1.0, 0.5, 0.25)
    full = np.concatenate([sph[:3], body, sph[3:]])
    rays = np.concatenate([pwnfps_amd.pixel_rays(24, 16, edge_scenes._cam(spawn[0] + 0.6, 0.45, spawn[1] + 0.55, yaw))[0] for yaw in (0.0, 0.8, 2.9, 5.6)])
    return sph, full, rays


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_hidden_body(variant):
    """a ray that starts inside sphere j: with hide = j the records are those of the table without j, objects numbered by the full
    table; with PWN_HIDE_NONE it reports j; all-NONE is the form without hide, bit for bit"""
    sph, full, rays = _body_scene()
    n, j = len(rays), 3
    rng = np.random.default_rng(4)
    reaches = [np.full(n, 0.35, np.float32), np.full(n, 2.0, np.float32), np.full(n, INF), (rng.uniform(0, 1, n) ** 2 * 8).astype(np.float32)]
    r = _renderer(variant)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(full)
    ref = _renderer(variant)
    ref.level_load(level_path("pwnfps_level"))
    ref.set_objects(sph)
    none = np.full(n, -1, np.int32)
    saw_body = differs = 0
    for reach in reaches:
        want = _device(ref, rays, reach)
        sp = want["kind"] == HC.SPHERE
        want["object"][sp & (want["object"] >= j)] += 1
        got = _device(r, rays, reach, hide=np.full(n, j, np.int32))
        assert got.tobytes() == want.tobytes(), (variant, float(reach[0]), np.flatnonzero(got != want)[:4].tolist())
        plain = _device(r, rays, reach)
        assert _device(r, rays, reach, hide=none).tobytes() == plain.tobytes()
        saw_body += int(((plain["kind"] == HC.SPHERE) & (plain["object"] == j)).sum())
        differs += int((plain != got).sum())
        # (mixed: every other ray hides the body)
        mixed = _device(r, rays, reach, hide=np.where(np.arange(n) % 2 == 0, j, 1 << 30).astype(np.int32))
        assert mixed[0::2].tobytes() == got[0::2].tobytes() and mixed[1::2].tobytes() == plain[1::2].tobytes()
    assert saw_body > 0 and differs > 0, (saw_body, differs)
    r.close()
    ref.close()


# ---------------------------------------------------------------- 5. tables built on the device ----

def test_tables_built_on_the_device(oracle_lib):
    """the level part's spheres through pwn_upload_spheres_device (the lists' device-memory form, built by sphere_bins.hip): the model's records"""
    import torch
    part = RC.corpus(oracle_lib)[0]
    r = _renderer()
    r.level_load(part.level)
    t = torch.from_numpy(np.ascontiguousarray(part.spheres).view(np.float32).reshape(-1, 8).copy()).cuda()
    r.upload_spheres_device(t, 4096)
    assert r.spheres_device_state()["in_force"] == 1
    for bi in (1, 3, 6):
        reach = RC.reaches(0, part)[bi]
        w = RC.model(part.chains, reach)
        got = _device(r, part.rays, reach)
        bad = RC.mismatches(got, w)
        assert len(bad) == 0, (bi, _report(got, w, bad, reach))
    r.close()


# ---------------------------------------------------------------- 6. left alone ----

def test_other_calls_are_not_disturbed():
    """blocking frames and batches of views interleaved with reach calls stay bit-identical to the same sequence without them (the
    depth that exhausted rays keep in the blocking call's plane and the view slots included); without the counters a device call leaves
    pwn_stats alone, and on one stream no launch has to wait for another"""
    import pwnfps_amd
    cams = np.load(os.path.join(GOLD, "levels", "synth256_cams.npy")).astype(np.float32)
    w, h = 240, 136
    rays, _, _ = pwnfps_amd.pixel_rays(w, h, cams[0])
    reach = np.resize(np.array([0.35, 3.0, np.inf, 40.0], np.float32), len(rays))
    res = []
    for between in (False, True):
        r = _renderer("indexed", w, h)
        r.level_load(level_path("synth256"))
        r.set_objects(load_spheres("synth256"))
        r.set_blur_passes(1)
        out = []

        def reach_calls():
            if not between:
                return
            r.trace_reach(rays, reach)
            st0 = r.stats()
            # (the host form went out on the context's stream, these go out on torch's: the first ones behind the change of stream are
            # put behind the launches whose ticket sets they clear, include/pwnhip.h; from then on none waits)
            for _ in range(3):
                _device(r, rays, reach)
            waits0 = r.launch_order_waits()
            _device(r, rays, reach)
            _device(r, rays, reach, hide=np.zeros(len(rays), np.int32))
            assert r.stats() == st0 and r.launch_order_waits() == waits0

        reach_calls()
        out += list(r.trace_screen_centred(cams[1], 0.0))
        reach_calls()
        out += list(r.trace_views(np.stack([cams[2], cams[0]]), np.zeros(2, np.float32)))
        reach_calls()
        out += list(r.trace_screen_centred(cams[0], 0.0))
        reach_calls()
        out += list(r.trace_views(np.stack([cams[3], cams[0]]), np.zeros(2, np.float32)))
        reach_calls()
        out += list(r.trace_screen_centred(cams[1], 0.0))
        res.append(out)
        r.close()
    assert len(res[0]) == len(res[1]) == 10
    for i, (a, b) in enumerate(zip(*res)):
        assert a.shape == b.shape and _same_bits(a, b), i


# ---------------------------------------------------------------- 7. Python's argument rules ----

class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


PY_REFUSALS = ["rays 4 bytes in", "hits 4 bytes in", "rays float64", "reach float64", "hits int64", "hide int64", "rays (n,7)", "rays 1-d",
               "reach n-1", "reach (n,1)", "hits (n,11)", "hits n+1 rows", "hide n+1", "rays strided", "reach strided", "hits strided",
               "hide strided", "reach on the CPU", "hits on the CPU", "hide on the CPU", "rays on the CPU"]


@pytest.mark.parametrize("what", PY_REFUSALS)
def test_python_refuses_before_the_library_is_entered(monkeypatch, what):
    """trace_reach_device's shape, dtype, contiguity, device and alignment rules on real GPU tensors, with the library replaced by an
    object that fails on any call: each raises ValueError first (and the good sets get through to the library)"""
    import torch
    from pwnfps_amd import render
    import pwnfps_amd
    dev = torch.device("cuda", 0)
    n = 6
    rbuf = torch.zeros(8 * n + 4, dtype=torch.float32, device=dev)
    hbuf = torch.zeros(12 * n + 4, dtype=torch.int32, device=dev)
    good = dict(rays=rbuf[:8 * n].view(n, 8), reach=torch.zeros(n, dtype=torch.float32, device=dev), hits=hbuf[:12 * n].view(n, 12),
                hide=torch.zeros(n, dtype=torch.int32, device=dev))
    bad = {
        "rays 4 bytes in": dict(rays=rbuf[1:8 * n + 1].view(n, 8)),
        "hits 4 bytes in": dict(hits=hbuf[1:12 * n + 1].view(n, 12)),
        "rays float64": dict(rays=torch.zeros((n, 8), dtype=torch.float64, device=dev)),
        "reach float64": dict(reach=torch.zeros(n, dtype=torch.float64, device=dev)),
        "hits int64": dict(hits=torch.zeros((n, 6), dtype=torch.int64, device=dev)),
        "hide int64": dict(hide=torch.zeros(n, dtype=torch.int64, device=dev)),
        "rays (n,7)": dict(rays=torch.zeros((n, 7), dtype=torch.float32, device=dev)),
        "rays 1-d": dict(rays=torch.zeros(8 * n, dtype=torch.float32, device=dev)),
        "reach n-1": dict(reach=torch.zeros(n - 1, dtype=torch.float32, device=dev)),
        "reach (n,1)": dict(reach=torch.zeros((n, 1), dtype=torch.float32, device=dev)),
        "hits (n,11)": dict(hits=torch.zeros((n, 11), dtype=torch.int32, device=dev)),
        "hits n+1 rows": dict(hits=torch.zeros((n + 1, 12), dtype=torch.int32, device=dev)),
        "hide n+1": dict(hide=torch.zeros(n + 1, dtype=torch.int32, device=dev)),
        "rays strided": dict(rays=torch.zeros((n, 16), dtype=torch.float32, device=dev)[:, ::2]),
        "reach strided": dict(reach=torch.zeros(2 * n, dtype=torch.float32, device=dev)[::2]),
        "hits strided": dict(hits=torch.zeros((n, 24), dtype=torch.int32, device=dev)[:, ::2]),
        "hide strided": dict(hide=torch.zeros(2 * n, dtype=torch.int32, device=dev)[::2]),
        "reach on the CPU": dict(reach=torch.zeros(n, dtype=torch.float32)),
        "hits on the CPU": dict(hits=torch.zeros((n, 12), dtype=torch.int32)),
        "hide on the CPU": dict(hide=torch.zeros(n, dtype=torch.int32)),
        "rays on the CPU": dict(rays=torch.zeros((n, 8), dtype=torch.float32)),
    }[what]
    assert good["rays"].data_ptr() % 16 == 0 and good["hits"].data_ptr() % 16 == 0
    if "bytes in" in what:
        t = list(bad.values())[0]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 32, 16, 0, None
    monkeypatch.setattr(render, "lib", _NoCall())
    with pytest.raises(ValueError):
        r.trace_reach_device(**dict(good, **bad))
    with pytest.raises(AssertionError, match="called into the library: pwn_trace_reach_hide_device"):
        r.trace_reach_device(**good)
    with pytest.raises(AssertionError, match="called into the library: pwn_trace_reach_device"):
        r.trace_reach_device(**dict(good, hide=None, hits=good["hits"].view(torch.uint8).view(n, 48)))
