"""pwn_players_step / pwn_players_step_device on the GPU: every float and every counter bit-identical to host/player.c
(tests/players_model.py: the model, the corpus and the hand-made level), in both forms, over the batch sizes around a wave, long
walks call by call and in calls of many ticks, the tick lengths that leave the grid and that take the sine's general path, states
outside the domain beside exact ones, the level in force behind uploads on the same stream, the cameras handed straight to
pwn_trace_views_device, what the call leaves alone, and its refusals."""
import numpy as np
import pytest

import players_model as M
from conftest import level_path, load_spheres

pytestmark = pytest.mark.gpu

PWN_EINVAL, PWN_ENOLEVEL, PWN_EBUSY, PWN_ENOTSUP = -1, -6, -8, -9
POISON = np.uint32(0x7fc0dead)            # a NaN pattern no computation makes
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same(got, want, what=""):
    """all arrays of a state (cams, gravity, traversals) bit for bit"""
    for name, g, w in zip(("cams", "gravity", "traversals"), got, want):
        if w is None:
            assert g is None
            continue
        bad = np.nonzero((_bits(g).reshape(len(w), -1) != _bits(w).reshape(len(w), -1)).any(axis=1))[0]
        assert len(bad) == 0, "%s %s: %d players differ, first %d: got %s want %s" % (what, name, len(bad), bad[0], g.reshape(len(w), -1)[bad[0]], w.reshape(len(w), -1)[bad[0]])


@pytest.fixture(scope="module")
def levels():
    data, pmap = M.shipped_level()
    hd, hp = M.parse_level(M.HAND_LEVEL)
    return {"shipped": (data, pmap), "hand": (hd, hp)}


@pytest.fixture(scope="module")
def rdr():
    import pwnfps_amd
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    data, pmap, _ = r.get_level()
    sd, sp = M.shipped_level()
    assert (data == sd).all() and (pmap == sp).all()          # (the model walks the level pwn_get_level returns)
    yield r
    r.close()


def _to_dev(start):
    import torch
    dev = torch.device("cuda", 0)
    keys, cams, grav, trav = start
    return (torch.from_numpy(np.array(keys, np.uint8)).to(dev), torch.from_numpy(np.array(cams, F).reshape(len(keys), 16)).to(dev),
            torch.from_numpy(np.array(grav, F)).to(dev), torch.from_numpy(np.array(trav, np.int32)).to(dev) if trav is not None else None)


def _from_dev(t):
    return tuple(x.cpu().numpy() if x is not None else None for x in t[1:])


def _device(r, start, tdiff, ticks=1, calls=1):
    """`calls` device calls on a stream of its own, nothing waited for between them -> the state on the host"""
    import torch
    s = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(s):
        t = _to_dev(start)
        for _ in range(calls):
            r.players_step_device(t[0], t[1], t[2], t[3], tdiff=tdiff, ticks=ticks)
        out = _from_dev(t)
    s.synchronize()
    return out


def _batch(levels, n=4096):
    data, pmap = levels["shipped"]
    edges = M.edge_walkers(data, pmap)
    b = M.concat(M.corpus_states(data, n - len(edges[0])), edges)
    b[1][:, 4:8] = POISON.view(F)
    return b


# ---------------------------------------------------------------- one tick ----

@pytest.mark.parametrize("form", ["host", "device"])
def test_one_tick_of_the_whole_corpus(rdr, levels, form):
    """about 4096 players, one tick of 1 / 60: both forms; row y of every camera is poison and comes back untouched"""
    data, pmap = levels["shipped"]
    b = _batch(levels)
    want = M.model_step(data, pmap, b[0], 1 / 60, 1, *b[1:])
    assert (_bits(want[0][:, 4:8]) == POISON).all()
    assert not (_bits(want[0]) == _bits(b[1])).all(axis=1).all()
    if form == "host":
        keep = [np.array(x) for x in b]
        got = rdr.players_step(b[0], b[1], b[2], b[3], tdiff=1 / 60, ticks=1)
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(b, keep))        # new arrays: the arguments are as they were
    else:
        got = _device(rdr, b, 1 / 60)
    _same(got, want, form)
    assert (_bits(got[0][:, 4:8]) == POISON).all()


@pytest.mark.parametrize("level", ["shipped", "hand"])
def test_edges_and_portals_tick_by_tick(levels, level):
    """the players that walk into every portal endpoint and over every step of a two-high room, 14 device calls, compared after
    each: on the shipped level and on the hand-made one (every rotation from both ends, the unpaired letter)"""
    import pwnfps_amd
    import torch
    data, pmap = levels[level]
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load_text(M.HAND_LEVEL) if level == "hand" else r.level_load(level_path("pwnfps_level"))
    gd, gp, _ = r.get_level()
    assert (gd == data).all() and (gp == pmap).all()
    start = M.edge_walkers(data, pmap)
    t = _to_dev(start)
    snaps, want, state = [], [], start[1:]
    for _ in range(14):
        r.players_step_device(*t, tdiff=1 / 60, ticks=1)
        snaps.append(tuple(x.clone() for x in t))
        state = M.model_step(data, pmap, start[0], 1 / 60, 1, *state)
        want.append(state)
    torch.cuda.synchronize()
    for i, (s, w) in enumerate(zip(snaps, want)):
        _same(_from_dev(s), w, "%s tick %d" % (level, i))
    assert (want[-1][2] > 0).sum() >= 9
    r.close()


# ---------------------------------------------------------------- batch edges ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(rdr, levels, n):
    """the tail of the last wave: one element behind each array is poison and stays"""
    import torch
    data, pmap = levels["shipped"]
    dev = torch.device("cuda", 0)
    b = M.corpus_states(data, n, seed=n)
    want = M.model_step(data, pmap, b[0], 1 / 60, 2, *b[1:])
    pad = lambda a, v: np.concatenate([np.ascontiguousarray(a).ravel(), np.array([v], a.dtype)])
    tk = torch.from_numpy(pad(b[0], 0xa5)).to(dev)
    tc = torch.from_numpy(pad(b[1], POISON.view(F))).to(dev)
    tg = torch.from_numpy(pad(b[2], POISON.view(F))).to(dev)
    tt = torch.from_numpy(pad(b[3], -77)).to(dev)
    rdr.players_step_device(tk[:n], tc[:16 * n].view(n, 16), tg[:4 * n].view(n, 4), tt[:n], tdiff=1 / 60, ticks=2)
    torch.cuda.synchronize()
    c, g, t, k = tc.cpu().numpy(), tg.cpu().numpy(), tt.cpu().numpy(), tk.cpu().numpy()
    _same((c[:16 * n].reshape(n, 16), g[:4 * n].reshape(n, 4), t[:n]), want, "n %d" % n)
    assert _bits(c[16 * n:])[0] == POISON and _bits(g[4 * n:])[0] == POISON and t[n] == -77 and k[n] == 0xa5 and (k[:n] == b[0]).all()
    _same(rdr.players_step(*b, tdiff=1 / 60, ticks=2), want, "host n %d" % n)


def test_empty_batch(rdr):
    from pwnfps_amd import _lib
    L = _lib.lib
    assert L.pwn_players_step(rdr._ctx, 0, None, 1 / 60, 1, None, None, None) == 0
    assert L.pwn_players_step_device(rdr._ctx, 0, None, 1 / 60, 1, None, None, None, None) == 0
    c, g, t = rdr.players_step(np.zeros(0, np.uint8), np.zeros((0, 16), F), np.zeros((0, 4), F), np.zeros(0, np.int32))
    assert c.shape == (0, 16) and g.shape == (0, 4) and t.shape == (0,)


# ---------------------------------------------------------------- walks ----

def _walk_start(levels):
    data, pmap = levels["shipped"]
    edges = M.edge_walkers(data, pmap)
    start = M.concat(M.corpus_states(data, 257 - len(edges[0]), seed=99), edges)
    rng = np.random.default_rng(4242)
    keysets = [start[0]] + [rng.integers(0, 256, 257).astype(np.uint8) for _ in range(29)]
    return start, keysets


@pytest.fixture(scope="module")
def walk(levels):
    """the model's walk: 257 players, 600 ticks, key bytes changing every 20 -- the states after every 50th tick and the last"""
    data, pmap = levels["shipped"]
    start, keysets = _walk_start(levels)
    state, marks = start[1:], {}
    for call in range(600):
        state = M.model_step(data, pmap, keysets[call // 20], 1 / 60, 1, *state)
        if (call + 1) % 50 == 0:
            marks[call + 1] = state
    assert (state[2] != start[3]).any(), "nobody walked through a portal"
    return start, keysets, marks


def test_walk_call_by_call(rdr, walk):
    """600 device calls on one stream, nothing waited for; compared after every 50th call and at the end"""
    import torch
    start, keysets, marks = walk
    s = torch.cuda.Stream(torch.device("cuda", 0))
    snaps = {}
    with torch.cuda.stream(s):
        t = _to_dev(start)
        tkeys = [torch.from_numpy(k).to(t[1].device) for k in keysets]
        for call in range(600):
            rdr.players_step_device(tkeys[call // 20], t[1], t[2], t[3], tdiff=1 / 60, ticks=1)
            if (call + 1) % 50 == 0:
                snaps[call + 1] = tuple(x.clone() for x in t)
    s.synchronize()
    for at in sorted(snaps):
        _same(_from_dev(snaps[at]), marks[at], "after call %d" % at)


def test_walk_in_calls_of_twenty_ticks(rdr, walk):
    """the same walk as 30 calls of ticks = 20: the same bits; without traversals the same cameras"""
    start, keysets, marks = walk
    for with_trav in (True, False):
        state = (start[1], start[2], start[3] if with_trav else None)
        for k in keysets:
            state = rdr.players_step(k, *state, tdiff=1 / 60, ticks=20)
        _same(state, (marks[600][0], marks[600][1], marks[600][2] if with_trav else None), "traversals %s" % with_trav)


def test_ticks_max(rdr, levels):
    data, pmap = levels["shipped"]
    b = M.corpus_states(data, 64, seed=5)
    want = M.model_step(data, pmap, b[0], 1 / 60, 1024, *b[1:])
    _same(_device(rdr, b, 1 / 60, ticks=1024), want)
    _same(_device(rdr, (b[0], b[1], b[2], None), 1 / 60, ticks=1024), (want[0], want[1], None))


@pytest.mark.parametrize("stage", ["0", "1"])
def test_both_kernels_whatever_the_ticks(levels, stage, monkeypatch):
    """PWN_PLAYERS_STAGE (read when a context is made) keeps the walk table out of LDS (0) or says what is the rule anyway (1): the same bits"""
    import pwnfps_amd
    monkeypatch.setenv("PWN_PLAYERS_STAGE", stage)
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    data, pmap = levels["shipped"]
    b = _batch(levels, 321)
    for ticks in (1, 33):
        _same(r.players_step(*b, tdiff=1 / 60, ticks=ticks), M.model_step(data, pmap, b[0], 1 / 60, ticks, *b[1:]), "ticks %d" % ticks)
    r.close()


# ---------------------------------------------------------------- tdiff ----

@pytest.mark.parametrize("tdiff,ticks", [(0.0, 3), (1 / 60, 3), (1e-4, 3), (1e4, 10), (-1 / 60, 3)])
def test_tick_lengths(rdr, levels, tdiff, ticks):
    """1e4 with move keys: a tick's move of 5e4 leaves the grid, the leading corner of the box is looked up through get_cell's clamp
    (a wall), and the push-back brings the player home: the states stay inside the domain"""
    data, pmap = levels["shipped"]
    b = M.corpus_states(data, 512, seed=11)
    want = M.model_step(data, pmap, b[0], tdiff, ticks, *b[1:])
    assert np.isfinite(want[0][:, [0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15]]).all() and (np.abs(want[0][:, [12, 14]]) <= 2 ** 20).all()
    if tdiff == 1e4:
        k = b[0].astype(np.int32)
        assert ((((k >> 4) & 1) != ((k >> 5) & 1)) | (((k >> 6) & 1) != ((k >> 7) & 1))).sum() > 256
    _same(_device(rdr, b, tdiff, ticks=ticks), want, "tdiff %g" % tdiff)


def test_turn_through_the_sines_general_path(rdr, levels):
    data, pmap = levels["shipped"]
    b = M.turners()
    want = M.model_step(data, pmap, b[0], 1e6, 1, *b[1:])
    _same(_device(rdr, b, 1e6), want, "turners (the model's sinf / cosf are this machine's libm)")
    _same(rdr.players_step(*b, tdiff=1e6, ticks=3), M.model_step(data, pmap, b[0], 1e6, 3, *b[1:]), "turners, 3 ticks")


# ---------------------------------------------------------------- outside the domain ----

def test_states_outside_the_domain(rdr, levels):
    """every fourth player has a NaN, an infinity or 1e30 in its position, heading or gravity: PWN_OK, the others exact, and an
    exact batch afterwards on the same context is exact"""
    data, pmap = levels["shipped"]
    b = M.corpus_states(data, 256, seed=21)
    bad = np.arange(0, 256, 4)
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for j, i in enumerate(bad):
        v = F(vals[j % 5])
        where = (j // 5) % 5
        if where < 3:
            b[1][i, (12, 14, 13)[where]] = v
        elif where == 3:
            b[1][i, 8 + 2 * (j % 2)] = v
        else:
            b[2][i, j % 4] = v
    good = np.setdiff1d(np.arange(256), bad)
    with np.errstate(all="ignore"):
        want = M.model_step(data, pmap, b[0], 1 / 60, 5, *b[1:])
    for got in (_device(rdr, b, 1 / 60, ticks=5), rdr.players_step(*b, tdiff=1 / 60, ticks=5), _device(rdr, b, 1 / 60, ticks=1, calls=5)):
        _same(tuple(x[good] for x in got), tuple(x[good] for x in want), "the players beside them")
    c = M.corpus_states(data, 256, seed=22)
    _same(_device(rdr, c, 1 / 60, ticks=1), M.model_step(data, pmap, c[0], 1 / 60, 1, *c[1:]), "the one-tick batch afterwards")


# ---------------------------------------------------------------- the level in force ----

@pytest.mark.parametrize("spheres_between", [False, True])
def test_level_in_force(levels, spheres_between):
    """level A, a step, level B, a step -- one stream, nothing waited for: the first result is the model's on A, the second the
    model's on B; also with an upload of spheres between the level and its step (the walk table follows the copy made current)"""
    import pwnfps_amd
    import torch
    (da, pa), (db, pb) = levels["shipped"], levels["hand"]
    start = M.concat(M.edge_walkers(db, pb), M.edge_walkers(da, pa), M.corpus_states(da, 128, seed=31))
    on_a = M.model_step(da, pa, start[0], 1 / 60, 14, *start[1:])
    on_b = M.model_step(db, pb, start[0], 1 / 60, 14, *start[1:])
    assert (on_a[2] != on_b[2]).any() and (_bits(on_a[0]) != _bits(on_b[0])).any()
    sph = load_spheres("t0")
    r = pwnfps_amd.Renderer(32, 16)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(s):
        t1, t2, t3 = _to_dev(start), _to_dev(start), _to_dev(start)
        r.level_load(level_path("pwnfps_level"))
        if spheres_between:
            r.set_objects(sph)
        r.players_step_device(*t1, tdiff=1 / 60, ticks=14)
        r.level_load_text(M.HAND_LEVEL)
        if spheres_between:
            r.set_objects(sph[:3])
            r.set_objects(sph)
        r.players_step_device(*t2, tdiff=1 / 60, ticks=14)
        r.level_load(level_path("pwnfps_level"))
        r.players_step_device(*t3, tdiff=1 / 60, ticks=1)
    s.synchronize()
    _same(_from_dev(t1), on_a, "on level A")
    _same(_from_dev(t2), on_b, "on level B")
    _same(_from_dev(t3), M.model_step(da, pa, start[0], 1 / 60, 1, *start[1:]), "on level A again")
    # ... and through more uploads than there are copies of the tables
    for i in range(6):
        r.set_objects(sph[:i + 1])
        _same(_device(r, start, 1 / 60, ticks=2), M.model_step(da, pa, start[0], 1 / 60, 2, *start[1:]), "upload %d" % i)
    r.close()


# ---------------------------------------------------------------- end to end ----

@pytest.mark.parametrize("blur", [0, 1])
def test_step_then_observe_on_one_stream(levels, blur):
    """players_step_device, then trace_views_device of the same camera tensor, one stream, nothing waited for: the frames are
    trace_views' of the cameras the model made"""
    import pwnfps_amd
    import torch
    data, pmap = levels["shipped"]
    w, h, n = 32, 16, 3
    start = tuple(x[[300, 600, 900]].copy() for x in M.corpus_states(data, 1024, seed=41))
    start[1][:, 4:8] = [0, 1, 0, 0]
    want = M.model_step(data, pmap, start[0], 1 / 60, 7, *start[1:])
    assert (want[0][:, [3, 7, 11, 15]] == [0, 0, 0, 1]).all()          # ordinary cameras: no PWN_VIEWS_HAS_W needed
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level_path("pwnfps_level"))
    r.set_objects(load_spheres("t0"))
    r.set_blur_passes(blur)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        t = _to_dev(start)
        secs = torch.zeros(n, dtype=torch.float32, device=dev)
        sb = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
        zb = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
        work = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
        r.players_step_device(*t, tdiff=1 / 60, ticks=7)
        r.trace_views_device(t[1], secs, sb, zb, work=work)
        got_sb, got_z = sb.cpu().numpy().view(np.uint32), zb.cpu().numpy()
    s.synchronize()
    _same(_from_dev(t), want)
    ref_sb, ref_z = r.trace_views(want[0], np.zeros(n, F))
    assert (got_sb == ref_sb).all() and (_bits(got_z) == _bits(ref_z)).all()
    assert len(np.unique(ref_sb)) > 8
    r.close()


# ---------------------------------------------------------------- left alone ----

def test_other_calls_are_not_disturbed():
    """a blocking frame, a batch of views, the stats of a counted frame and the launch-order waits, before and after 100 steps of both
    forms: identical, the depth that the exhausted rays of tests/step_limit.py's scene keep included"""
    import pwnfps_amd
    import step_limit
    f = step_limit.fixture()
    mask = step_limit.none_mask(f)
    assert mask.any()
    r = pwnfps_amd.Renderer(f.w, f.h)
    r.set_blur_passes(0)
    # what the exhausted rays of the frames below keep: a frame and two views of the shipped level, where every ray ends on something
    r.level_load(level_path("pwnfps_level"))
    c0 = pwnfps_amd.spawn_camera(r.get_level()[2], ang_y=0.6).reshape(16)
    r.trace_screen_centred(c0, 0.0)
    r.trace_views(np.stack([c0, c0]), np.zeros(2, F))
    r.level_load_text(f.text)
    r.set_objects(f.sph)
    r.set_counters(True)
    other = np.array(f.cam, F).reshape(4, 4).copy()
    other[3, 1] += F(0.25)

    def look():
        sb, z = r.trace_screen_centred(f.cam, f.sec)
        vsb, vz = r.trace_views(np.stack([np.array(f.cam, F).reshape(16), other.reshape(16)]), np.array([f.sec, f.sec], F))
        return [sb, z, vsb, vz]

    before = look()
    assert (before[1][mask] != 0).any(), "the depth persistence is not exercised"
    st0, waits0 = r.stats(), r.launch_order_waits()
    data, pmap, spawn = r.get_level()
    cams, grav, trav = pwnfps_amd.players_spawn(spawn, 100)
    keys = np.full(100, pwnfps_amd.PWN_MOVE_FORWARD | pwnfps_amd.PWN_MOVE_TURN_LEFT, np.uint8)
    state = (cams, grav, trav)
    for _ in range(50):
        state = r.players_step(keys, *state)
    state = _device(r, (keys,) + tuple(state), 1 / 60, calls=50)
    _same(state, M.model_step(data, pmap, keys, 1 / 60, 100, cams, grav, trav))
    assert r.stats() == st0 and r.launch_order_waits() == waits0
    after = look()
    for a, b in zip(before, after):
        assert (_bits(a) == _bits(b)).all()
    st1 = r.stats()
    for k in ("rays", "steps", "portals", "sphere_tests", "exhausted"):
        assert st1[k] == st0[k], k
    assert r.launch_order_waits() == waits0
    r.close()


# ---------------------------------------------------------------- refusals ----

class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _gpu_tensors(n=6):
    """a good argument set of players_step_device on the GPU, in buffers with room for views that start 4 bytes in"""
    import torch
    dev = torch.device("cuda", 0)
    cbuf = torch.zeros(16 * n + 4, dtype=torch.float32, device=dev)
    gbuf = torch.zeros(4 * n + 4, dtype=torch.float32, device=dev)
    good = dict(keys=torch.zeros(n, dtype=torch.uint8, device=dev), cams=cbuf[:16 * n].view(n, 16), gravity=gbuf[:4 * n].view(n, 4),
                traversals=torch.zeros(n, dtype=torch.int32, device=dev))
    return torch, dev, n, cbuf, gbuf, good


PY_REFUSALS = ["cams 4 bytes in", "gravity 4 bytes in", "cams float64", "gravity float64", "traversals int64", "keys int8", "keys n-1",
               "keys (n,1)", "gravity (n,3)", "gravity n-1 rows", "cams (n,15)", "cams strided", "cams 1-d", "gravity strided",
               "traversals n+1", "traversals strided", "keys strided", "keys on the CPU", "gravity on the CPU", "ticks 0", "ticks 1025",
               "tdiff nan", "tdiff inf"]


@pytest.mark.parametrize("what", PY_REFUSALS)
def test_python_refuses_before_the_library_is_entered(monkeypatch, what):
    """players_step_device's shape, dtype, contiguity, device and alignment rules on real GPU tensors, with the library replaced by an
    object that fails on any call: each raises ValueError first (and the good set gets through to the library)"""
    from pwnfps_amd import render
    import pwnfps_amd
    torch, dev, n, cbuf, gbuf, good = _gpu_tensors()
    bad = {
        "cams 4 bytes in": dict(cams=cbuf[1:16 * n + 1].view(n, 16)),
        "gravity 4 bytes in": dict(gravity=gbuf[1:4 * n + 1].view(n, 4)),
        "cams float64": dict(cams=torch.zeros((n, 16), dtype=torch.float64, device=dev)),
        "gravity float64": dict(gravity=torch.zeros((n, 4), dtype=torch.float64, device=dev)),
        "traversals int64": dict(traversals=torch.zeros(n, dtype=torch.int64, device=dev)),
        "keys int8": dict(keys=torch.zeros(n, dtype=torch.int8, device=dev)),
        "keys n-1": dict(keys=torch.zeros(n - 1, dtype=torch.uint8, device=dev)),
        "keys (n,1)": dict(keys=torch.zeros((n, 1), dtype=torch.uint8, device=dev)),
        "gravity (n,3)": dict(gravity=torch.zeros((n, 3), dtype=torch.float32, device=dev)),
        "gravity n-1 rows": dict(gravity=torch.zeros((n - 1, 4), dtype=torch.float32, device=dev)),
        "cams (n,15)": dict(cams=torch.zeros((n, 15), dtype=torch.float32, device=dev)),
        "cams strided": dict(cams=torch.zeros((n, 32), dtype=torch.float32, device=dev)[:, ::2]),
        "cams 1-d": dict(cams=torch.zeros(16 * n, dtype=torch.float32, device=dev)),
        "gravity strided": dict(gravity=torch.zeros((n, 8), dtype=torch.float32, device=dev)[:, ::2]),
        "traversals n+1": dict(traversals=torch.zeros(n + 1, dtype=torch.int32, device=dev)),
        "traversals strided": dict(traversals=torch.zeros(2 * n, dtype=torch.int32, device=dev)[::2]),
        "keys strided": dict(keys=torch.zeros(2 * n, dtype=torch.uint8, device=dev)[::2]),
        "keys on the CPU": dict(keys=torch.zeros(n, dtype=torch.uint8)),
        "gravity on the CPU": dict(gravity=torch.zeros((n, 4), dtype=torch.float32)),
        "ticks 0": dict(ticks=0), "ticks 1025": dict(ticks=1025), "tdiff nan": dict(tdiff=float("nan")), "tdiff inf": dict(tdiff=float("inf")),
    }[what]
    assert good["cams"].data_ptr() % 16 == 0 and good["gravity"].data_ptr() % 16 == 0
    if "bytes in" in what:
        t = list(bad.values())[0]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 32, 16, 0, None
    monkeypatch.setattr(render, "lib", _NoCall())
    with pytest.raises(ValueError):
        r.players_step_device(**dict(good, **bad))
    # the good set passes every check: it is the library that is reached
    with pytest.raises(AssertionError, match="called into the library"):
        r.players_step_device(**good)
    with pytest.raises(AssertionError, match="called into the library"):
        r.players_step_device(**dict(good, traversals=None, cams=good["cams"].view(n, 4, 4)))


def test_steps_on_two_streams_and_a_new_level(levels):
    """steps that read one copy of the tables from two streams, the first held back behind other work, then more level uploads than
    there are copies: every step walks the level that was in force when it was called"""
    import pwnfps_amd
    import torch
    (da, pa), (db, pb) = levels["shipped"], levels["hand"]
    start = M.concat(M.edge_walkers(db, pb), M.edge_walkers(da, pa), M.corpus_states(da, 128, seed=61))
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    dev = torch.device("cuda", 0)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    t1, t2, t3 = _to_dev(start), _to_dev(start), _to_dev(start)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        busy = torch.zeros(1 << 26, device=dev)
        for _ in range(60):                      # (work in front of the step on s1)
            busy.add_(1.0)
        r.players_step_device(*t1, tdiff=1 / 60, ticks=14, stream=s1)
    with torch.cuda.stream(s2):
        r.players_step_device(*t2, tdiff=1 / 60, ticks=14, stream=s2)
    for i in range(5):
        r.level_load_text(M.HAND_LEVEL)
    with torch.cuda.stream(s2):
        r.players_step_device(*t3, tdiff=1 / 60, ticks=14, stream=s2)
    torch.cuda.synchronize()
    on_a = M.model_step(da, pa, start[0], 1 / 60, 14, *start[1:])
    on_b = M.model_step(db, pb, start[0], 1 / 60, 14, *start[1:])
    _same(_from_dev(t1), on_a, "the held-back step on the first stream")
    _same(_from_dev(t2), on_a, "the step on the second stream")
    _same(_from_dev(t3), on_b, "the step behind the uploads")
    r.close()


def test_refusals(levels):
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    L = _lib.lib
    n = 70
    data, _ = levels["shipped"]
    b = M.corpus_states(data, n, seed=51)
    host = [np.array(x) for x in b]
    t = _to_dev(b)
    pk, pc, pg, pt = (x.data_ptr() for x in t)

    def h(ctx, n_=n, tdiff=1 / 60, ticks=1, k=host[0], c=host[1], g=host[2], tr=host[3]):
        p = lambda a: None if a is None else a.ctypes.data
        return L.pwn_players_step(ctx, n_, p(k), tdiff, ticks, p(c), p(g), p(tr))

    def d(ctx, n_=n, tdiff=1 / 60, ticks=1, k=pk, c=pc, g=pg, tr=pt):
        return L.pwn_players_step_device(ctx, n_, k, tdiff, ticks, c, g, tr, None)

    def untouched():
        torch.cuda.synchronize()
        return all((_bits(x) == _bits(y)).all() for x, y in zip(host, b)) and all((_bits(x.cpu().numpy()) == _bits(y)).all() for x, y in zip(t, b))

    # a fresh context: every PWN_EINVAL of the list comes before PWN_ENOLEVEL
    nl = pwnfps_amd.Renderer(32, 16)
    for ctx in (None, nl._ctx):
        for kw in (dict(n_=-1), dict(n_=(1 << 20) + 1), dict(ticks=0), dict(ticks=1025), dict(tdiff=float("nan")), dict(tdiff=float("inf")),
                   dict(k=None), dict(c=None), dict(g=None)):
            assert h(ctx, **kw) == PWN_EINVAL and d(ctx, **kw) == PWN_EINVAL, kw
    for kw in (dict(c=pc + 4), dict(c=pc + 8), dict(g=pg + 4), dict(tr=pt + 2), dict(tr=pt + 1),              # a misaligned pointer
               dict(g=pc + 16), dict(c=pg), dict(tr=pc + 64 * n - 4), dict(k=pg + 3), dict(k=pt + 4 * n - 1), dict(tr=pg + 16 * n - 4)):      # two ranges overlap
        assert d(nl._ctx, **kw) == PWN_EINVAL, kw
    assert h(nl._ctx) == PWN_ENOLEVEL and d(nl._ctx) == PWN_ENOLEVEL
    assert h(nl._ctx, n_=0) == PWN_ENOLEVEL and d(nl._ctx, n_=0) == PWN_ENOLEVEL
    assert untouched()
    nl.close()
    # a pwn_init_multi handle
    g = pwnfps_amd.Renderer(32, 16, devices=[0, 0])
    g.level_load(level_path("pwnfps_level"))
    assert h(g._ctx) == PWN_ENOTSUP and d(g._ctx) == PWN_ENOTSUP
    g.close()
    assert untouched()
    # while the context runs a row tiling
    r = pwnfps_amd.Renderer(32, 16)
    r.level_load(level_path("pwnfps_level"))
    r.tiled_init(0, 1, pwnfps_amd.Renderer.tiled_unique_id("shm"), "shm", -1)
    assert h(r._ctx) == PWN_EBUSY and d(r._ctx) == PWN_EBUSY
    r.tiled_shutdown()
    assert untouched()
    # (d_keys may have any alignment, and traversals may be missing; the same context serves again)
    assert d(r._ctx, k=pk + 1, n_=n - 1) == 0 and h(r._ctx, tr=None) == 0
    torch.cuda.synchronize()
    assert not untouched()
    r.close()
