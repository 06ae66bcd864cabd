"""Sphere tables that outgrow LDS: the scenes of tests/test_big_scenes.py and tests/test_gpu_big_scenes.py (and of
tools/big_bench.py), generated from seeds.  Each breaks one of the rules that kept a sphere set on chip -- 16-bit sphere offsets
(2048 spheres), 72 KiB of blob, 32767 list entries -- and is rendered by the oracle in well under a second.

    scene(name, oracle_mod) -> Scene(name, level, spheres, spawn)       spheres marked (hit_chain.mark_spheres)
    cameras(spawn, oracle_mod) -> the three cameras of hit_chain.level_frames at that spawn cell
    oracle_for(sc, oracle_mod) -> an Oracle with the scene loaded (one per scene, shared: do not change its spheres)

Run as a program it is one rank of a two-rank row tiling over shared memory that prints the hash of a scene's frame:
    python3 tests/big_scenes.py rank RANK WORLD IDFILE SCENE W H
"""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPHERE_DTYPE = np.dtype([("r", "<f4"), ("refl", "<f4"), ("x", "<f4"), ("y", "<f4"),
                         ("z", "<f4"), ("cb", "<f4"), ("cg", "<f4"), ("cr", "<f4")])
Scene = namedtuple("Scene", "name level spheres spawn")
YAWS = (0.0, 0.8, 5.6)
NAMES = ("swarm_near", "swarm_all", "fat", "one_over")
LEVELS = {"swarm_near": "pwnfps_level", "swarm_all": "synth64", "fat": "pwnfps_level", "one_over": "pwnfps_level"}


def swarm(data, spawn, n, rlo, rhi, seed, reach):   # data, spawn: Oracle.get_level()
    rng = np.random.default_rng(seed)
    zs, xs = np.nonzero(np.isin(data, [ord(c) for c in ';$"#&']))
    if reach is not None:
        k = (abs(xs - spawn[0]) <= reach) & (abs(zs - spawn[1]) <= reach)
        xs, zs = xs[k], zs[k]
    j = rng.integers(0, len(xs), n)
    s = np.zeros(n, SPHERE_DTYPE)
    s["x"] = xs[j] + rng.random(n)
    s["z"] = zs[j] + rng.random(n)
    s["y"] = rng.uniform(0.3, 0.6, n)
    s["r"] = rng.uniform(rlo, rhi, n)
    s["refl"] = rng.uniform(0, 0.9, n)
    for c in ("cb", "cg", "cr"):
        s[c] = rng.uniform(0.1, 1.0, n)
    return s


def level_path(name):
    return os.path.join(HERE, "golden", "levels", name + ".txt")


_levels = {}


def _level(name, oracle_mod):
    if name not in _levels:
        O = oracle_mod.Oracle()
        O.load_level(level_path(name))
        data, _, spawn = O.get_level()
        _levels[name] = (data, spawn)
    return _levels[name]


def form_of(spheres):
    import pwnfps_amd
    return pwnfps_amd.sphere_tables_plan(spheres)["form"]


def one_over_k(spheres):
    """the k with form <= 1 for the first k spheres and form 2 for the first k + 1 (pwn_sphere_tables_plan), by bisection"""
    lo, hi = 0, len(spheres)
    assert form_of(spheres[:lo]) <= 1 and form_of(spheres[:hi]) == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if form_of(spheres[:mid]) <= 1:
            lo = mid
        else:
            hi = mid
    return lo


_scenes = {}


def scene(name, oracle_mod):
    """the scene, or for "one_over" the scene of k + 1 spheres (its first k are the other side of the rule: one_over_pair)"""
    if name not in _scenes:
        from hit_chain import mark_spheres
        data, spawn = _level(LEVELS[name], oracle_mod)
        if name == "swarm_near":
            s = swarm(data, spawn, 2100, 0.02, 0.08, 7, 6)
        elif name == "swarm_all":
            s = swarm(data, spawn, 10000, 0.02, 0.2, 7, None)
        elif name == "fat":
            s = swarm(data, spawn, 800, 1.5, 4.0, 7, None)
            rng2 = np.random.default_rng(8)
            sign = rng2.choice([-1, 1], len(s))
            u = rng2.uniform(-0.35, 0.6, len(s))
            s["y"] = 0.5 + sign * (s["r"] + u)
        elif name == "one_over":
            s = swarm(data, spawn, 2000, 0.03, 0.1, 9, 6)
            s = s[:one_over_k(s) + 1]
        else:
            raise KeyError(name)
        _scenes[name] = Scene(name, LEVELS[name], mark_spheres(s), spawn)
    return _scenes[name]


def one_over_pair(oracle_mod):
    """(the scene of k spheres: form <= 1, the scene of k + 1: form 2)"""
    over = scene("one_over", oracle_mod)
    return over._replace(name="one_over_k", spheres=over.spheres[:-1]), over


def cameras(spawn, oracle_mod):
    cams = []
    L = oracle_mod.lib()
    for yaw in YAWS:
        cam = np.eye(4, dtype=np.float32)
        L.pwno_mat4_roty(cam.ctypes.data, C.c_float(yaw))
        cam[3, :3] = (spawn[0] + 0.5, 0.5, spawn[1] + 0.5)
        cams.append(cam)
    return cams


_oracles = {}


def oracle_for(sc, oracle_mod):
    key = (sc.name, len(sc.spheres))
    if key not in _oracles:
        O = oracle_mod.Oracle()
        O.load_level(level_path(sc.level))
        O.set_spheres(sc.spheres)
        _oracles[key] = O
    return _oracles[key]


def bins(sc, oracle_mod):
    """(pairs, non-empty cells, longest list, entries of the indexed lists) by the oracle's binning"""
    counts, _ = oracle_for(sc, oracle_mod).get_bins()
    counts = counts.astype(np.int64)
    return int(counts.sum()), int((counts > 0).sum()), int(counts.max()), int(counts.sum() + (counts > 0).sum())


def _rank_main(argv):
    """one rank of a row tiling over shared memory (as tools/tiled_rank.py): rank 0 prints `frame fnv64 HASH`"""
    import time
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    rank, world, idfile, name, w, h = int(argv[0]), int(argv[1]), argv[2], argv[3], int(argv[4]), int(argv[5])
    import pwnfps_amd
    import oracle
    sc = scene(name, oracle)
    r = pwnfps_amd.Renderer(w, h)
    r.level_load(level_path(sc.level))
    if rank == 0:
        uid = pwnfps_amd.Renderer.tiled_unique_id("shm")
        with open(idfile + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            if time.time() - t0 > 120:
                sys.exit("rank %d: no id file" % rank)
            time.sleep(0.01)
        uid = open(idfile, "rb").read()
    r.tiled_init(rank, world, uid, "shm", -1)
    r.set_objects(sc.spheres)
    r.tiled_submit(cameras(sc.spawn, oracle)[1], 0.0)
    fr = r.tiled_wait(host=True)
    if fr.get("sbuf") is not None:
        print("frame fnv64 %s form %d" % (oracle.fnv64(fr["sbuf"]), r.sphere_tables()["form"]), flush=True)
    r.tiled_shutdown()
    r.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rank":
        _rank_main(sys.argv[2:])
