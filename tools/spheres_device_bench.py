#!/usr/bin/env python3
"""What pwn_upload_spheres_device costs (profiles/spheres_device/bench.txt), three things, the two sides of each alternating in one run
and every figure the median of 20 (measuring-on-mi355x):

1. The call alone and back to back, n = 14 (level.txt's spheres), 64, 1024 and 10000 (tests/big_scenes.py swarm_all), beside the host
   route on the same spheres: the records copied down into pinned memory, pwn_upload_spheres, the wait for its upload.
   Device: HIP events around ONE call (its four launches), and around a run of 20 calls, / 20.  Host: a wall clock around the three
   legs, ending in a synchronise.  Before a time is printed the state words are held against pwn_sphere_tables_plan.
2. What the forced device-memory form of the lists costs the TRACE: level.txt's 14 spheres and synth64's at 3840x2160, device-built
   tables (form 2) against the on-chip form pwn_upload_spheres picks, the blocking call's trace_ms (the library's HIP events), frames
   compared bit for bit first.
3. The ten-tick loop of tests/test_gpu_spheres_device.py -- step, spheres from the cameras, tables, first-hit planes of every
   player's view -- for 64 and 1024 players at 160x120: HIP events around ten device ticks on one stream against a wall clock around
   ten host-driven ticks.

    python tools/spheres_device_bench.py [--commit TEXT] [--out FILE] [--parts 123]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
med = statistics.median


def level_path(name):
    return os.path.join(ROOT, "tests", "golden", "levels", name + ".txt")


def tensor(torch, np, s, dev):
    return torch.from_numpy(np.ascontiguousarray(s).view(np.int32).reshape(len(s), 8).copy()).to(dev).view(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="123")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("spheres_device_bench: no GPU; nothing is measured without one")
    import pwnfps_amd
    dev = torch.device("cuda", 0)
    DT = pwnfps_amd.SPHERE_DTYPE
    gold = os.path.join(ROOT, "tests", "golden")
    lines = ["# tools/spheres_device_bench.py: pwn_upload_spheres_device", "# commit: %s" % a.commit,
             "# command: python tools/spheres_device_bench.py --out profiles/spheres_device/bench.txt",
             "# device: %s; torch %s; every figure the median of 20, the two sides alternating in one run" % (torch.cuda.get_device_name(0), torch.__version__)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def rand(n, seed, cx, cz, spread):
        rng = np.random.default_rng(seed)
        s = np.zeros(n, DT)
        s["x"], s["z"] = cx + rng.uniform(-spread, spread, n), cz + rng.uniform(-spread, spread, n)
        s["y"], s["r"], s["refl"] = rng.uniform(0.2, 0.8, n), rng.uniform(0.05, 0.3, n), rng.uniform(0, 0.9, n)
        for c in ("cb", "cg", "cr"):
            s[c] = rng.uniform(0.1, 1.0, n)
        return s

    # ---- 1: the call
    if "1" in a.parts:
        say("# 1. the call: one_us HIP events around one call (four launches); run_us around 20 calls, / 20; host_us a wall clock around the host")
        say("#    route (d2h_us the records down, upload_us pwn_upload_spheres, wait_us the synchronise behind it); host/device = host_us / run_us")
        say("%-6s %8s %6s %8s %9s %9s %9s %8s %10s %8s %12s" % ("n", "pairs", "cells", "longest", "one_us", "run_us", "host_us", "d2h_us", "upload_us", "wait_us", "host/device"))
        import oracle
        import big_scenes
        oracle.build()
        sets = []
        r0 = pwnfps_amd.Renderer(64, 32)
        r0.level_load(level_path("pwnfps_level"))
        sp = r0.get_level()[2]
        r0.close()
        sets.append(("pwnfps_level", np.ascontiguousarray(np.load(os.path.join(gold, "spheres_t0.npy")), DT)))
        sets.append(("pwnfps_level", rand(64, 1, sp[0] + 0.5, sp[1] + 0.5, 4.0)))
        sets.append(("pwnfps_level", rand(1024, 2, sp[0] + 0.5, sp[1] + 0.5, 8.0)))
        sc = big_scenes.scene("swarm_all", oracle)
        sets.append((sc.level, np.ascontiguousarray(sc.spheres, DT)))
        for level, s in sets:
            n = len(s)
            plan = pwnfps_amd.sphere_tables_plan(s)
            rd, rh = pwnfps_amd.Renderer(64, 32), pwnfps_amd.Renderer(64, 32)
            for r in (rd, rh):
                r.level_load(level_path(level))
            t = tensor(torch, np, s, dev)
            pinned = torch.empty((n, 8), dtype=torch.float32).pin_memory()
            mp = plan["pairs"]
            one, run, host, d2h, up, wait = [], [], [], [], [], []
            for it in range(25):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                rd.upload_spheres_device(t, mp)
                e[1].record()
                e[2].record()
                for _ in range(20):
                    rd.upload_spheres_device(t, mp)
                e[3].record()
                e[3].synchronize()
                if it == 0:          # (a timing of a wrong answer is no timing)
                    st = rd.spheres_device_state()
                    assert (st["pairs"], st["cells"], st["longest"], st["reason"]) == (plan["pairs"], plan["cells"], plan["longest"], 0), st
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                pinned.copy_(t, non_blocking=True)
                torch.cuda.synchronize()
                c1 = time.perf_counter()
                rh.set_objects(pinned.numpy().view(DT).reshape(n))
                c2 = time.perf_counter()
                torch.cuda.synchronize()
                c3 = time.perf_counter()
                if it >= 5:
                    one.append(e[0].elapsed_time(e[1]) * 1e3)
                    run.append(e[2].elapsed_time(e[3]) * 1e3 / 20)
                    host.append((c3 - c0) * 1e6); d2h.append((c1 - c0) * 1e6); up.append((c2 - c1) * 1e6); wait.append((c3 - c2) * 1e6)
            say("%-6d %8d %6d %8d %9.1f %9.1f %9.1f %8.1f %10.1f %8.1f %12.1f" % (n, plan["pairs"], plan["cells"], plan["longest"], med(one), med(run), med(host),
                                                                              med(d2h), med(up), med(wait), med(host) / med(run)))
            rd.close()
            rh.close()

    # ---- 2: what the device-memory form costs the trace
    if "2" in a.parts:
        W, H = 3840, 2160
        say("# 2. the trace at %dx%d: pwn_stats.trace_ms of the blocking call (the library's HIP events: the call runs in row strips, so from its" % (W, H))
        say("#    start to the end of the last strip's trace, earlier strips' blur and copies beside it -- the same on every side), tables built on the")
        say("#    device (form 2: records in device memory; device_ms with max_pairs = 4096: 42 KB of LDS; tight_ms with max_pairs = the pairs)")
        say("#    against pwn_upload_spheres' on-chip form")
        say("%-14s %6s %10s %12s %12s %12s %10s %10s" % ("scene", "n", "host_form", "host_ms", "device_ms", "tight_ms", "dev/host", "tight/host"))
        for level, key in (("pwnfps_level", "t0"), ("synth64", "synth64")):
            s = np.load(os.path.join(gold, "spheres_t0.npy") if key == "t0" else os.path.join(gold, "levels", key + "_spheres.npy"))
            s = np.ascontiguousarray(s, DT)
            plan = pwnfps_amd.sphere_tables_plan(s)
            rs = [pwnfps_amd.Renderer(W, H) for _ in range(3)]
            for r in rs:
                r.level_load(level_path(level))
            t = tensor(torch, np, s, dev)
            rs[0].set_objects(s)
            rs[1].upload_spheres_device(t, max(4096, plan["pairs"]))
            rs[2].upload_spheres_device(t, plan["pairs"])
            cam = pwnfps_amd.spawn_camera(rs[0].get_level()[2], ang_y=0.6)
            frames = [r.trace_screen_centred(cam, 1.25) for r in rs]
            for f in frames[1:]:
                assert (f[0] == frames[0][0]).all() and (f[1].view(np.uint32) == frames[0][1].view(np.uint32)).all()
            ms = [[], [], []]
            for it in range(25):
                for k, r in enumerate(rs):
                    r.trace_screen_centred(cam, 1.25)
                    if it >= 5:
                        ms[k].append(r.stats()["trace_ms"])
            m = [med(v) for v in ms]
            say("%-14s %6d %10d %12.4f %12.4f %12.4f %10.3f %10.3f" % (level, len(s), rs[0].sphere_tables()["form"], m[0], m[1], m[2], m[1] / m[0], m[2] / m[0]))
            for r in rs:
                r.close()

    # ---- 3: the loop
    if "3" in a.parts:
        W, H, ticks = 160, 120, 10
        say("# 3. ten ticks at %dx%d, every player's view observed (first-hit planes): device_ms HIP events around the ten ticks on one stream" % (W, H))
        say("#    (step, spheres from the cameras, tables, planes; nothing waited for), host_ms a wall clock around the host-driven ticks")
        say("%-8s %12s %12s %12s" % ("players", "device_ms", "host_ms", "host/device"))
        for n in (64, 1024):
            rd, rh = pwnfps_amd.Renderer(W, H), pwnfps_amd.Renderer(W, H)
            for r in (rd, rh):
                r.level_load(level_path("pwnfps_level"))
            sp = rd.get_level()[2]
            cams0 = np.stack([pwnfps_amd.spawn_camera(sp, ang_y=0.07 * i).reshape(16) for i in range(n)]).astype(np.float32)
            grav0 = np.zeros((n, 4), np.float32)
            keys = np.random.default_rng(3).choice([16, 17, 18, 32, 64, 128, 0], n).astype(np.uint8)
            d_keys = torch.from_numpy(keys).to(dev)
            d_sph = torch.zeros((n, 8), dtype=torch.float32, device=dev)
            d_sph[:, 0], d_sph[:, 1] = 0.25, 0.2
            d_sph[:, 5], d_sph[:, 6], d_sph[:, 7] = 0.3, 0.6, 0.9
            label = torch.empty((n, H, W), dtype=torch.int32, device=dev)
            hs = np.zeros(n, DT)
            hs["r"], hs["refl"], hs["cb"], hs["cg"], hs["cr"] = 0.25, 0.2, 0.3, 0.6, 0.9
            dms, hms = [], []
            for it in range(25):
                d_cams, d_grav = torch.from_numpy(cams0.copy()).to(dev), torch.from_numpy(grav0.copy()).to(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(ticks):
                    rd.players_step_device(d_keys, d_cams, d_grav, tdiff=1 / 60, ticks=3)
                    d_sph[:, 2:5] = d_cams[:, 12:15]
                    rd.upload_spheres_device(d_sph, 4 * n)
                    rd.trace_view_hits_device(d_cams, label)
                e1.record()
                e1.synchronize()
                last_dev = label.cpu().numpy()
                hc, hg = cams0.copy(), grav0.copy()
                c0 = time.perf_counter()
                for _ in range(ticks):
                    hc, hg, _t = rh.players_step(keys, hc, hg, tdiff=1 / 60, ticks=3)
                    hs["x"], hs["y"], hs["z"] = hc[:, 12], hc[:, 13], hc[:, 14]
                    rh.set_objects(hs)
                    last_host = rh.trace_view_hits(hc, want_cell=False, want_dist=False)[0]
                c1 = time.perf_counter()
                assert (last_dev.view(np.uint32) == last_host).all()
                if it >= 5:
                    dms.append(e0.elapsed_time(e1))
                    hms.append((c1 - c0) * 1e3)
            say("%-8d %12.3f %12.3f %12.1f" % (n, med(dms), med(hms), med(hms) / med(dms)))
            rd.close()
            rh.close()

    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
