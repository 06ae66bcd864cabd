#!/usr/bin/env python3
"""What a step of a batch of players costs (profiles/players/step.txt): pwn_players_step_device on the GPU, and beside it what the
same step cost before it existed -- host/player.c's loop over the n players on one CPU thread plus the upload of the n x 64 B of
cameras.  n = 64, 1024, 65536 and 1048576 players, ticks 1 and 64, on the shipped level.

Device: the time between two HIP events around ONE call, median of 20 after 5 warm-ups, the state put back before every call
(outside the events).  Each (n, ticks) twice: as the library runs it (every workgroup copies the walk table into LDS), and with
PWN_PLAYERS_STAGE=0 in a context of its own (the table read from device memory) -- the A/B behind that choice.
Host: a wall clock around the loop alone (host/player.c stepping preallocated arrays in place) and around the copy (which ends in a
synchronise), median of 5 (of 3 from 2^20 x 64 ticks on).
At 64 and 1024 players the device figure is the launch itself, not the kernel.

    python tools/players_bench.py [--commit TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (64, 1024, 65536, 1048576)
TICKS = (1, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("players_bench: no GPU; nothing is measured without one")
    import pwnfps_amd
    import players_model as M
    dev = torch.device("cuda", 0)
    data, pmap = M.shipped_level()
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    lines = ["# tools/players_bench.py: one step of n players on tests/golden/levels/pwnfps_level.txt, tdiff 1/60",
             "# commit: %s" % a.commit, "# command: python tools/players_bench.py --sizes %s --out profiles/players/step.txt" % a.sizes,
             "# device: %s; torch %s; host CPU thread: 1" % (torch.cuda.get_device_name(0), torch.__version__),
             "# device_us: HIP events around one pwn_players_step_device, median of 20 after 5 warm-ups (lds = as shipped: the walk table staged",
             "#            in LDS; global = PWN_PLAYERS_STAGE=0); host_loop_ms: host/player.c over the n players, one thread;",
             "#            upload_ms: n x 64 B of cameras host -> device, synchronised; host/device = (host_loop + upload) / lds",
             "%9s %5s %12s %12s %14s %11s %12s" % ("n", "ticks", "lds_us", "global_us", "host_loop_ms", "upload_ms", "host/device")]

    ctxs = {}
    for mode, env in (("lds", None), ("global", "0")):
        if env is None:
            os.environ.pop("PWN_PLAYERS_STAGE", None)
        else:
            os.environ["PWN_PLAYERS_STAGE"] = env
        r = pwnfps_amd.Renderer(32, 16)
        r.level_load(level)
        ctxs[mode] = r
    os.environ.pop("PWN_PLAYERS_STAGE", None)

    for n in (int(v) for v in a.sizes.split(",")):
        start = M.corpus_states(data, n, seed=n)
        t0 = tuple(torch.from_numpy(x).to(dev) for x in start)
        t = tuple(x.clone() for x in t0)
        pinned = torch.from_numpy(start[1]).pin_memory()
        for ticks in TICKS:
            us = {}
            for mode, r in ctxs.items():
                samples = []
                for it in range(25):
                    for dst, src in zip(t, t0):
                        dst.copy_(src)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r.players_step_device(t[0], t[1], t[2], t[3], tdiff=1 / 60, ticks=ticks)
                    e1.record()
                    e1.synchronize()
                    if it >= 5:
                        samples.append(e0.elapsed_time(e1) * 1e3)
                us[mode] = statistics.median(samples)
            # (both kernels' results are the model's: a timing of a wrong answer is no timing)
            if n <= 65536:
                want = M.model_step(data, pmap, start[0], 1 / 60, ticks, *start[1:])
                got = tuple(x.cpu().numpy() for x in t[1:])
                assert all((g.view(np.uint32) == w.view(np.uint32)).all() for g, w in zip(got, want)), (n, ticks)
            reps = 3 if n * ticks >= (1 << 26) else 5
            loop, up = [], []
            # (the loop alone: arrays made and touched before the clock starts, host/player.c stepping them in place)
            hd, hp = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(pmap, np.int32)
            for _ in range(reps):
                hs = [np.array(x, order="C") for x in start]
                c0 = time.perf_counter()
                M.model_step_inplace(hd, hp, hs[0], 1 / 60, ticks, hs[1], hs[2], hs[3])
                loop.append((time.perf_counter() - c0) * 1e3)
            for _ in range(7):
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                t[1].copy_(pinned, non_blocking=True)
                torch.cuda.synchronize()
                up.append((time.perf_counter() - c0) * 1e3)
            hl, hu = statistics.median(loop), statistics.median(up[2:])
            lines.append("%9d %5d %12.1f %12.1f %14.3f %11.3f %12.1f" % (n, ticks, us["lds"], us["global"], hl, hu, (hl + hu) * 1e3 / us["lds"]))
            print(lines[-1], flush=True)
    for r in ctxs.values():
        r.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
