#!/usr/bin/env python3
"""What pwn_upload_level_device costs (profiles/level_device/bench.txt), the two sides alternating in one run and every figure the
median of 20 with its spread (measuring-on-mi355x):

The call alone and back to back, with a given table and with a derived one, on the three shipped levels' grids, beside the host
route for a grid that lives on the device: the grid and the table copied down into pinned memory, pwn_upload_level, the wait for
its upload.
Device: HIP events around ONE call (its five launches), and around a run of 20 calls, / 20.  Host: a wall clock around the three
legs, ending in a synchronise.  Before a time is printed the state words and pwn_get_level_device are held against the host's level.

    python tools/level_device_bench.py [--commit TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
med = statistics.median


def level_path(name):
    return os.path.join(ROOT, "tests", "golden", "levels", name + ".txt")


def spread(v):
    """the half-width of the middle half of the samples: what a median of 20 moves by from run to run"""
    q = statistics.quantiles(v, n=4)
    return (q[2] - q[0]) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("level_device_bench: no GPU; nothing is measured without one")
    import pwnfps_amd
    dev = torch.device("cuda", 0)
    lines = ["# tools/level_device_bench.py: pwn_upload_level_device", "# commit: %s" % a.commit,
             "# command: python tools/level_device_bench.py --out profiles/level_device/bench.txt",
             "# device: %s; torch %s; every figure the median of 20 (+- half the interquartile range), the two sides alternating in one run" % (torch.cuda.get_device_name(0), torch.__version__),
             "# one_us: HIP events around one call (five launches); run_us: around 20 calls, / 20; host_us: a wall clock around the host route",
             "# (d2h_us the grid and the table down, upload_us pwn_upload_level, wait_us the synchronise behind it); host/device = host_us / run_us"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say("%-14s %-8s %8s %7s %16s %16s %16s %8s %10s %8s %12s" % ("level", "table", "records", "paired", "one_us", "run_us", "host_us", "d2h_us", "upload_us", "wait_us", "host/device"))
    for level in ("pwnfps_level", "synth64", "synth256"):
        rd, rh = pwnfps_amd.Renderer(64, 32), pwnfps_amd.Renderer(64, 32)
        for r in (rd, rh):
            r.level_load(level_path(level))
        data, pmap, _ = rh.get_level()
        for table in ("given", "derived"):
            d_data = torch.from_numpy(data.copy()).to(dev)
            d_pmap = torch.from_numpy(pmap.copy()).to(dev) if table == "given" else None
            p_data = torch.empty((64, 64), dtype=torch.uint8).pin_memory()
            p_pmap = torch.empty((26, 7), dtype=torch.int32).pin_memory()
            d_pm_host = torch.from_numpy(pmap.copy()).to(dev)
            one, run, host, d2h, up, wait = [], [], [], [], [], []
            st = None
            for it in range(25):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                rd.upload_level_device(d_data, d_pmap)
                e[1].record()
                e[2].record()
                for _ in range(20):
                    rd.upload_level_device(d_data, d_pmap)
                e[3].record()
                e[3].synchronize()
                if it == 0:          # (a timing of a wrong answer is no timing)
                    st = rd.level_device_state()
                    got = rd.get_level_device()
                    assert st["verdict"] == 0 and st["in_force"] == 1 and (got[0] == data).all(), st
                    assert table == "derived" or (got[1] == pmap).all()
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                p_data.copy_(d_data, non_blocking=True)
                p_pmap.copy_(d_pm_host, non_blocking=True)
                torch.cuda.synchronize()
                c1 = time.perf_counter()
                rh.upload_level(p_data.numpy(), p_pmap.numpy())
                c2 = time.perf_counter()
                torch.cuda.synchronize()
                c3 = time.perf_counter()
                if it >= 5:
                    one.append(e[0].elapsed_time(e[1]) * 1e3)
                    run.append(e[2].elapsed_time(e[3]) * 1e3 / 20)
                    host.append((c3 - c0) * 1e6); d2h.append((c1 - c0) * 1e6); up.append((c2 - c1) * 1e6); wait.append((c3 - c2) * 1e6)
            pm = lambda v: "%8.1f +- %4.1f" % (med(v), spread(v))
            say("%-14s %-8s %8d %7d %16s %16s %16s %8.1f %10.1f %8.1f %12.1f" % (level, table, st["records"], st["paired"], pm(one), pm(run), pm(host),
                                                                                med(d2h), med(up), med(wait), med(host) / med(run)))
        rd.close()
        rh.close()

    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
