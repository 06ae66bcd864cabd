"""sphere_box.h on the CPU: the box arithmetic that the device's table builder (sphere_bins.hip) shares with the host, compiled with
gcc into tests/sphere_box_driver.c and held, per sphere and over the whole set, to level_host.c's pwn_bin_spheres; the totals
against pwn_sphere_tables_plan.  A few thousand seeded spheres, NaN, the infinities, +-2^31 and one ulp inside, +-1e30, denormal
and negative radii, boxes that straddle 0 and 63, a box over the whole grid.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
F = np.float32
SPHERE = np.dtype([("r", "<f4"), ("refl", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("cb", "<f4"), ("cg", "<f4"), ("cr", "<f4")])


def hostile_values():
    big = F(2.0 ** 31)
    return [np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, F(0)), np.nextafter(-big, F(0)), F(1e30), F(-1e30),
            F(1e-45), F(-1e-45), F(1e-39), F(1e-20), F(-1e-20), F(-0.3), F(-40.0), F(0.0), F(-0.0), F(2.0 ** 24), F(63.0), F(64.0), F(-1.0)]


def spheres():
    rng = np.random.default_rng(2026)
    parts = []
    # seeded: all over and around the grid, radii from tiny to several cells
    n = 3000
    s = np.zeros(n, SPHERE)
    s["x"], s["z"] = rng.uniform(-6, 70, n), rng.uniform(-6, 70, n)
    s["r"] = np.where(rng.random(n) < 0.8, rng.uniform(0.01, 0.9, n), rng.uniform(0.9, 6.0, n))
    parts.append(s)
    # every hostile value as radius, as x and as z, against ordinary and hostile partners
    vals = hostile_values()
    rows = []
    for v in vals:
        for w in (F(0.3), F(10.5), F(63.5), F(-0.2)) + tuple(vals[:9]):
            rows += [(v, 0, w, 0, 10.5, 0, 0, 0), (w, 0, v, 0, 10.5, 0, 0, 0), (0.4, 0, 10.5, 0, v, 0, 0, 0), (v, 0, v, 0, w, 0, 0, 0)]
    parts.append(np.array(rows, dtype=SPHERE))
    # boxes that straddle 0 and 63 on either axis, exactly on the cell edges too; a box over the whole grid
    edge = [(r, 0, x, 0, z, 0, 0, 0) for r in (0.25, 0.5, 1.0, 1.5) for x in (-0.75, -0.25, 0.0, 0.25, 1.0, 62.75, 63.0, 63.25, 63.75, 64.0, 64.25)
            for z in (-0.25, 0.5, 31.0, 63.5, 64.25)]
    parts.append(np.array(edge + [(100.0, 0, 32.0, 0, 32.0, 0, 0, 0), (32.5, 0, 32.0, 0, 32.0, 0, 0, 0), (31.5, 0, 32.0, 0, 32.0, 0, 0, 0)], dtype=SPHERE))
    out = np.concatenate(parts).astype(SPHERE)
    for c in ("refl", "y", "cb", "cg", "cr"):
        out[c] = rng.uniform(0, 1, len(out))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("sphere_box")
    exe = str(d / "sphere_box_driver")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "sphere_box_driver.c"),
                           os.path.join(CSRC, "level_host.c"), "-o", exe, "-lm"])
    return exe, d


def _run(driver, s, name):
    exe, d = driver
    path = str(d / (name + ".bin"))
    np.ascontiguousarray(s, SPHERE).tofile(path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout + p.stderr)[-2000:]
    return tuple(int(v) for v in p.stdout.split()[:3])


def _plan(s):
    from pwnfps_amd import _lib
    out = (C.c_uint64 * 6)()
    rc = _lib.lib.pwn_sphere_tables_plan(np.ascontiguousarray(s, SPHERE).ctypes.data, len(s), out)
    assert rc in (0, -7)
    return int(out[3]), int(out[4]), int(out[5])


def test_box_is_the_hosts_binning(driver):
    s = spheres()
    assert 3000 < len(s) <= 10000 and np.isnan(s["r"]).any() and np.isinf(s["x"]).any()
    got = _run(driver, s, "all")
    assert got == _plan(s)
    assert got[1] == 4096          # (the whole-grid box reaches every cell)


@pytest.mark.parametrize("k", [0, 1, 64, 65])
def test_small_sets(driver, k):
    s = spheres()[:k]
    assert _run(driver, s, "n%d" % k) == (_plan(s) if k else (0, 0, 0))


def test_the_header_is_what_the_kernels_and_the_stand_in_compile():
    """one text: the kernels' file and the sanitizer builds' stand-in include the header, neither restates it"""
    hip = open(os.path.join(CSRC, "sphere_bins.hip")).read()
    fake = open(os.path.join(ROOT, "tools", "sanitize", "fake_kernels.cpp")).read()
    for text in (hip, fake):
        assert '#include "sphere_box.h"' in text and "pwn_box_pack(" in text and "pwn_box_r2(" in text and "2147483648" not in text
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sphere_bins.o: $(HERE)sphere_bins.hip $(HERE)sphere_box.h" in mk
