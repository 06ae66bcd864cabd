"""The geometry of a trace launch (pwnfps_amd/csrc/launch_plan.h: units, tile pairs, division constants, grid) on the CPU, held
to the arithmetic of the kernel that relies on it.  tests/launch_plan_driver.cpp prints the plan for a sweep of frame widths,
row counts, resident grids, reserves, PWN_TILE_PAIRS settings, schedulers and batch kinds; the kernel's side -- units_x, rows_all,
tiles_x, single_rows and the item count of trace_kernel.hip, and its quotient __umulhi(n, magic) >> shift -- is restated here."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
FRAME, VIEWS, RAYS, VIEWPORTS = 0, 1, 2, 3
COLS = ("w y0 y1 kind n vp_units resident reserve refill want_cost tile_pairs_in rc tiles_x tiles_total ux_magic ux_shift "
        "views_magic views_shift vp_step0 tile_pairs single tx_magic tx_shift items grid cost_mul cost_div").split()


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lp") / "launch_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "launch_plan_driver.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    plans = np.array([l.split()[1:] for l in out if l.startswith("P ")], dtype=np.int64)
    magics = np.array([l.split()[1:] for l in out if l.startswith("M ")], dtype=np.int64)
    assert plans.shape == (13 * 8 * 4 * 3 * 3 * 2 * 2 * 5, len(COLS)) and magics.shape == (4100, 3)
    return {k: plans[:, i] for i, k in enumerate(COLS)}, magics


def ceil_div(a, b):
    return (a + b - 1) // b


def test_the_plan_is_the_kernels_arithmetic(sweep):
    p, _ = sweep
    assert (p["rc"] == 0).all()
    frame, views, rays, vps = (p["kind"] == k for k in (FRAME, VIEWS, RAYS, VIEWPORTS))
    # trace_kernel.hip
    units_x = (p["w"] + 15) >> 4
    rows_all = (p["y1"] - p["y0"] + 3) >> 2
    tiles_x = (units_x + 1) >> 1
    pairs = p["tile_pairs"] != 0
    single_rows = np.where(pairs, np.minimum(p["single"], rows_all), rows_all)
    units = (single_rows * units_x + tiles_x * (rows_all - single_rows)) * np.where(views, p["n"], 1)
    units = np.where(vps, p["tiles_total"], np.where(rays, (p["n"] + 63) >> 6, units))
    assert (p["items"] == units).all()
    assert (p["tiles_x"] == units_x).all()
    whole = units_x * rows_all * np.where(views, p["n"], 1)
    assert (p["tiles_total"] == np.where(vps, p["vp_units"], np.where(rays, 2, whole))).all()
    # the grid: one item per wave at the most, a workgroup has four waves
    assert (p["grid"] >= 1).all() and (p["grid"] <= p["items"]).all()
    assert (p["grid"] <= ceil_div(p["items"], 4))[p["refill"] == 0].all()
    assert (p["cost_mul"] == p["resident"]).all()
    g = np.where((p["reserve"] > 0) & (p["resident"] > 2 * p["reserve"]), p["resident"] - p["reserve"], p["resident"])
    assert (p["cost_div"] == g).all()
    assert (p["grid"] == np.where(p["refill"] != 0, np.minimum(g, p["items"]), np.minimum(g, ceil_div(p["items"], 4)))).all()
    # tile pairs: frames of the units scheduler without an order only; by the setting; from 16 units per wave of the grid on
    can = frame & (p["refill"] == 0) & (p["want_cost"] == 0)
    assert not pairs[~can].any()
    tp = p["tile_pairs_in"]
    assert not pairs[tp == 0].any() and pairs[can & (tp == 2)].all()
    assert (pairs == (p["tiles_total"] >= 16 * 4 * g))[can & (tp == 1)].all()
    assert pairs[can & (tp == 1)].any() and not pairs[can & (tp == 1)].all()
    # ... and the rows that stay single units: the launch's first round, a fifth of the rows
    on1, on2 = pairs & (tp == 1), pairs & (tp == 2)
    s = p["single"]
    assert (s[on2] == 0).all() and (s[~pairs] == 0).all()
    assert (s <= rows_all)[on1].all()
    assert (s >= np.minimum(rows_all, ceil_div(4 * g, units_x)))[on1].all() and (s >= ceil_div(rows_all, 5))[on1].all()
    assert (s == np.minimum(rows_all, np.maximum(ceil_div(4 * g, units_x), ceil_div(rows_all, 5))))[on1].all()          # (and no more than that)
    # the kernel's search for a ticket's viewport starts at the largest power of two below n
    assert (p["vp_step0"] == np.where(vps, 2, 0)).all()


def quotients(n, magic, shift):
    """trace_kernel.hip: shift >= 0 ? __umulhi(n, magic) >> shift : n"""
    return ((n.astype(np.uint64) * np.uint64(magic)) >> np.uint64(32)) >> np.uint64(shift) if shift >= 0 else n.astype(np.uint64)


def test_every_division_constant_divides_exactly(sweep):
    p, magics = sweep
    seen = {(int(d), int(m), int(s)) for d, m, s in magics}
    units_x = (p["w"] + 15) >> 4
    seen |= set(zip(units_x.tolist(), p["ux_magic"].tolist(), p["ux_shift"].tolist()))
    on = p["tile_pairs"] != 0
    seen |= set(zip(((units_x + 1) >> 1)[on].tolist(), p["tx_magic"][on].tolist(), p["tx_shift"][on].tolist()))
    v = p["kind"] == VIEWS
    seen |= set(zip(p["n"][v].tolist(), p["views_magic"][v].tolist(), p["views_shift"][v].tolist()))
    assert {d for d, _, _ in seen} >= set(range(1, 4101))
    rng = np.random.default_rng(4100)
    rand = rng.integers(0, 1 << 31, 1000)
    for d, magic, shift in sorted(seen):
        # (no shift: the kernel takes the quotient to be n itself, right for a divisor of 1 alone)
        assert (shift < 0) == (d == 1), (d, magic, shift)
        assert 0 <= magic < 1 << 32 and shift < 32
        n = np.concatenate([np.array([0, 1, d - 1, d, d + 1, 1 << 24, (1 << 31) - 1]), rand])
        assert (quotients(n, magic, shift) == (n // d).astype(np.uint64)).all(), (d, magic, shift)
