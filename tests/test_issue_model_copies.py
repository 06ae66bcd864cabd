"""The region tools (tools/issue_model.py, tools/op_histogram.py) read the units kernel by region, and the segment's regions stand in
it once per bounce depth (trace_segment.inc).  The kernel is cross-compiled once, as the tool compiles it (no GPU needed), and parsed:
every instruction of a segment region belongs to a copy, the copies are the programs they are meant to be (the last one has no
bounce code), and every copy is weighted with its own entries."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def parsed(tmp_path_factory):
    import issue_model as im
    asm = str(tmp_path_factory.mktemp("isa") / "trace_kernel.s")
    im.build_asm(asm)
    return im, im.parse(asm, im.region_maps())


def test_segment_file_is_read_and_its_line_directives_hold():
    import issue_model as im
    marks = im.region_maps()           # (asserts that every #line of trace_segment.inc is copy * COPY_LINES + its own line + 1)
    assert {r for _, r in marks[im.SEGMENT_FILE]} >= {"p_setup", "p_walk_ctl", "p_post", "p_exhausted", "p_jitter"}


def test_every_segment_instruction_has_a_copy(parsed):
    im, ins = parsed
    regions = {reg.split("~")[0] for _, reg, _, _ in ins}
    assert not [r for r in regions if im.in_segment(r) and "@" not in r], regions
    assert not [r for r in regions if not im.in_segment(r) and "@" in r], regions
    for base in ("p_setup", "p_walk_ctl", "p_post", "p_wall", "p_sphere", "w_head", "w_room", "w_portal"):
        assert {base + "@%d" % d for d in range(3)} <= regions, base
    # the last copy cannot bounce
    for base in ("p_floor", "p_sphrefl", "p_jitter"):
        assert {base + "@0", base + "@1"} <= regions and base + "@2" not in regions, base
    # the walk's per-step code is the same size in every copy (the back edge is the loop's alone: entry and exits are p_walk_exit)
    n = [sum(1 for _, reg, cl, _ in ins if reg == "p_walk_ctl@%d" % d and cl in ("full", "half", "quarter")) for d in range(3)]
    assert max(n) - min(n) <= 1 and 0 < min(n) <= 6, n
    assert im.parse.disagree <= 2


def test_every_copy_by_its_own_entries(parsed):
    im, ins = parsed
    regions = {reg for _, reg, _, _ in ins}
    cnt = {"segs": 600, "seg1": 200, "seg2": 100, "wave_steps": 9000, "wsteps1": 3000, "wsteps2": 1000, "jitter": 300, "floor": 90, "wp1": 900,
           "wall": 60}
    e = im.copy_entries(regions, cnt)
    assert [e["p_setup@%d" % d] for d in range(3)] == [300, 200, 100]
    assert [e["p_walk_ctl@%d" % d] for d in range(3)] == [5000, 3000, 1000]
    assert [e["p_jitter@%d" % d] for d in range(2)] == [200, 100]
    assert [e["w_room@%d" % d] for d in range(3)] == [500, 300, 100]          # by the copies' walk iterations
    assert [e["p_floor@%d" % d] for d in range(2)] == [54, 36]                # by the entries of the copies that hold it
    assert [e["p_wall@%d" % d] for d in range(3)] == [30, 20, 10]
    assert all(v == 0 for r, v in e.items() if r.endswith("~slow"))
