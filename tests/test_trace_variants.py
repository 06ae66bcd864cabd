"""The one table of the units kernel's variants (pwnfps_amd/csrc/trace_variants.h) and the mode of a launch (launch_plan.h
pwn_launch_mode), without a GPU.  tests/trace_variants_driver.cpp, plain g++, prints every (kernel name, ORDER, LISTS, MODE) the table
declares and the mode of every launch descriptor; the first is held to the kernel symbols of the built library, in both directions,
the second to a table written out here from the launchers as they were before there was one function."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pwnfps_amd", "csrc")
LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")

FRAME, VIEWS, RAYS, HITS, VIEWPORTS, VIEW_HITS, VIEWPORT_HITS, HIDE, REACH = 0, 1, 2, 3, 4, 5, 6, 8, 16
K_FRAME, K_VIEWS, K_RAYS, K_VIEWPORTS = 0, 1, 2, 3          # launch_plan.h PWN_LAUNCH_*
# (kind, label / hits given, hide, reach) -> the mode, or None: no variant.  One legal row per family of entry points of
# include/pwnhip.h, read off the four launchers this table replaced: the frame; pwn_trace_views, _view_hits, _views_hide_device,
# _view_hits_hide_device; pwn_trace_viewports, _viewport_hits and their _hide_device forms; pwn_trace_rays, _hits, _rays_hide_device,
# _hits_hide_device, pwn_trace_reach, _reach_hide_device.  A frame has neither planes of labels nor a hidden sphere, and a reach
# belongs to first-hit records.
EXPECT = {
    (K_FRAME, 0, 0, 0): FRAME,
    (K_FRAME, 0, 1, 0): None,
    (K_FRAME, 1, 0, 0): None,
    (K_FRAME, 1, 1, 0): None,
    (K_VIEWS, 0, 0, 0): VIEWS,
    (K_VIEWS, 0, 1, 0): VIEWS | HIDE,
    (K_VIEWS, 1, 0, 0): VIEW_HITS,
    (K_VIEWS, 1, 1, 0): VIEW_HITS | HIDE,
    (K_VIEWPORTS, 0, 0, 0): VIEWPORTS,
    (K_VIEWPORTS, 0, 1, 0): VIEWPORTS | HIDE,
    (K_VIEWPORTS, 1, 0, 0): VIEWPORT_HITS,
    (K_VIEWPORTS, 1, 1, 0): VIEWPORT_HITS | HIDE,
    (K_RAYS, 0, 0, 0): RAYS,
    (K_RAYS, 0, 0, 1): None,
    (K_RAYS, 0, 1, 0): RAYS | HIDE,
    (K_RAYS, 0, 1, 1): None,
    (K_RAYS, 1, 0, 0): HITS,
    (K_RAYS, 1, 0, 1): HITS | REACH,
    (K_RAYS, 1, 1, 0): HITS | HIDE,
    (K_RAYS, 1, 1, 1): HITS | HIDE | REACH,
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tv") / "trace_variants_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "trace_variants_driver.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    return {k: [l.split()[1:] for l in out if l.startswith(k + " ")] for k in "NVD"}


def test_the_numbers_are_tables_h(printed):
    """trace_variants.h restates the mode and list-form numbers for host tools that cannot include tables.h: the same numbers"""
    tab = open(os.path.join(CSRC, "tables.h")).read()
    assert len(printed["N"]) == 12
    for name, value in printed["N"]:
        assert re.search(r"\b%s = %s\b" % (name, value), tab), name
    got = {n: int(v) for n, v in printed["N"]}
    assert [got["PWN_KM_" + n] for n in "FRAME VIEWS RAYS HITS VIEWPORTS VIEW_HITS VIEWPORT_HITS HIDE REACH".split()] == \
           [FRAME, VIEWS, RAYS, HITS, VIEWPORTS, VIEW_HITS, VIEWPORT_HITS, HIDE, REACH]


def test_the_table_is_the_built_library(printed):
    """every declared variant x COUNT x HAS_W, as a mangled symbol, against the kernel symbols in libpwnhip.so: the same set"""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    rows = [(u, k, int(o), int(l), int(m)) for u, k, o, l, m in printed["V"]]
    assert len(set(rows)) == len(rows)
    assert len({(k, o, l, m) for _, k, o, l, m in rows}) == len(rows)          # no kernel in two units
    per_unit = {u: 4 * sum(1 for r in rows if r[0] == u) for u in ("MAIN", "HIDE", "HIDE_VP", "REACH")}
    assert per_unit == {"MAIN": 92, "HIDE": 36, "HIDE_VP": 36, "REACH": 24}
    assert {r[1] for r in rows if r[0] in ("MAIN", "HIDE")} == {"pwn_trace_kernel"}
    assert {r[1] for r in rows if r[0] == "HIDE_VP"} == {"pwn_trace_hide2_kernel"} and {r[1] for r in rows if r[0] == "REACH"} == {"pwn_trace_reach_kernel"}
    declared = {"_Z%d%sILb%dELb%dELb%dELi%dELi%dEEv16pwn_trace_params" % (len(k), k, c, w, o, l, m)
                for _, k, o, l, m in rows for c in (0, 1) for w in (0, 1)}
    assert len(declared) == 188
    blob = open(LIB, "rb").read()
    built = {s.decode() for s in re.findall(rb"_Z\d+pwn_trace_(?:hide2_|reach_)?kernelI[0-9A-Za-z_]*Ev16pwn_trace_params", blob)}
    assert built == declared, (sorted(built - declared), sorted(declared - built))
    by_name = {n: sum(1 for s in built if re.match(r"_Z\d+%sI" % n, s)) for n in ("pwn_trace_kernel", "pwn_trace_hide2_kernel", "pwn_trace_reach_kernel")}
    assert by_name == {"pwn_trace_kernel": 92 + 36, "pwn_trace_hide2_kernel": 36, "pwn_trace_reach_kernel": 24}


def test_the_mode_of_every_launch(printed):
    got = {tuple(int(x) for x in d[:4]): (None if d[4] == "none" else int(d[4])) for d in printed["D"]}
    assert len(printed["D"]) == 20 and got == EXPECT
    assert sum(1 for v in EXPECT.values() if v is not None) == 15
    # every mode the table holds is the mode of exactly one launch
    assert sorted(v for v in got.values() if v is not None) == sorted({int(m) for _, _, _, _, m in printed["V"]})


def test_the_old_launchers_are_gone():
    gone = re.compile(r"\bpwn_launch_trace_(hide2?|reach)\b")
    for d in (CSRC, os.path.join(ROOT, "tools", "sanitize")):
        for root, _, files in os.walk(d):
            if os.path.basename(root).startswith("build"):
                continue
            for f in files:
                if f.endswith((".o", ".so")):
                    continue
                text = open(os.path.join(root, f), errors="replace").read()
                assert not gone.search(text), os.path.join(root, f)
