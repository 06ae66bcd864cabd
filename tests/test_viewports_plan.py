"""pwn_viewports_plan without a GPU: the units and pixels of hand-computed layouts, every cause of PWN_EINVAL with out[3]
naming the offender, the blur-only rules, the binding -- and the stand-alone fuzz program of tools/sanitize/ under
AddressSanitizer + UBSan (its own main, nothing preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
OK, EINVAL = 0, -1
VIEWS_MAX = 1024


def _lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    lib = C.CDLL(LIB)
    lib.pwn_viewports_plan.restype = C.c_int
    lib.pwn_viewports_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _plan(W, H, blur, rects, n=None):
    r = np.ascontiguousarray(np.array(rects, np.int32).reshape(-1, 4))
    out = np.full(4, 0xdeadbeef, np.uint64)
    rc = _lib().pwn_viewports_plan(W, H, blur, len(r) if n is None else n, r.ctypes.data, out.ctypes.data)
    return rc, [int(v) for v in out]


def test_units_and_pixels_of_hand_computed_layouts():
    # one rectangle: ceil(w / 16) * ceil(h / 4) units
    assert _plan(640, 480, 0, [(0, 0, 1, 1)]) == (OK, [1, 1, 1, 1])
    assert _plan(640, 480, 0, [(5, 7, 17, 5)]) == (OK, [2 * 2, 85, 4, 1])
    assert _plan(640, 480, 0, [(0, 0, 16, 4)]) == (OK, [1, 64, 1, 1])
    assert _plan(640, 480, 1, [(0, 0, 640, 480)]) == (OK, [40 * 120, 640 * 480, 4800, 1])
    # w = 1, w = 17, h = 5 side by side: 1 * 2 + 2 * 2 + 3 * 1
    assert _plan(100, 50, 0, [(0, 0, 1, 5), (1, 0, 17, 5), (18, 0, 40, 4)]) == (OK, [2 + 4 + 3, 5 + 85 + 160, 4, 3])
    # the issue's layout L1: 336 x 208, full cover, blur-legal
    L1 = [(0, 0, 160, 100), (160, 0, 176, 100), (0, 100, 100, 108), (100, 100, 36, 38), (136, 100, 4, 4), (136, 104, 4, 104),
          (100, 138, 36, 70), (140, 100, 196, 108)]
    units = [10 * 25, 11 * 25, 7 * 27, 3 * 10, 1, 26, 3 * 18, 13 * 27]
    for blur in (0, 1, 2):
        assert _plan(336, 208, blur, L1) == (OK, [sum(units), 336 * 208, max(units), 8])
    # L2: gaps, blur off only
    L2 = [(1, 1, 1, 1), (3, 0, 17, 5), (21, 2, 33, 3), (55, 7, 277, 193), (0, 10, 50, 190)]
    units = [1, 2 * 2, 3 * 1, 18 * 49, 4 * 48]
    assert _plan(333, 201, 0, L2) == (OK, [sum(units), 1 + 85 + 99 + 277 * 193 + 50 * 190, 18 * 49, 5])
    assert _plan(333, 201, 1, L2)[0] == EINVAL


def test_touching_rectangles_are_accepted():
    assert _plan(64, 64, 1, [(0, 0, 32, 32), (32, 0, 32, 32), (0, 32, 32, 32), (32, 32, 32, 32)]) == (OK, [4 * 16, 4096, 16, 4])
    assert _plan(10, 10, 0, [(0, 0, 5, 10), (5, 0, 5, 10)])[0] == OK
    assert _plan(10, 10, 0, [(3, 3, 1, 1), (4, 3, 1, 1), (3, 4, 1, 1), (4, 4, 1, 1)])[0] == OK


@pytest.mark.parametrize("blur", [0, 1])
def test_every_cause_of_einval_names_the_offender(blur):
    good = [(0, 0, 32, 32), (32, 0, 32, 32), (0, 32, 64, 32)]
    assert _plan(64, 64, blur, good) == (OK, [2 * 16 + 4 * 8, 4096, 32, 3])

    def bad(rects, who, W=64, H=64):
        rc, out = _plan(W, H, blur, rects)
        assert rc == EINVAL and out[3] == who, (rects, rc, out)

    # overlap by one pixel (a corner; a column; the later rectangle is the offender)
    bad([(0, 0, 32, 32), (28, 31, 32, 32), (0, 32, 28, 32)], 1)
    bad([(0, 0, 32, 32), (32, 0, 32, 32), (0, 28, 64, 36)], 2)
    bad([(0, 0, 36, 32), (32, 0, 32, 32)], 1)
    bad([(0, 0, 32, 32), (0, 0, 32, 32)], 1)
    bad([(0, 0, 64, 64), (20, 20, 4, 4)], 1)          # one inside the other
    # one pixel outside the frame, on each side
    bad([(0, 0, 32, 32), (36, 0, 32, 32)], 1)
    bad([(0, 0, 32, 32), (32, 33, 32, 32)], 1)
    bad([(-4, 0, 32, 32)], 0)
    bad([(0, 0, 32, 32), (0, -1, 32, 32)], 1)
    bad([(0, 0, 68, 64)], 0)
    bad([(0, 0, 64, 65)], 0)
    # empty and negative sizes
    bad([(0, 0, 32, 32), (32, 0, 0, 32)], 1)
    bad([(0, 0, 32, 0)], 0)
    bad([(0, 0, 32, 32), (32, 0, 32, 32), (0, 32, -4, 32)], 2)
    # values that would wrap in 32 bits
    bad([(2 ** 31 - 1, 0, 2 ** 31 - 1, 4)], 0)
    bad([(0, 0, 32, 32), (4, 2 ** 31 - 4, 8, 8)], 1)
    bad([(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)], 0)
    # the first offender is the one reported
    bad([(0, 0, 32, 32), (32, 0, 0, 32), (0, 0, 32, 32)], 1)
    # n and the pointers: no rectangle is the offender
    lib = _lib()
    out = np.zeros(4, np.uint64)
    r = np.array(good, np.int32)
    assert lib.pwn_viewports_plan(64, 64, blur, 0, r.ctypes.data, out.ctypes.data) == EINVAL and list(out) == [0, 0, 0, 0]
    assert lib.pwn_viewports_plan(64, 64, blur, -5, r.ctypes.data, out.ctypes.data) == EINVAL and list(out) == [0, 0, 0, 0]
    many = np.zeros((VIEWS_MAX + 1, 4), np.int32)
    many[:, 0] = np.arange(VIEWS_MAX + 1) % 64 * 4
    many[:, 1] = np.arange(VIEWS_MAX + 1) // 64 * 4
    many[:, 2:] = 4
    assert lib.pwn_viewports_plan(256, 128, blur, VIEWS_MAX + 1, many.ctypes.data, out.ctypes.data) == EINVAL
    assert list(out) == [0, 0, 0, VIEWS_MAX + 1]
    assert lib.pwn_viewports_plan(256, 128, blur, VIEWS_MAX, many.ctypes.data, out.ctypes.data) == OK
    assert list(out) == [VIEWS_MAX, VIEWS_MAX * 16, 1, VIEWS_MAX]
    assert lib.pwn_viewports_plan(64, 64, blur, 3, None, out.ctypes.data) == EINVAL and list(out) == [0, 0, 0, 3]
    assert lib.pwn_viewports_plan(64, 64, blur, 3, r.ctypes.data, None) == EINVAL
    # the frame itself
    for W, H in ((0, 64), (64, 0), (-64, 64), (32769, 64), (64, 32769)):
        rc, o = _plan(W, H, blur, [(0, 0, 4, 4)])
        assert rc == EINVAL, (W, H)


def test_blur_rules_apply_with_blur_on_only():
    cases = [
        (64, 64, [(0, 0, 32, 64), (34, 0, 28, 64)], 1),          # x % 4
        (64, 64, [(0, 0, 30, 64), (32, 0, 32, 64)], 0),          # w % 4
        (64, 64, [(0, 0, 32, 64), (32, 0, 31, 64)], 1),
        (64, 64, [(1, 1, 1, 1)], 0),
    ]
    for W, H, rects, who in cases:
        for blur in (1, 2, 7):
            rc, out = _plan(W, H, blur, rects)
            assert rc == EINVAL and out[3] == who, (rects, blur, out)
        rc, out = _plan(W, H, 0, rects)
        assert rc == OK and out[3] == len(rects), (rects, out)
        assert _plan(W, H, -1, rects)[0] == OK
    # W % 4 with blur on: the frame, not a rectangle -- out[3] = n and nothing is counted
    rects = [(0, 0, 32, 64), (32, 0, 28, 64)]
    assert _plan(62, 64, 1, rects) == (EINVAL, [0, 0, 0, 2])
    assert _plan(62, 64, 0, rects) == (OK, [2 * 16 + 2 * 16, 60 * 64, 32, 2])
    # y and h are free
    assert _plan(64, 64, 1, [(0, 1, 32, 3), (0, 5, 32, 7), (32, 3, 32, 61)])[0] == OK


def test_binding():
    import pwnfps_amd
    from pwnfps_amd import _lib as binding
    assert {"pwn_viewports_plan", "pwn_trace_viewports"} <= {n for n, _, _ in binding.ABI}
    assert C.sizeof(binding.Viewport) == 16
    p = pwnfps_amd.viewports_plan(64, 64, [(0, 0, 32, 32), (32, 0, 17, 5)], 0)
    assert p == {"ok": True, "units": 16 + 4, "pixels": 1024 + 85, "largest": 16, "offender": 2}
    p = pwnfps_amd.viewports_plan(64, 64, [(0, 0, 32, 32), (32, 0, 17, 5)], 1)
    assert not p["ok"] and p["offender"] == 1
    with pytest.raises(ValueError):
        pwnfps_amd.viewports_plan(64, 64, [(0, 0, 32)], 0)
    # Renderer.trace_viewports refuses badly shaped arguments before it calls into the library, and passes good ones on
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    for rects, cams, secs in (([(0, 0, 4, 4)], np.zeros((2, 16)), [0.0]), ([(0, 0, 4)], np.zeros((1, 16)), [0.0]),
                              ([(0, 0, 4, 4)], np.zeros((1, 16)), [0.0, 1.0]), (np.zeros((0, 4)), np.zeros((0, 16)), [])):
        with pytest.raises(ValueError):
            r.trace_viewports(rects, cams, secs)
    with pytest.raises(pwnfps_amd.PwnError) as e:
        r.trace_viewports([(0, 0, 4, 4), (4, 0, 4, 4)], np.zeros((2, 4, 4)), [0.0, 1.0])
    assert e.value.code == EINVAL            # (no context behind it)


def test_fuzz_under_asan_ubsan(tmp_path):
    """tools/sanitize/fuzz_viewports.c: random small layouts against a painted grid, hostile values, n at its limits"""
    out_dir = str(tmp_path)
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "viewports", "OUT=" + out_dir],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(out_dir, "fuzz_viewports")], capture_output=True, text=True, timeout=300, env=env, cwd=out_dir)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
