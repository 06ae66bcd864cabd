"""The host logic of the row tiling and of the group (pwn_tiled.cpp, pwn_group.cpp and the host API's files they stand on) on the CPU: compiled with g++
against a stand-in HIP runtime and stand-in kernels (tools/sanitize/), run under ThreadSanitizer and AddressSanitizer + UBSan.
Every frame of 2..5 members -- blocking calls, frames in flight delivered and resident, moving cuts, a deep band that leaves the
halo (repeat with whole strips), depth that carries over -- must equal the frame of one context; a member that is late past the
deadline comes back as PWN_ETIMEDOUT and the handle recovers; processes over the shared-memory transport; a call that one
context refuses is refused by a group with the same code and leaves it as it was (`refusals`: the same scripts on one context
and on groups, transcripts equal); a real failure with frames in flight is reported once per lost slot and mended (`lost`).
No GPU needed: the N > 1 host paths run in the CPU suite."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(target, out):
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), target, "OUT=" + out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.parametrize("target,modes", [("tsan", ("group", "late", "shm", "refusals", "lost")), ("asan", ("all",))])
def test_host_logic_under_sanitizers(target, modes, tmp_path):
    out_dir = str(tmp_path)
    _build(target, out_dir)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for m in modes:
        p = subprocess.run([os.path.join(out_dir, "group_" + target), m], capture_output=True, text=True, timeout=600, env=env, cwd=out_dir)
        out = p.stdout + p.stderr
        assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
        assert "Sanitizer" not in out, out[-4000:]
        if m in ("late", "all"):
            assert "one call failed at the deadline" in out
        if m in ("refusals", "all"):
            assert "a group's info unchanged over every refused call" in out
        if m in ("lost", "all"):
            assert "every lost slot's wait failed once, naming a member" in out and out.count("reported once, naming the member") == 3 and "refused by one member only is a failure naming it" in out


def test_host_calls_transcript(tmp_path):
    """What every entry point of the host API sends to the device (tools/sanitize/calls_driver.cpp: runtime calls, launches with
    their parameters, hashes of the outputs, the refusals, the out-of-memory paths) is what tests/golden/host_calls.txt recorded
    before the batch calls' common code was folded -- and, in its sections for the branches of the trace launcher, before the
    launch geometry became a plan and pwn_api.cpp five files -- byte for byte, and the run is clean under AddressSanitizer + UBSan."""
    out_dir = str(tmp_path)
    _build("calls", out_dir)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    level = os.path.join(ROOT, "tests", "golden", "levels", "pwnfps_level.txt")
    p = subprocess.run([os.path.join(out_dir, "calls_asan"), level], capture_output=True, timeout=600, env=env, cwd=out_dir)
    assert p.returncode == 0, (p.stdout[-2000:] + p.stderr[-2000:]).decode(errors="replace")
    assert b"Sanitizer" not in p.stdout + p.stderr, p.stderr[-4000:].decode(errors="replace")
    with open(os.path.join(ROOT, "tests", "golden", "host_calls.txt"), "rb") as f:
        want = f.read()
    if p.stdout != want:
        got, exp = p.stdout.split(b"\n"), want.split(b"\n")
        first = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        call = next((got[i] for i in range(min(first, len(got) - 1), -1, -1) if got[i].startswith(b"==")), b"")
        raise AssertionError("line %d differs, in %r:\n  now      %r\n  recorded %r" % (first + 1, call, got[first:first + 1], exp[first:first + 1]))
