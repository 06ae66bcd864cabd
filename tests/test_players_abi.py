"""pwn_players_step without a GPU: the exports, bindings and header entries, the PWN_MOVE_* bits against host/player.h's PWN_KEY_*,
the C entries' argument checks that need no context, Renderer's shape, dtype and alignment checks before it calls into the library,
players_spawn against pwn_player_init, and the new kernel in the built library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")
PWN_EINVAL = -1
ENTRIES = ("pwn_players_step", "pwn_players_step_device")
MOVES = ("TURN_LEFT", "TURN_RIGHT", "TURN_UP", "TURN_DOWN", "FORWARD", "BACK", "LEFT", "RIGHT")
KEYS = ("LEFT", "RIGHT", "UP", "DOWN", "W", "S", "A", "D")


def _lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
    from pwnfps_amd import _lib as binding
    return binding.lib


def test_entries_are_exported_bound_and_declared():
    _lib()
    raw = C.CDLL(LIB)
    from pwnfps_amd import _lib as binding
    import pwnfps_amd
    names = {n for n, _, _ in binding.ABI}
    hdr = open(os.path.join(ROOT, "include", "pwnhip.h")).read()
    for e in ENTRIES:
        assert hasattr(raw, e), e
        assert e in names, e
        assert re.search(r"^int %s\(" % e, hdr, re.M), e
    for m in ("players_step", "players_step_device"):
        assert callable(getattr(pwnfps_amd.Renderer, m)), m
    assert callable(pwnfps_amd.players_spawn)
    for i, m in enumerate(MOVES):
        assert getattr(pwnfps_amd, "PWN_MOVE_" + m) == 1 << i
    assert pwnfps_amd.PWN_PLAYERS_MAX == 1 << 20 and pwnfps_amd.PWN_TICKS_MAX == 1024


def test_move_bits_are_the_key_fields(tmp_path):
    """a C program with both headers: PWN_MOVE_* == 1 << PWN_KEY_* for all eight, and pwn_keys has its fields in that order"""
    src = tmp_path / "moves.c"
    checks = "".join('\t_Static_assert(PWN_MOVE_%s == 1 << PWN_KEY_%s, "%s");\n' % (m, k, m) for m, k in zip(MOVES, KEYS))
    src.write_text('#include <stddef.h>\n#include "pwnhip.h"\n#include "player.h"\nint main(void) {\n' + checks +
                   '\t_Static_assert(offsetof(pwn_keys, moveright) == 7 * sizeof(int), "eight ints");\n'
                   '\t_Static_assert(PWN_PLAYERS_MAX == 1 << 20 && PWN_TICKS_MAX == 1024, "limits");\n\treturn 0;\n}\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "host"), str(src), "-o", str(tmp_path / "moves")])
    subprocess.check_call([str(tmp_path / "moves")])


def test_c_entries_refuse_bad_arguments_without_a_context():
    lib = _lib()
    n = 4
    keys = np.zeros(n, np.uint8)
    buf = np.zeros(64 * n, np.float32)          # 16-byte aligned at its start (numpy allocates so); room for every array
    base = buf.ctypes.data
    assert base % 16 == 0
    cams, grav, trav = base, base + 64 * n, base + 80 * n
    k = keys.ctypes.data
    # a NULL context refuses whatever else is given; the rest of the list is then told apart on the GPU (tests/test_gpu_players.py)
    for args in [(None, n, k, 1 / 60, 1, cams, grav, trav), (None, 0, None, 1 / 60, 1, None, None, None),
                 (None, -1, k, 1 / 60, 1, cams, grav, trav), (None, (1 << 20) + 1, k, 1 / 60, 1, cams, grav, trav),
                 (None, n, k, 1 / 60, 0, cams, grav, trav), (None, n, k, 1 / 60, 1025, cams, grav, trav),
                 (None, n, k, float("nan"), 1, cams, grav, trav), (None, n, k, float("inf"), 1, cams, grav, trav),
                 (None, n, None, 1 / 60, 1, cams, grav, trav), (None, n, k, 1 / 60, 1, None, grav, trav), (None, n, k, 1 / 60, 1, cams, None, trav)]:
        assert lib.pwn_players_step(*args) == PWN_EINVAL, args
        assert lib.pwn_players_step_device(*args, None) == PWN_EINVAL, args
    assert lib.pwn_players_step_device(None, n, k, 1 / 60, 1, cams + 4, grav, trav, None) == PWN_EINVAL
    assert lib.pwn_players_step_device(None, n, k, 1 / 60, 1, cams, grav, trav + 2, None) == PWN_EINVAL
    assert lib.pwn_players_step_device(None, n, k, 1 / 60, 1, cams, cams + 16, trav, None) == PWN_EINVAL


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("called into the library: " + name)


def _bare_renderer(monkeypatch=None):
    import pwnfps_amd
    from pwnfps_amd import render
    if monkeypatch is not None:
        monkeypatch.setattr(render, "lib", _NoCall())
    r = object.__new__(pwnfps_amd.Renderer)
    r.w, r.h, r.device, r._ctx = 8, 4, 0, C.c_void_p()
    return r


def _good(n=3):
    return dict(keys=np.zeros(n, np.uint8), cams=np.zeros((n, 16), np.float32), gravity=np.zeros((n, 4), np.float32), traversals=np.zeros(n, np.int32))


@pytest.mark.parametrize("change", [
    dict(keys=np.zeros(3, np.int32)), dict(keys=np.zeros(2, np.uint8)), dict(keys=np.zeros((3, 1), np.uint8)),
    dict(cams=np.zeros((3, 15), np.float32)), dict(cams=np.zeros(48, np.float32)), dict(cams=np.zeros((3, 3, 4), np.float32)),
    dict(gravity=np.zeros((3, 3), np.float32)), dict(gravity=np.zeros((2, 4), np.float32)), dict(traversals=np.zeros(4, np.int32)),
    dict(ticks=0), dict(ticks=1025), dict(ticks=1.5), dict(tdiff=float("nan")), dict(tdiff=float("inf")), dict(tdiff=1e39),
    dict(keys=np.zeros((1 << 20) + 1, np.uint8), cams=np.zeros(((1 << 20) + 1, 16), np.float32), gravity=np.zeros(((1 << 20) + 1, 4), np.float32), traversals=None),
])
def test_players_step_rejects_bad_arguments_before_the_call(monkeypatch, change):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.players_step(**dict(_good(), **change))


def test_players_step_passes_good_arguments_to_the_library():
    """(with no context behind it the library answers PWN_EINVAL: the call got through, and the arguments are left as they were)"""
    import pwnfps_amd
    r = _bare_renderer()
    for kw in (_good(), dict(_good(), cams=np.ones((3, 4, 4), np.float64), traversals=None, ticks=1024, tdiff=0.0)):
        before = {k: np.array(v) for k, v in kw.items() if isinstance(v, np.ndarray)}
        with pytest.raises(pwnfps_amd.PwnError) as e:
            r.players_step(**kw)
        assert e.value.code == PWN_EINVAL
        assert all((kw[k] == v).all() for k, v in before.items())


def _device_cases():
    import torch
    n = 3
    t = dict(keys=torch.zeros(n, dtype=torch.uint8), cams=torch.zeros((n, 16)), gravity=torch.zeros((n, 4)), traversals=torch.zeros(n, dtype=torch.int32))
    return [
        _good(),                                            # numpy arrays are not taken
        t,                                                  # tensors, but not on a GPU
        dict(t, cams=123),                                  # raw pointers are not taken
        dict(t, gravity=np.zeros((n, 4), np.float32)),      # one numpy array among tensors
        dict(t, keys=None),
    ]
# (what the wrapper says of dtype, shape, contiguity, the device and the alignment of GPU tensors needs GPU tensors:
# tests/test_gpu_players.py test_python_refuses_before_the_library_is_entered)


@pytest.mark.parametrize("case", range(5))
def test_players_step_device_rejects_bad_arguments_before_the_call(monkeypatch, case):
    r = _bare_renderer(monkeypatch)
    with pytest.raises(ValueError):
        r.players_step_device(**_device_cases()[case])


def test_players_spawn_is_pwn_player_init():
    import pwnfps_amd
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), os.path.join(ROOT, "host", "libpwnplayer.so")])
    L = C.CDLL(os.path.join(ROOT, "host", "libpwnplayer.so"))

    class Player(C.Structure):
        _fields_ = [("cam", C.c_float * 16), ("gravity", C.c_float * 4), ("traversals", C.c_int)]
    p = Player()
    spawn = np.array([9, 4], np.int32)
    L.pwn_player_init(C.byref(p), C.c_void_p(spawn.ctypes.data))
    cams, grav, trav = pwnfps_amd.players_spawn(spawn, 5)
    assert cams.shape == (5, 16) and cams.dtype == np.float32 and grav.shape == (5, 4) and trav.shape == (5,) and trav.dtype == np.int32
    assert (cams == np.array(list(p.cam), np.float32)).all() and (grav == np.array(list(p.gravity), np.float32)).all() and (trav == p.traversals).all()


def test_library_holds_the_step_kernel_built_without_the_flush():
    """both instantiations (walk table from device memory, and staged in LDS) are registered under their mangled names, and the
    Makefile gives player_step.hip view_setup.hip's flags"""
    _lib()
    blob = open(LIB, "rb").read()
    found = set(re.findall(rb"_Z23pwn_players_step_kernelILb([01])EEv", blob))
    assert found == {b"0", b"1"}, sorted(found)
    mk = open(os.path.join(ROOT, "pwnfps_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^\$\(B\)/player_step\.o:.*\n(?:\t.*\n)+", mk, re.M)
    assert rule and "$(VIEW_SETUP_FLAGS)" in rule.group(0)
    assert "player_step.o" in re.search(r"^OBJ = .*$", mk, re.M).group(0)
