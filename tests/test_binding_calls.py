"""What Renderer's device forms send to the library, and what they refuse before they send anything: golden/host_calls.txt's idiom
one level up.  The renderer is a stand-in (no context) and render.lib a recorder that returns 0, so nothing reaches the library and
no kernel runs; the cases are binding_cases.py's.  golden/binding_calls.txt is the transcript of the accepted cases, recorded from
the render.py BEFORE its device forms were rewritten on shared helpers:

    BINDING_RENDER=<that render.py> BINDING_RECORD=<new transcript> pytest tests/test_binding_calls.py     (on a GPU machine)

BINDING_RENDER alone runs the cases against that file instead of the package's."""
import ctypes as C
import importlib.util
import os
import subprocess

import pytest

import binding_cases as bc
from conftest import GOLD, ROOT

GOLDEN = os.path.join(GOLD, "binding_calls.txt")
RECORD = os.environ.get("BINDING_RECORD")
_state = {}


def _render():
    """the module under test: pwnfps_amd.render, or the file BINDING_RENDER names loaded as a module of the package"""
    if "render" not in _state:
        if not os.path.exists(os.path.join(ROOT, "pwnfps_amd", "libpwnhip.so")):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pwnfps_amd", "csrc")])
        import pwnfps_amd.render
        _state["render"] = pwnfps_amd.render
        path = os.environ.get("BINDING_RENDER")
        if path:
            spec = importlib.util.spec_from_file_location("pwnfps_amd.render_recorded", path)
            _state["render"] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(_state["render"])
    return _state["render"]


def _golden():
    if "golden" not in _state:
        with open(GOLDEN) as f:
            _state["golden"] = dict(line.rstrip("\n").split(": ", 1) for line in f)
    return _state["golden"]


class Recorder:
    """render.lib's stand-in: every function of the ABI table returns 0 and logs its name and arguments"""

    def __init__(self, abi):
        self.log, self.types = [], {name: args for name, _, args in abi}

    def __getattr__(self, name):
        if name == "types" or name not in self.types:
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, args))
            return 0
        fn.__name__ = name
        return fn


def _stand_in(monkeypatch):
    render = _render()
    rec = Recorder(render._lib.ABI)
    monkeypatch.setattr(render, "lib", rec)

    def bare():
        r = object.__new__(render.Renderer)
        r.w, r.h, r.device, r._ctx = bc.W, bc.H, 0, C.c_void_p()
        return r
    r = bare()
    layouts = {bc.LAYOUT: render.ViewportsLayout(r, C.c_void_p(bc.LPTR), bc.LW, bc.LH, bc.LN),
               bc.DEAD: render.ViewportsLayout(r, None, bc.LW, bc.LH, bc.LN),
               bc.FOREIGN: render.ViewportsLayout(bare(), C.c_void_p(bc.LPTR), bc.LW, bc.LH, bc.LN)}
    return r, rec, layouts


def _streams(torch):
    if "streams" not in _state:
        _state["streams"] = torch.cuda.Stream(0), torch.cuda.Stream(0)           # (torch's current stream of a call, the one given)
    return _state["streams"]


def _call(case, r, layouts):
    """the case's call -> (what it returned, the tensors made for it by name, the stream handles by form)"""
    import torch
    method, kwargs = case[1], case[2]
    gpu = bc.needs_gpu(kwargs)
    current, given = _streams(torch) if gpu else (None, None)
    made, args = {}, {}
    for k, v in kwargs.items():
        if isinstance(v, bc.t):
            if v.how == "gpu1" and torch.cuda.device_count() < 2:
                pytest.skip("a tensor on a second GPU")
            v = made[k] = v.make(torch)
        elif isinstance(v, bc.Sym):
            v = given if v is bc.GIVEN else layouts[v]
        args[k] = v
    handles = {"raw": bc.RAW if kwargs.get("stream") == bc.RAW else None, "given": given.cuda_stream if kwargs.get("stream") is bc.GIVEN else None,
               "current": current.cuda_stream if gpu and kwargs.get("stream") is None else None}
    assert not gpu or (current.cuda_stream and given.cuda_stream and current.cuda_stream != given.cuda_stream)
    if gpu:
        with torch.cuda.stream(current):
            ret = getattr(r, method)(**args)
    else:
        ret = getattr(r, method)(**args)
    return ret, made, handles


def _where(p, tensors):
    """a pointer as the tensor it points into plus an offset; one that is absent as None, a raw one of the case's in hex"""
    if not p:
        return "None"
    for name, x in tensors.items():
        if hasattr(x, "data_ptr") and x.data_ptr() and x.data_ptr() <= p < x.data_ptr() + x.numel() * x.element_size():
            return "%s+%d" % (name, p - x.data_ptr())
    return hex(p) if p < 0x10000 else "scratch"


def _transcript(ret, rec, made, handles):
    import torch
    tensors = dict(made)
    for i, x in enumerate(ret if isinstance(ret, tuple) else ()):
        tensors["returned%d" % i] = x
    calls = []
    for name, args in rec.log:
        types = rec.types[name]
        assert len(args) == len(types), name
        out = []
        for i, (a, ty) in enumerate(zip(args, types)):
            ty.from_param(a)                                  # ctypes would take it
            if ty is C.c_void_p:
                p = a.value if isinstance(a, C.c_void_p) else a
                assert p is None or type(p) is int, (name, i, a)
                if i == 0:
                    assert p is None
                    out.append("ctx")
                elif i == len(args) - 1:
                    out.append(([k for k, h in handles.items() if h is not None and h == (p or 0)] + [hex(p or 0)])[0])
                else:
                    out.append(_where(p, tensors))
            else:
                assert type(a) is {C.c_int: int, C.c_float: float}[ty], (name, i, a)
                out.append(repr(a))
        calls.append("%s(%s)" % (name, ", ".join(out)))

    def result(x):
        if isinstance(x, torch.Tensor):
            given = [k for k, v in made.items() if v is x]
            return given[0] if given else "new %s %s %s" % (str(x.dtype)[6:], tuple(x.shape), x.device.type)
        return repr(x)
    res = "(%s)" % ", ".join(result(x) for x in ret) if isinstance(ret, tuple) else result(ret)
    return "; ".join(calls) + " -> " + res


def _params(cases):
    return [pytest.param(c, id=c[0], marks=[pytest.mark.gpu] if bc.needs_gpu(c[2]) else []) for c in cases]


@pytest.mark.parametrize("case", _params(bc.ACCEPTED))
def test_accepted_call_sends_what_the_transcript_says(monkeypatch, case):
    r, rec, layouts = _stand_in(monkeypatch)
    ret, made, handles = _call(case, r, layouts)
    assert len(rec.log) == 1
    line = _transcript(ret, rec, made, handles)
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("%s: %s\n" % (case[0], line))
        return
    assert line == _golden()[case[0]]


@pytest.mark.parametrize("case", _params(bc.REFUSED))
def test_refused_call_raises_before_any_call_into_the_library(monkeypatch, case):
    method, name = case[1], case[3]
    r, rec, layouts = _stand_in(monkeypatch)
    with pytest.raises(ValueError) as e:
        _call(case, r, layouts)
    assert rec.log == []
    msg = str(e.value)
    assert msg.startswith(method + ": "), msg
    if name is not None:
        assert name in msg[len(method) + 2:], msg


@pytest.mark.skipif(bool(RECORD), reason="recording")
def test_the_transcript_holds_the_accepted_cases_and_no_others():
    assert list(_golden()) == [c[0] for c in bc.ACCEPTED]
