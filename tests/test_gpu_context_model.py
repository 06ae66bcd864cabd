"""Random call sequences over every call family, judged by one model (tests/context_model.py): one Renderer per sequence, every
operation record applied to the Renderer and to the Model, every output compared bit for bit (depth as uint32).  What the
sequences cover is asserted on the CPU, from the generator and the oracle alone, by tests/test_context_model.py -- for exactly
the seed list used here, context_model.SEEDS.

A failure names the seed, the index and the record of the failing operation, the first differing coordinates, the number of
operations before it, and the one line that replays exactly that prefix:

    python tests/test_gpu_context_model.py SEED PROFILE N_OPS INDEX

No call here is expected to fault or hang; an expected error is a returned code.  The device forms synchronise their stream before
the comparison and nowhere else.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import context_model as CM
import hit_chain as HC
from conftest import level_path

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Runner:
    """the library's side of a sequence: the Renderer, and the planes of the caller's that the device forms work on"""

    def __init__(self, profile):
        import torch
        import pwnfps_amd
        p = CM.PROFILES[profile]
        self.torch, self.pwn = torch, pwnfps_amd
        self.W, self.H = p["w"], p["h"]
        with _env(p["env"]):                  # (read when a context is created)
            self.r = pwnfps_amd.Renderer(self.W, self.H)
        self.foreign = torch.cuda.Stream()
        z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
        self.dev_z, self.dev_sb, self.dev_work = z(4, self.H, self.W, dt=torch.float32), z(4, self.H, self.W), z(4, self.H, self.W)
        self.rows_pre, self.rows_z, self.rows_out = z(self.H, self.W), z(self.H, self.W, dt=torch.float32), z(self.H, self.W)
        torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        self.r.close()

    def _stream(self, rec):
        return self.foreign if rec["foreign"] else self.torch.cuda.current_stream()

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _full(self, shape, word, as_float=False):
        t = self.torch.full(shape, int(word), dtype=self.torch.int32, device="cuda")
        return t.view(self.torch.float32) if as_float else t

    @staticmethod
    def _down(t):
        return t.cpu().numpy().view(np.uint32)

    def _tables(self):
        return {"form2": self.r.sphere_tables()["form"] == 2}

    # state changes
    def op_level(self, rec, inp):
        self.r.level_load(level_path(rec["level"]))
        return {}

    def op_objects(self, rec, inp):
        self.r.set_objects(inp["spheres"])
        return self._tables()

    def op_obj_new(self, rec, inp):
        return {"ret": self.r.obj_new()}

    def op_obj_set(self, rec, inp):
        self.r.obj_set(rec["obj"], "sphere", *rec["sphere"])
        return {}

    def op_obj_free(self, rec, inp):
        self.r.obj_free(rec["obj"])
        return {}

    def op_prepare(self, rec, inp):
        self.r.level_prepare_render()
        return self._tables()

    def op_blur(self, rec, inp):
        self.r.set_blur_passes(rec["n"])
        return {}

    def op_overlap(self, rec, inp):
        self.r.set_frame_overlap(rec["on"])
        return {}

    def op_counters(self, rec, inp):
        self.r.set_counters(rec["on"])
        return {}

    def op_sched(self, rec, inp):
        self.r.set_scheduler(rec["which"])
        return {}

    def op_unit_order(self, rec, inp):
        self.r.set_unit_order(rec["on"])
        return {}

    def op_strips(self, rec, inp):
        self.r.set_call_strips(rec["n"])
        return {}

    # the families
    def op_frame(self, rec, inp):
        sb, zb = self.r.trace_screen_centred(inp["cams"][0], rec["sec"])
        return {"sbuf": sb, "zbuf": zb, "strips": self.r.call_strips_state()["strips_last"]}

    def op_views(self, rec, inp):
        sb, zb = self.r.trace_views(inp["cams"], np.array(rec["secs"], np.float32))
        return {"sbuf": sb, "zbuf": zb}

    def op_views_dev(self, rec, inp):
        n = len(inp["cams"])
        s = self._stream(rec)
        cams, secs = self._up(inp["cams"].reshape(n, 16)), self._up(np.array(rec["secs"], np.float32))
        self.r.trace_views_device(cams, secs, self.dev_sb[:n], self.dev_z[:n], work=self.dev_work[:n], has_w=rec["has_w"], stream=s)
        s.synchronize()
        return {"sbuf": self._down(self.dev_sb[:n]), "zbuf": self._down(self.dev_z[:n])}

    def op_viewports(self, rec, inp):
        sb, zb = self.r.trace_viewports(inp["rects"], inp["cams"], np.array(rec["secs"], np.float32))
        return {"sbuf": sb, "zbuf": zb}

    def op_rays(self, rec, inp):
        xy = inp["xy"]
        n = len(xy)
        rays, seeds, _ = self.pwn.pixel_rays(self.W, self.H, inp["cams"][0], xy)
        if not rec["dev"]:
            col, z = self.r.trace_rays(rays, seeds, rec["sec"], np.full(n, CM.POISON_Z, np.uint32).view(np.float32))
            return {"col": col, "depth": CM.bits(z)}
        s = self._stream(rec)
        t_rays, t_seeds = self._up(rays), self._up(seeds.view(np.int32))
        t_col, t_z = self._full((n,), CM.POISON_S), self._full((n,), CM.POISON_Z, as_float=True)
        self.r.trace_rays_device(t_rays, t_col, t_z, t_seeds, rec["sec"], has_w=rec["has_w"], stream=s)
        s.synchronize()
        return {"col": self._down(t_col), "depth": self._down(t_z)}

    def op_hits(self, rec, inp):
        xy = inp["xy"]
        rays, _, _ = self.pwn.pixel_rays(self.W, self.H, inp["cams"][0], xy)
        if not rec["dev"]:
            return {"hits": self.r.trace_hits(rays)}
        s = self._stream(rec)
        t_rays, t_hits = self._up(rays), self._full((len(xy), 12), CM.POISON_S)
        self.r.trace_hits_device(t_rays, t_hits, has_w=rec["has_w"], stream=s)
        s.synchronize()
        return {"hits": t_hits.cpu().numpy().view(HC.HIT_DTYPE).reshape(-1)}

    def op_view_hits(self, rec, inp):
        n = len(inp["cams"])
        if not rec["dev"]:
            label, cell, dist = self.r.trace_view_hits(inp["cams"])
            return {"label": label, "cell": cell.view(np.uint32).reshape(n, self.H, self.W), "dist": CM.bits(dist)}
        s = self._stream(rec)
        shape = (n, self.H, self.W)
        cams = self._up(inp["cams"].reshape(n, 16))
        label, cell, dist = self._full(shape, CM.POISON_S), self._full(shape, CM.POISON_S), self._full(shape, CM.POISON_Z, as_float=True)
        self.r.trace_view_hits_device(cams, label, cell, dist, has_w=rec["has_w"], stream=s)
        s.synchronize()
        return {"label": self._down(label), "cell": self._down(cell), "dist": self._down(dist)}

    def op_config(self, rec, inp):
        self.r.frames_config(rec["n"], sbuf=rec["sbuf"], zbuf=rec["zbuf"], surface_scale=rec["surface"])
        return {}

    def op_submit(self, rec, inp):
        self.r.submit_frame(inp["cams"][0], rec["sec"], rec["slot"])
        return {}

    def op_wait(self, rec, inp):
        fr = self.r.wait_frame(rec["slot"])
        out = {"seq": int(fr["seq"]), "sec": CM.bits(np.float32(fr["sec"])).item(),
               "sbuf": fr["sbuf"].copy() if "sbuf" in fr else self.r.read_plane(fr["d_sbuf"]),
               "zbuf": fr["zbuf"].copy() if "zbuf" in fr else self.r.read_plane(fr["d_zbuf"], np.float32)}
        if "surface" in fr:
            out["surface"] = fr["surface"].copy()
        return out

    def op_rows(self, rec, inp):
        s = self._stream(rec)
        ptr = s.cuda_stream
        out = {"blur_err": CM.OK}
        self.r.trace_rows_device(inp["cams"][0], rec["sec"], rec["y0"], rec["y1"], self.rows_pre.data_ptr(), self.rows_z.data_ptr(), ptr)
        try:
            self.r.blur_rows_device(rec["y0"], rec["y1"], self.rows_pre.data_ptr(), self.rows_z.data_ptr(), self.rows_out.data_ptr(), ptr)
        except self.pwn.PwnError as e:
            out["blur_err"] = e.code
        s.synchronize()
        out.update(pre=self._down(self.rows_pre), zbuf=self._down(self.rows_z), out=self._down(self.rows_out))
        return out

    def op_upscale(self, rec, inp):
        return {"pixels": self.r.screen_upscale(None, rec["scale"])}

    def run(self, rec, inp, want):
        try:
            got = getattr(self, "op_" + rec["op"])(rec, inp)
        except self.pwn.PwnError as e:
            return {"err": e.code}
        if "stats" in want:
            st = self.r.stats()
            got["stats"] = {k: int(st[k]) for k in want["stats"]}
        return got


def _first(bad):
    return "%d differ, the first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist())


def differs(want, got):
    """None, or what differs first between the model's outputs and the library's"""
    if want.get("err", CM.OK) != got.get("err", CM.OK):
        return "returned %d, the model says %d" % (got.get("err", CM.OK), want.get("err", CM.OK))
    if "err" in want:
        return None
    for key, w in want.items():
        if key in ("cmp_dy", "none", "sample_xy", "sample_label", "sample_cell"):
            continue
        if key not in got:
            return "no %s" % key
        g = got[key]
        if key == "hits":
            bad = HC.mismatches(g, w, want["cmp_dy"])
            if len(bad):
                return "hits: %d records differ, the first at %d: got %s, the model says %s" % (len(bad), bad[0], g[bad[0]], w[bad[0]])
        elif isinstance(w, np.ndarray):
            if g.shape != w.shape:
                return "%s: shape %s, the model says %s" % (key, g.shape, w.shape)
            bad = CM.bits(g) != CM.bits(w)
            if bad.any():
                at = tuple(np.argwhere(bad)[0])
                return "%s: %s: got %08x, the model says %08x" % (key, _first(bad), CM.bits(g)[at], CM.bits(w)[at])
        elif g != w:
            return "%s: got %r, the model says %r" % (key, g, w)
    if "none" in want:
        # first-hit planes: 0 exactly where the primary ray runs out of steps, no poison left, and the sampled pixels' words
        for key in ("label", "cell"):
            bad = (got[key] == 0) != want["none"] if key == "label" else (want["none"] & (got[key] != 0))
            if bad.any():
                return "%s against the exhausted rays: %s" % (key, _first(bad))
            if (got[key] == np.uint32(CM.POISON_S)).any():
                return "%s: pixels not written: %s" % (key, _first(got[key] == np.uint32(CM.POISON_S)))
            for i, xy in enumerate(want["sample_xy"]):
                g, w = got[key][i][xy[:, 1], xy[:, 0]], want["sample_" + key][i]
                if (g != w).any():
                    k = int(np.flatnonzero(g != w)[0])
                    return "%s: view %d pixel %s: got %08x, the model says %08x" % (key, i, xy[k].tolist(), g[k], w[k])
    return None


def run_sequence(seed, profile, n_ops, upto=None, model=CM.Model):
    """the sequence, or its prefix up to and with operation `upto`, through a Renderer and a Model: None, or the failure's report"""
    ops = CM.generate(seed, n_ops, profile)
    if upto is not None:
        ops = ops[:upto + 1]
    p = CM.PROFILES[profile]
    m = model(p["w"], p["h"])
    run = Runner(profile)
    try:
        for i, rec in enumerate(ops):
            inp = m.inputs(rec)
            want = m.apply(rec, inp)
            got = run.run(rec, inp, want)
            what = differs(want, got)
            if what is not None:
                return ("seed %d (%s), operation %d: %r\n  %s\n  %d operations before it\n  replay: python tests/test_gpu_context_model.py %d %s %d %d"
                        % (seed, profile, i, rec, what, i, seed, profile, n_ops, i))
    finally:
        run.close()
    return None


@pytest.mark.parametrize("seed,profile,n_ops", CM.SEEDS, ids=["seed%d-%s" % (s, p) for s, p, _ in CM.SEEDS])
def test_random_sequence(seed, profile, n_ops, oracle_lib):
    report = run_sequence(seed, profile, n_ops)
    assert report is None, "\n" + report


if __name__ == "__main__":
    oracle = __import__("oracle")
    oracle.build()
    seed, profile, n_ops, index = int(sys.argv[1]), sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    report = run_sequence(seed, profile, n_ops, upto=index)
    print(report if report is not None else "seed %d (%s): operations 0 .. %d agree with the model" % (seed, profile, index))
    sys.exit(1 if report is not None else 0)
