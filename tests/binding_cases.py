"""The cases of test_binding_calls.py: calls of Renderer's device forms on a stand-in renderer of 8 x 4 pixels whose library is a
recorder.  ACCEPTED: (id, method, kwargs) -- the call reaches the library, and the transcript of what it passes is
golden/binding_calls.txt.  REFUSED: (id, method, kwargs, name) -- exactly one fault, ValueError before any call into the library,
the message names parameter `name` unless that is None.  Tensors are described (class t) and made by the test; a case without a
GPU tensor runs without a GPU."""
import numpy as np

W, H, N, R, P = 8, 4, 2, 4, 3               # the renderer's frame; views, rays and players of a call
LW, LH, LN, LPTR = 16, 8, 2, 0x1000         # the layout: ViewportsLayout(r, c_void_p(LPTR), LW, LH, LN)
WORK = 20                                   # PWN_PIXEL_WORK_BYTES / 4
RAYS_MAX, OBJ_MAX = 1 << 28, 10000


class Sym:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<%s>" % self.name


LAYOUT, DEAD, FOREIGN = Sym("layout"), Sym("dead layout"), Sym("another renderer's layout")
GIVEN = Sym("a torch.cuda.Stream")          # stream=GIVEN; stream=RAW is a raw handle, stream=None torch's current stream
RAW = 0x5000


class t:
    """A tensor of `dtype` and `shape`.  how: "gpu" (zeros on cuda:0, aligned), "off4" (the same, starting 4 bytes past an aligned
    address), "strided" (not contiguous), "cpu", "numpy", "gpu1" (on cuda:1)."""

    def __init__(self, dtype, *shape, how="gpu"):
        self.dtype, self.shape, self.how = dtype, tuple(shape), how

    def but(self, **kw):
        d = t(self.dtype, *self.shape, how=self.how)
        d.__dict__.update(kw)
        return d

    def needs_gpu(self):
        return self.how not in ("cpu", "numpy")

    def make(self, torch):
        if self.how == "numpy":
            return np.zeros(self.shape, self.dtype)
        dtype = getattr(torch, self.dtype)
        if self.how == "cpu":
            return torch.zeros(self.shape, dtype=dtype)
        dev = "cuda:1" if self.how == "gpu1" else "cuda:0"
        if self.how == "off4":
            size = int(np.prod(self.shape))
            k = 4 // np.dtype(self.dtype).itemsize
            x = torch.zeros(size + k, dtype=dtype, device=dev)[k:].view(self.shape)
            assert x.data_ptr() % 16 == 4 and x.is_contiguous()
            return x
        if self.how == "strided":
            x = torch.zeros(self.shape[:-1] + (2 * self.shape[-1],), dtype=dtype, device=dev)[..., ::2]
            assert tuple(x.shape) == self.shape and not x.is_contiguous()
            return x
        return torch.zeros(self.shape, dtype=dtype, device=dev)


def needs_gpu(kwargs):
    return any(isinstance(v, t) and v.needs_gpu() for v in kwargs.values()) or kwargs.get("stream") is GIVEN


F, I, U, S, B = "float32", "int32", "uint32", "int16", "uint8"
WRONG = {F: "float64", I: "int64", U: "float32", S: "int64", B: "int8"}

# per method: the kwargs of a plain accepted call, and per tensor parameter (alignment the binding holds it to, how a wrong row
# count shows: "named" in the message, "other" = it sets n, so another parameter is blamed, None = any count is right)
BASE = {
    "trace_views_device": (dict(cams=t(F, N, 16), secs=t(F, N), sbuf=t(I, N, H, W), zbuf=t(F, N, H, W)),
                           dict(cams=(4, "other"), secs=(4, "named"), sbuf=(4, "named"), zbuf=(4, "named"), work=(4, "named"), hide=(4, "named"))),
    "trace_viewports_device": (dict(layout=LAYOUT, cams=t(F, LN, 16), secs=t(F, LN), sbuf=t(I, LH, LW), zbuf=t(F, LH, LW)),
                               dict(cams=(16, "named"), secs=(16, "named"), sbuf=(16, "named"), zbuf=(16, "named"), work=(16, "named"),
                                    hide=(4, "named"))),
    "trace_rays_device": (dict(rays=t(F, R, 8), col=t(I, R), depth=t(F, R)),
                          dict(rays=(16, "other"), col=(4, "named"), depth=(4, "named"), seeds=(4, "named"), hide=(4, "named"))),
    "trace_hits_device": (dict(rays=t(F, R, 8), hits=t(I, R, 12)), dict(rays=(16, "other"), hits=(16, "named"), hide=(4, "named"))),
    "trace_reach_device": (dict(rays=t(F, R, 8), reach=t(F, R), hits=t(I, R, 12)),
                           dict(rays=(16, "other"), reach=(4, "named"), hits=(16, "named"), hide=(4, "named"))),
    "trace_view_hits_device": (dict(cams=t(F, N, 16), label=t(I, N, H, W)),
                               dict(cams=(16, "other"), label=(16, "named"), cell=(16, "named"), dist=(16, "named"), hide=(4, "named"))),
    "trace_viewport_hits_device": (dict(layout=LAYOUT, cams=t(F, LN, 16), label=t(I, LH, LW)),
                                   dict(cams=(16, "named"), label=(16, "named"), cell=(16, "named"), dist=(16, "named"), hide=(4, "named"))),
    "players_step_device": (dict(keys=t(B, P), cams=t(F, P, 16), gravity=t(F, P, 4)),
                            dict(keys=(1, "named"), cams=(16, "other"), gravity=(16, "named"), traversals=(4, "named"))),
    "pixel_rays_device": (dict(cams=t(F, N, 16)),
                          dict(cams=(16, "other"), xy=(8, None), rays=(16, "named"), seeds=(4, "named"), work=(16, "named"))),
    "upload_spheres_device": (dict(spheres=t(F, P, 8), max_pairs=100), dict(spheres=(16, None))),
}
# the optional tensors, as a call that is accepted gives them
OPTIONAL = {
    "trace_views_device": dict(work=t(I, N, H, W), hide=t(I, N)),
    "trace_viewports_device": dict(work=t(I, LH, LW), hide=t(I, LN)),
    "trace_rays_device": dict(seeds=t(I, R), hide=t(I, R)),
    "trace_hits_device": dict(hide=t(I, R)),
    "trace_reach_device": dict(hide=t(I, R)),
    "trace_view_hits_device": dict(cell=t(I, N, H, W), dist=t(F, N, H, W), hide=t(I, N)),
    "trace_viewport_hits_device": dict(cell=t(I, LH, LW), dist=t(F, LH, LW), hide=t(I, LN)),
    "players_step_device": dict(traversals=t(I, P)),
    "pixel_rays_device": dict(xy=t(I, 3, 2), rays=t(F, N * W * H, 8), seeds=t(I, N * W * H), work=t(F, N, WORK)),
    "upload_spheres_device": {},
}

_M = W * H
# per method: (tag, the kwargs that differ from the plain call)
VARIANTS = {
    "trace_views_device": [
        ("cams44", dict(cams=t(F, N, 4, 4))), ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, N))), ("work", dict(work=t(I, N, H, W))),
        ("uint32", dict(sbuf=t(U, N, H, W), work=t(U, N, H, W))), ("all", dict(cams=t(F, N, 4, 4), has_w=True, hide=t(I, N), work=t(I, N, H, W))),
        ("one_view", dict(cams=t(F, 1, 16), secs=t(F, 1), sbuf=t(I, 1, H, W), zbuf=t(F, 1, H, W)))],
    "trace_viewports_device": [
        ("cams44", dict(cams=t(F, LN, 4, 4))), ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, LN))), ("work", dict(work=t(I, LH, LW))),
        ("uint32", dict(sbuf=t(U, LH, LW), work=t(U, LH, LW))), ("all", dict(cams=t(F, LN, 4, 4), has_w=True, hide=t(I, LN), work=t(I, LH, LW)))],
    "trace_rays_device": [
        ("n0", dict(rays=t(F, 0, 8), col=t(I, 0), depth=t(F, 0))), ("n0_hide", dict(rays=t(F, 0, 8), col=t(I, 0), depth=t(F, 0), hide=t(I, 0))),
        ("seeds", dict(seeds=t(I, R))), ("uint32", dict(col=t(U, R), seeds=t(U, R))), ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, R))),
        ("sec", dict(sec_current=1.5)), ("n_given", dict(n=R)), ("all", dict(seeds=t(I, R), hide=t(I, R), has_w=True, sec_current=2, n=R)),
        ("pointers", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R)), ("pointers_stream", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R, stream=RAW)),
        ("pointers_seeds", dict(rays=0x2000, col=0x3000, depth=0x4000, seeds=0x6000, n=R, has_w=True, sec_current=0.25)),
        ("pointers_n0", dict(rays=0x2000, col=0x3000, depth=0x4000, n=0)), ("pointers_none", dict(rays=None, col=None, depth=None, n=R)),
        ("pointers_hide", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R, hide=t(I, R))),
        ("pointers_hide_stream", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R, hide=t(I, R), stream=RAW))],
    "trace_hits_device": [
        ("n0", dict(rays=t(F, 0, 8), hits=t(I, 0, 12))), ("float32", dict(hits=t(F, R, 12))), ("uint8", dict(hits=t(B, R, 48))),
        ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, R))), ("n_given", dict(n=R)), ("all", dict(hide=t(I, R), has_w=True, n=R)),
        ("pointers", dict(rays=0x2000, hits=0x3000, n=R)), ("pointers_stream", dict(rays=0x2000, hits=0x3000, n=R, stream=RAW, has_w=True)),
        ("pointers_n0", dict(rays=0x2000, hits=0x3000, n=0)), ("pointers_hide", dict(rays=0x2000, hits=0x3000, n=R, hide=t(I, R)))],
    "trace_reach_device": [
        ("n0", dict(rays=t(F, 0, 8), reach=t(F, 0), hits=t(I, 0, 12))), ("float32", dict(hits=t(F, R, 12))), ("uint8", dict(hits=t(B, R, 48))),
        ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, R))), ("all", dict(hide=t(I, R), has_w=True))],
    "trace_view_hits_device": [
        ("cams44", dict(cams=t(F, N, 4, 4))), ("uint32", dict(label=t(U, N, H, W), cell=t(U, N, H, W))), ("cell_words", dict(cell=t(I, N, H, W))),
        ("cell_pairs", dict(cell=t(S, N, H, W, 2))), ("dist", dict(dist=t(F, N, H, W))), ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, N))),
        ("all", dict(cams=t(F, N, 4, 4), cell=t(S, N, H, W, 2), dist=t(F, N, H, W), hide=t(I, N), has_w=True))],
    "trace_viewport_hits_device": [
        ("cams44", dict(cams=t(F, LN, 4, 4))), ("uint32", dict(label=t(U, LH, LW), cell=t(U, LH, LW))), ("cell_words", dict(cell=t(I, LH, LW))),
        ("cell_pairs", dict(cell=t(S, LH, LW, 2))), ("dist", dict(dist=t(F, LH, LW))), ("has_w", dict(has_w=True)), ("hide", dict(hide=t(I, LN))),
        ("all", dict(cams=t(F, LN, 4, 4), cell=t(S, LH, LW, 2), dist=t(F, LH, LW), hide=t(I, LN), has_w=True))],
    "players_step_device": [
        ("n0", dict(keys=t(B, 0), cams=t(F, 0, 16), gravity=t(F, 0, 4))), ("n0_traversals", dict(keys=t(B, 0), cams=t(F, 0, 16), gravity=t(F, 0, 4),
                                                                                                  traversals=t(I, 0))),
        ("cams44", dict(cams=t(F, P, 4, 4))), ("traversals", dict(traversals=t(I, P))), ("numbers", dict(tdiff=0.5, ticks=3)),
        ("numpy_numbers", dict(tdiff=np.float32(0.25), ticks=np.int64(1024)))],
    "pixel_rays_device": [
        ("cams44", dict(cams=t(F, N, 4, 4))), ("xy_shared", dict(xy=t(I, 3, 2))), ("xy_own", dict(xy=t(I, N, 3, 2))),
        ("xy_empty", dict(xy=t(I, 0, 2))), ("n0", dict(cams=t(F, 0, 16))), ("rays", dict(rays=t(F, N * _M, 8))), ("rays3", dict(rays=t(F, N, _M, 8))),
        ("seeds", dict(seeds=t(I, N * _M))), ("seeds2", dict(seeds=t(U, N, _M))), ("no_seeds", dict(seeds=False)), ("work", dict(work=t(F, N, WORK))),
        ("size", dict(width=4, height=2)), ("size_numpy", dict(width=np.int32(5), height=np.int64(3))), ("shared_true", dict(shared=True)),
        ("shared_true_xy", dict(xy=t(I, 3, 2), shared=True)), ("shared_false_xy", dict(xy=t(I, N, 3, 2), shared=np.bool_(False))),
        ("all", dict(cams=t(F, N, 4, 4), xy=t(I, N, 3, 2), width=4, height=2, shared=False, rays=t(F, N, 3, 8), seeds=t(I, N, 3), work=t(F, N, WORK)))],
    "upload_spheres_device": [("n0", dict(spheres=t(F, 0, 8), max_pairs=0)), ("numpy_pairs", dict(max_pairs=np.int64(2 ** 31 - 1)))],
}

# (method, tag, kwargs that differ from the plain call, the parameter the message names): the faults that no rule below makes
OTHER_REFUSED = [(m, k + "_layout", dict(layout=v), "layout") for m in ("trace_viewports_device", "trace_viewport_hits_device")
                 for k, v in (("dead", DEAD), ("foreign", FOREIGN), ("no", 7), ("none", None))] + [
    ("trace_views_device", "n0", dict(cams=t(F, 0, 16), secs=t(F, 0), sbuf=t(I, 0, H, W), zbuf=t(F, 0, H, W)), "cams"),
    ("trace_view_hits_device", "n0", dict(cams=t(F, 0, 16), label=t(I, 0, H, W)), "cams"),
    ("trace_view_hits_device", "cell_pairs_flat", dict(cell=t(S, N, H, W)), "cell"),
    ("trace_view_hits_device", "cell_words_paired", dict(cell=t(I, N, H, W, 2)), "cell"),
    ("trace_viewport_hits_device", "cell_pairs_flat", dict(cell=t(S, LH, LW)), "cell"),
    ("trace_viewport_hits_device", "cell_words_paired", dict(cell=t(I, LH, LW, 2)), "cell"),
    ("trace_rays_device", "mixed", dict(col=0x3000), None), ("trace_rays_device", "mixed_seeds", dict(seeds=0x6000), None),
    ("trace_rays_device", "mixed_numpy", dict(rays=t(F, R, 8, how="numpy"), col=0x3000, depth=0x4000, n=R), None),
    ("trace_rays_device", "pointers_without_n", dict(rays=0x2000, col=0x3000, depth=0x4000), None),
    ("trace_rays_device", "pointers_n_negative", dict(rays=0x2000, col=0x3000, depth=0x4000, n=-1), None),
    ("trace_rays_device", "pointers_n_too_large", dict(rays=0x2000, col=0x3000, depth=0x4000, n=RAYS_MAX + 1), None),
    ("trace_rays_device", "n_disagrees", dict(n=R + 1), None),
    ("trace_rays_device", "pointers_hide_numpy", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R, hide=t(I, R, how="numpy")), "hide"),
    ("trace_rays_device", "pointers_hide_rows", dict(rays=0x2000, col=0x3000, depth=0x4000, n=R, hide=t(I, R + 1)), "hide"),
    ("trace_hits_device", "mixed", dict(hits=0x3000), None), ("trace_hits_device", "mixed_none", dict(rays=None, hits=0x3000, n=R), None),
    ("trace_hits_device", "mixed_numpy", dict(rays=t(F, R, 8, how="numpy"), hits=0x3000, n=R), None),
    ("trace_hits_device", "pointers_without_n", dict(rays=0x2000, hits=0x3000), None),
    ("trace_hits_device", "pointers_n_negative", dict(rays=0x2000, hits=0x3000, n=-1), None),
    ("trace_hits_device", "pointers_n_too_large", dict(rays=0x2000, hits=0x3000, n=RAYS_MAX + 1), None),
    ("trace_hits_device", "n_disagrees", dict(n=R - 1), None),
    ("trace_hits_device", "hits_int32_48", dict(hits=t(I, R, 48)), "hits"), ("trace_hits_device", "hits_uint8_12", dict(hits=t(B, R, 12)), "hits"),
    ("trace_hits_device", "pointers_hide_cpu", dict(rays=0x2000, hits=0x3000, n=R, hide=t(I, R, how="cpu")), "hide"),
    ("trace_reach_device", "hits_int32_48", dict(hits=t(I, R, 48)), "hits"), ("trace_reach_device", "hits_uint8_12", dict(hits=t(B, R, 12)), "hits"),
    ("players_step_device", "ticks_0", dict(ticks=0), "ticks"), ("players_step_device", "ticks_too_many", dict(ticks=1025), "ticks"),
    ("players_step_device", "ticks_fraction", dict(ticks=1.5), "ticks"), ("players_step_device", "tdiff_inf", dict(tdiff=float("inf")), "tdiff"),
    ("players_step_device", "tdiff_nan", dict(tdiff=float("nan")), "tdiff"), ("players_step_device", "tdiff_overflows", dict(tdiff=1e39), "tdiff"),
    ("pixel_rays_device", "width_0", dict(width=0), "width"), ("pixel_rays_device", "width_too_large", dict(width=32769), "width"),
    ("pixel_rays_device", "width_bool", dict(width=True), "width"), ("pixel_rays_device", "width_float", dict(width=8.0), "width"),
    ("pixel_rays_device", "height_0", dict(height=0), "height"), ("pixel_rays_device", "height_too_large", dict(height=32769), "height"),
    ("pixel_rays_device", "height_float", dict(height=4.0), "height"), ("pixel_rays_device", "shared_int", dict(shared=1), "shared"),
    ("pixel_rays_device", "shared_false_whole_frame", dict(shared=False), None),
    ("pixel_rays_device", "shared_false_xy_shared", dict(xy=t(I, 3, 2), shared=False), "shared"),
    ("pixel_rays_device", "shared_true_xy_own", dict(xy=t(I, N, 3, 2), shared=True), "shared"),
    ("pixel_rays_device", "xy_1d", dict(xy=t(I, 6)), "xy"), ("pixel_rays_device", "xy_4d", dict(xy=t(I, 1, N, 3, 2)), "xy"),
    ("pixel_rays_device", "xy_own_rows", dict(xy=t(I, N + 1, 3, 2)), "xy"), ("pixel_rays_device", "xy_list", dict(xy=[[0, 0]]), "xy"),
    ("pixel_rays_device", "too_many_rays", dict(width=32768, height=32768), None),
    ("pixel_rays_device", "cams_rows", dict(cams=t(F, N + 1, 16), work=t(F, N, WORK)), None),
    ("pixel_rays_device", "rays3_rows", dict(rays=t(F, N + 1, _M, 8)), "rays"), ("pixel_rays_device", "rays3_pixels", dict(rays=t(F, N, _M + 1, 8)), "rays"),
    ("pixel_rays_device", "rays_1d", dict(rays=t(F, N * _M * 8)), "rays"), ("pixel_rays_device", "seeds2_pixels", dict(seeds=t(I, N, _M + 1)), "seeds"),
    ("pixel_rays_device", "seeds_3d", dict(seeds=t(I, N, _M, 1)), "seeds"), ("pixel_rays_device", "seeds_true", dict(seeds=True), "seeds"),
    ("upload_spheres_device", "too_many", dict(spheres=t(F, OBJ_MAX + 1, 8)), None),
    ("upload_spheres_device", "max_pairs_negative", dict(max_pairs=-1), "max_pairs"),
    ("upload_spheres_device", "max_pairs_too_large", dict(max_pairs=2 ** 31), "max_pairs"),
    ("upload_spheres_device", "max_pairs_bool", dict(max_pairs=True), "max_pairs"),
    ("upload_spheres_device", "max_pairs_float", dict(max_pairs=100.0), "max_pairs"),
]


def _accepted():
    out = []
    for method, (base, params) in BASE.items():
        streams = [("plain", {}), ("stream_raw", dict(stream=RAW)), ("stream_given", dict(stream=GIVEN))]
        for tag, kw in streams + VARIANTS[method]:
            out.append(("%s-%s" % (method, tag), method, dict(base, **kw)))
        # a parameter held to 4 bytes only may start 4 bytes past an aligned address
        for name, (align, _) in params.items():
            d = dict(base, **OPTIONAL[method]).get(name)
            if align == 4:
                out.append(("%s-%s_off4" % (method, name), method, dict(base, **{name: d.but(how="off4")})))
    return out


def _refused():
    out = []
    for method, (base, params) in BASE.items():
        for name, (align, rows) in params.items():
            d = dict(base, **OPTIONAL[method])[name]
            wider = d.shape[:-1] + (d.shape[-1] + 1,) if len(d.shape) > 1 else d.shape + (1,)
            faults = [("dtype", d.but(dtype=WRONG[d.dtype]), name), ("trailing", d.but(shape=wider), name), ("strided", d.but(how="strided"), name),
                      ("cpu", d.but(how="cpu"), name), ("numpy", d.but(how="numpy"), name), ("other_gpu", d.but(how="gpu1"), None)]
            if rows is not None and not (method == "pixel_rays_device" and name == "cams"):
                faults.append(("rows", d.but(shape=(d.shape[0] + 1,) + d.shape[1:]), name if rows == "named" else None))
            if align >= 8:
                faults.append(("off4", d.but(how="off4"), name))
            if name in base and method != "trace_hits_device":        # (there None is a pointer that is none: the mixing rule)
                faults.append(("none", None, name))
            for tag, v, named in faults:
                out.append(("%s-%s_%s" % (method, name, tag), method, dict(base, **{name: v}), named))
    for method, tag, kw, named in OTHER_REFUSED:
        out.append(("%s-%s" % (method, tag), method, dict(BASE[method][0], **kw), named))
    return out


ACCEPTED = _accepted()
REFUSED = _refused()
assert len({c[0] for c in ACCEPTED + REFUSED}) == len(ACCEPTED) + len(REFUSED)
