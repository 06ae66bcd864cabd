"""Host-side mirror of the reference's render interface, over libpwnhip.so.

Names follow the reference: ``level_load`` (level.h:107), ``level_prepare_render``
(level.h:64; here ``set_objects``), ``trace_screen_centred`` (screen.h:31),
``screen_upscale`` (screen.h:126).  Errors the reference reports by returning
NULL / asserting are raised as ``PwnError`` with the library's code.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib

# pwn_hit (pwnhip.h): a first-hit record of trace_hits, 48 bytes
HIT_DTYPE = np.dtype([("kind", "<i4"), ("face", "<i4"), ("object", "<i4"), ("portals", "<i4"),
                      ("dist", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                      ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("cell_x", "<i2"), ("cell_z", "<i2")])
SPHERE_DTYPE = np.dtype([("r", "<f4"), ("refl", "<f4"), ("x", "<f4"), ("y", "<f4"),
                         ("z", "<f4"), ("cb", "<f4"), ("cg", "<f4"), ("cr", "<f4")])
PORTAL_DTYPE = np.dtype([(n, "<i4") for n in ("x1", "z1", "x2", "z2", "rot12", "c1", "c2")])


class PwnError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = "%s: %s (%d)" % (where, lib.pwn_strerror(code).decode(), code)
        if detail:
            msg += ": " + detail
        super().__init__(msg)


class Renderer:
    """One GPU context for a fixed frame size (rwidth x rheight, main.c:26-27)."""

    def __init__(self, width, height, device=0, devices=None):
        """devices: a list of HIP ordinals -> pwn_init_multi, ONE handle whose frames are row-tiled over them inside this
        process (the same ordinal several times: so many members on that device)"""
        self.w, self.h, self.device = int(width), int(height), int(device)
        self._ctx = C.c_void_p()
        self.devices = None
        if devices is not None:
            self.devices = [int(d) for d in devices]
            self.device = self.devices[0]
            arr = (C.c_int * len(self.devices))(*self.devices)
            rc = lib.pwn_init_multi(C.byref(self._ctx), arr, len(self.devices), self.w, self.h)
            if rc != 0:
                self._ctx = C.c_void_p()
                raise PwnError(rc, "pwn_init_multi(devices=%s, %dx%d)" % (self.devices, width, height))
            return
        rc = lib.pwn_init(C.byref(self._ctx), self.device, self.w, self.h)
        if rc != 0:
            self._ctx = C.c_void_p()
            raise PwnError(rc, "pwn_init(device=%d, %dx%d)" % (device, width, height))

    def group_info(self):
        gi = _lib.GroupInfo()
        self._chk(lib.pwn_group_info_get(self._ctx, C.byref(gi)), "pwn_group_info_get")
        n = gi.members
        return {"members": n, "transport": {0: "rccl", 1: "shm", 2: "local"}.get(gi.transport, gi.transport), "devices": [gi.devices[i] for i in range(n)],
                "cuts": [gi.cuts[i] for i in range(n + 1)], "halo_rows": gi.halo_rows, "host_sink": bool(gi.host_sink),
                "frames": int(gi.frames), "frames_redone": int(gi.frames_redone), "recuts": int(gi.recuts),
                "note": gi.note.decode("latin-1")}

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            lib.pwn_destroy(self._ctx)
            self._ctx = C.c_void_p()
            for lay in getattr(self, "_layouts", None) or []:       # (pwn_destroy freed them)
                lay._ptr = None
            self._layouts = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc < 0:
            raise PwnError(rc, where, lib.pwn_last_error(self._ctx).decode(errors="replace"))
        return rc

    # -- options -----------------------------------------------------------
    def set_blur_passes(self, n):
        """POSTPROC_BLUR (defs.h:9); 0 disables the post-process."""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_BLUR_PASSES, int(n)), "pwn_set_option")

    def set_scheduler(self, which):
        """PWN_OPT_SCHEDULER: "units" (a wave64 traces 16x4-pixel units in step) or "refill"
        (lanes whose ray ended are refilled by ballot + prefix rank)."""
        v = {"units": _lib.PWN_SCHED_UNITS, "refill": _lib.PWN_SCHED_REFILL}.get(which, which)
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_SCHEDULER, int(v)), "pwn_set_option")

    def set_frame_timing(self, every):
        """HIP events around the kernels of every N-th frame in flight (0: never, 1: all)."""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_FRAME_TIMING, int(every)), "pwn_set_option")

    def set_frame_overlap(self, on):
        """frames in flight: successive frames alternate between two compute streams (default) or all run on one"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_FRAME_OVERLAP, 1 if on else 0), "pwn_set_option")

    def set_tiled_choreo(self, split):
        """PWN_OPT_TILED_CHOREO, before tiled_init: False (default) = everything of a frame in order on the frame's own compute stream;
        True = the exchanges on a third stream, blur and gather one and two submits late (rounds 2-3).  Same frames."""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_TILED_CHOREO, 1 if split else 0), "pwn_set_option")

    def set_tiled_comms(self, per_stream):
        """PWN_OPT_TILED_COMMS, before tiled_init: False (default) = one RCCL communicator; True = one per compute stream"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_TILED_COMMS, 2 if per_stream else 1), "pwn_set_option")

    def set_tiled_streams(self, n):
        """PWN_OPT_TILED_STREAMS, before tiled_init: compute streams the frames of an in-stream tiling rotate over, 2 or 3"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_TILED_STREAMS, int(n)), "pwn_set_option")

    def set_unit_order(self, on):
        """PWN_OPT_UNIT_ORDER: the trace kernel's units handed out by what they cost in the last launch (True) or
        in arithmetic order (False, the default).  Never changes a frame."""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_UNIT_ORDER, 1 if on else 0), "pwn_set_option")

    def launch_order_waits(self):
        """trace launches so far that left the rotation over the compute streams and were ordered behind the launch R before them"""
        out = C.c_uint64(0)
        self._chk(lib.pwn_launch_order_waits(self._ctx, C.byref(out)), "pwn_launch_order_waits")
        return int(out.value)

    def unit_order_state(self):
        out = (C.c_uint64 * 4)()
        self._chk(lib.pwn_unit_order_state(self._ctx, out), "pwn_unit_order_state")
        return {"option": int(out[0]), "launches_in_sorted_order": int(out[1]), "sorts": int(out[2]), "units_ordered": int(out[3])}

    def unit_order_probe(self, cost):
        """pwn_unit_order_probe: the per-queue sort of `cost` (uint16 per unit) -> [64, cap] uint32, unused entries 0xffffffff"""
        cost = np.ascontiguousarray(cost, np.uint16)
        cap = (cost.size + 63) // 64
        out = np.zeros((64, cap), np.uint32)
        self._chk(lib.pwn_unit_order_probe(self._ctx, cost.ctypes.data, cost.size, out.ctypes.data), "pwn_unit_order_probe")
        return out

    def set_trace_room(self, workgroups):
        """PWN_OPT_TRACE_ROOM: workgroups the persistent trace grid leaves free for the other stream's kernels while frames
        alternate between two streams; -1 (default) = the library measures which of 0 / one per CU is faster and keeps it"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_TRACE_ROOM, int(workgroups)), "pwn_set_option")

    def trace_room_state(self):
        out = (C.c_int * 4)()
        self._chk(lib.pwn_trace_room_state(self._ctx, out), "pwn_trace_room_state")
        return {"option": out[0], "room_now": out[1], "comparisons": out[2], "changes": out[3]}

    def set_wave_log(self, on):
        """stats()["wave_time"] / (["waves"] * ["kernel_span"]) = mean wave residency of the last frame"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_WAVE_LOG, 1 if on else 0), "pwn_set_option")

    def set_refill_limit(self, n):
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_REFILL_LIMIT, int(n)), "pwn_set_option")

    def set_counters(self, on):
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_COUNTERS, 1 if on else 0), "pwn_set_option")

    # -- level (level.h:107-228) ---------------------------------------------
    def level_load(self, path):
        self._chk(lib.pwn_level_load(self._ctx, str(path).encode()), "pwn_level_load(%s)" % path)

    def level_load_text(self, text):
        if isinstance(text, str):
            text = text.encode("latin-1")
        self._chk(lib.pwn_level_load_mem(self._ctx, text, len(text)), "pwn_level_load_mem")

    def upload_level(self, data, pmap):
        data = np.ascontiguousarray(data, np.uint8)
        pmap = np.ascontiguousarray(pmap, np.int32)
        if data.shape != (64, 64) or pmap.shape != (26, 7):
            raise ValueError("data must be (64,64) uint8 and pmap (26,7) int32")
        self._chk(lib.pwn_upload_level(self._ctx, data.ctypes.data, pmap.ctypes.data), "pwn_upload_level")

    def get_level(self):
        data = np.zeros((64, 64), np.uint8)
        pmap = np.zeros((26, 7), np.int32)
        spawn = np.zeros(2, np.int32)
        self._chk(lib.pwn_get_level(self._ctx, data.ctypes.data, pmap.ctypes.data, spawn.ctypes.data), "pwn_get_level")
        return data, pmap, spawn

    # -- objects (script.h:10-40 + level.h:64-81) ----------------------------
    def set_objects(self, spheres):
        """The live sphere set for the next frames; binning per cell
        (level_prepare_render) happens inside."""
        spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
        self._chk(lib.pwn_upload_spheres(self._ctx, spheres.ctypes.data if len(spheres) else None,
                                         len(spheres)), "pwn_upload_spheres")

    def obj_new(self):
        """obj_new() (script.h:1-8): index of a fresh object slot."""
        return self._chk(lib.pwn_obj_new(self._ctx), "pwn_obj_new")

    def obj_set(self, obj, typ, r, refl, x, y, z, cb, cg, cr):
        """obj_set(o, "sphere", r, refl, x, y, z, b, g, r) (script.h:10-40)."""
        if str(typ).lower() != "sphere":
            raise ValueError('obj_set: invalid typ "%s"' % typ)
        self._chk(lib.pwn_obj_set_sphere(self._ctx, int(obj), r, refl, x, y, z, cb, cg, cr), "pwn_obj_set_sphere")
        return obj

    def obj_free(self, obj):
        self._chk(lib.pwn_obj_free(self._ctx, int(obj)), "pwn_obj_free")

    def level_get(self, cx, cz):
        """level_get(cx, cz) (script.h:53-64): the cell as a 1-character string."""
        return chr(self._chk(lib.pwn_level_get(self._ctx, int(cx), int(cz)), "pwn_level_get"))

    def level_prepare_render(self):
        """level_prepare_render (level.h:64-81) over the object table."""
        self._chk(lib.pwn_prepare_render(self._ctx), "pwn_prepare_render")

    def get_objects(self):
        n = self._chk(lib.pwn_get_objects(self._ctx, None, 0), "pwn_get_objects")
        out = np.zeros(n, SPHERE_DTYPE)
        if n:
            self._chk(lib.pwn_get_objects(self._ctx, out.ctypes.data, n), "pwn_get_objects")
        return out

    def get_bins(self):
        counts = np.zeros(4096, np.uint16)
        n = self._chk(lib.pwn_get_bins(self._ctx, counts.ctypes.data, None, 0), "pwn_get_bins")
        idx = np.zeros(max(n, 1), np.int32)
        self._chk(lib.pwn_get_bins(self._ctx, counts.ctypes.data, idx.ctypes.data, n), "pwn_get_bins")
        return counts, idx[:n]

    def sphere_tables(self):
        """pwn_sphere_tables_state: form, size and shape of the sphere tables in force (see sphere_tables_plan)"""
        out = (C.c_uint64 * 6)()
        self._chk(lib.pwn_sphere_tables_state(self._ctx, out), "pwn_sphere_tables_state")
        return _tables_dict(out)

    # -- sphere tables built on the GPU (pwn_upload_spheres_device) ------------
    def upload_spheres_device(self, spheres, max_pairs, stream=None):
        """pwn_upload_spheres_device: upload_spheres for spheres that are on the GPU already, at most five launches on `stream` (a
        torch stream or a raw hipStream_t; None = torch's current stream), no synchronisation.  spheres: a contiguous float32 GPU
        tensor (n,8) on this context's GPU, 16-byte aligned, rows r, refl, x, y, z, cb, cg, cr (SPHERE_DTYPE's order); max_pairs: the
        most (cell, sphere) pairs the tables may hold -- spheres that make more put tables without any sphere into force
        (spheres_device_state says so).  The tensor may be overwritten, in stream order, once the call has returned."""
        who = "upload_spheres_device"
        n, dev = _check(who, [("spheres", spheres, _F32, (None, 8), 16)], device=self.device)
        _count(who, "spheres", n, 0, _lib.PWN_OBJ_MAX)
        if isinstance(max_pairs, bool) or not isinstance(max_pairs, (int, np.integer)) or not 0 <= int(max_pairs) < 2 ** 31:
            raise ValueError("%s: max_pairs must be an integer 0 .. 2^31 - 1, not %r" % (who, max_pairs))
        _device_call(self, lib.pwn_upload_spheres_device, stream, dev, (n, _ptr(spheres), int(max_pairs)))

    def spheres_device_state(self):
        """pwn_spheres_device_state (blocks: waits for the last build): dict(in_force, n, max_pairs, pairs, cells, longest, reason,
        uploads); reason 0 = built, 1 = more pairs than max_pairs, 2 = a list longer than PWN_LIST_MAX"""
        out = (C.c_uint64 * 8)()
        self._chk(lib.pwn_spheres_device_state(self._ctx, out), "pwn_spheres_device_state")
        return dict(zip(("in_force", "n", "max_pairs", "pairs", "cells", "longest", "reason", "uploads"), (int(v) for v in out)))

    # -- the level's tables baked on the GPU (pwn_upload_level_device) ---------
    def upload_level_device(self, data, pmap=None, stream=None):
        """pwn_upload_level_device: upload_level for a grid that is on the GPU already, five launches on `stream` (a torch stream or a
        raw hipStream_t; None = torch's current stream), no synchronisation.  data: a contiguous uint8 GPU tensor (64, 64), data[z][x];
        pmap: a contiguous int32 GPU tensor (26, 7), rows x1 z1 x2 z2 rot12 c1 c2, or None -- the table is then derived from the cells
        as the level loader derives it.  Both on this context's GPU and 16-byte aligned; they may be overwritten, in stream order, once
        the call has returned.  A table that upload_level would refuse leaves the level in force in force (level_device_state says
        why).  Either way the tables in force hold no sphere: follow the call with upload_spheres_device."""
        who = "upload_level_device"
        _, dev = _check(who, [("data", data, _U8, (64, 64), 16)], [("pmap", pmap, _I32, (26, 7), 16)], device=self.device)
        _device_call(self, lib.pwn_upload_level_device, stream, dev, (_ptr(data), _ptr(pmap)))

    def level_device_state(self):
        """pwn_level_device_state (blocks: waits for the last device level build): dict(in_force, uploads, verdict, letter, records,
        paired, derived); verdict 0 = taken, 1 = a coordinate outside -1 .. 63, 2 = the rule for cells outside the grid; letter =
        the lowest offending letter 0 .. 25, else 26"""
        out = (C.c_uint64 * 8)()
        self._chk(lib.pwn_level_device_state(self._ctx, out), "pwn_level_device_state")
        return dict(zip(("in_force", "uploads", "verdict", "letter", "records", "paired", "derived"), (int(v) for v in out)))

    def get_level_device(self):
        """pwn_get_level_device (blocks): (data (64,64) uint8, pmap (26,7) int32) of the device-built level in force, as numpy arrays"""
        data = np.zeros((64, 64), np.uint8)
        pmap = np.zeros((26, 7), np.int32)
        self._chk(lib.pwn_get_level_device(self._ctx, data.ctypes.data, pmap.ctypes.data), "pwn_get_level_device")
        return data, pmap

    # -- frame (screen.h:31-124) ---------------------------------------------
    def trace_screen_centred(self, cam, sec_current=0.0, want_z=True, sbuf=None, zbuf=None):
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        if sbuf is None:
            sbuf = np.empty((self.h, self.w), np.uint32)
        if want_z and zbuf is None:
            zbuf = np.empty((self.h, self.w), np.float32)
        self._chk(lib.pwn_trace_screen_centred(self._ctx, cam.ctypes.data, float(sec_current),
                                               sbuf.ctypes.data, zbuf.ctypes.data if want_z else None),
                  "pwn_trace_screen_centred")
        return (sbuf, zbuf) if want_z else sbuf

    def trace_views(self, cams, secs, want_z=True):
        """pwn_trace_views: n views of this context's size in one call.  cams (n,4,4) or (n,16), secs (n,).  Returns (n,h,w)
        uint32 colour and, with want_z, (n,h,w) float32 depth; view i as trace_screen_centred(cams[i], secs[i]) renders it."""
        cams = _cam_records(cams, "trace_views")
        n = _count("trace_views", "views (cams' rows)", cams.shape[0], 1, _lib.PWN_VIEWS_MAX)
        secs = np.asarray(secs)
        if secs.shape != (n,):
            raise ValueError("trace_views: secs must have shape (%d,), not %s" % (n, secs.shape))
        secs = np.ascontiguousarray(secs, np.float32)
        sbuf = np.empty((n, self.h, self.w), np.uint32)
        zbuf = np.empty((n, self.h, self.w), np.float32) if want_z else None
        self._chk(lib.pwn_trace_views(self._ctx, n, cams.ctypes.data, secs.ctypes.data, sbuf.ctypes.data,
                                      zbuf.ctypes.data if want_z else None), "pwn_trace_views")
        return (sbuf, zbuf) if want_z else sbuf

    def trace_views_device(self, cams, secs, sbuf, zbuf, work=None, has_w=False, stream=None, hide=None):
        """pwn_trace_views_device: the batch of trace_views from cameras on the GPU into planes on the GPU, stream-ordered, no
        synchronisation and no host copy.  All torch tensors on this context's GPU, contiguous: cams (n,16) or (n,4,4) float32,
        secs (n,) float32, sbuf (n,h,w) int32 or uint32 (the finished views), zbuf (n,h,w) float32 (in / out: a primary ray that
        runs out of steps keeps what it holds), work (n,h,w) int32 or uint32 scratch, needed with blur on.  has_w: honour the
        cameras' w lanes (PWN_VIEWS_HAS_W; else they are taken as 0, 0, 0, 1).  stream: a torch.cuda.Stream or a raw hipStream_t;
        None = torch's current stream on the tensors' device.
        hide: None, or an (n,) int32 tensor (pwn_trace_views_hide_device): view i does not see sphere hide[i] of the table in force,
        on any segment of its rays; PWN_HIDE_NONE (-1) and every other value that is no sphere's index hide nothing."""
        who = "trace_views_device"
        cams, plane = _cams16(cams), (None, self.h, self.w)
        n, dev = _check(who, [("cams", cams, _F32, (None, 16), 4), ("secs", secs, _F32, (None,), 4),
                              ("sbuf", sbuf, _WORDS, plane, 4), ("zbuf", zbuf, _F32, plane, 4)],
                        [("work", work, _WORDS, plane, 4), ("hide", hide, _I32, (None,), 4)])
        _count(who, "views (cams' rows)", n, 1, _lib.PWN_VIEWS_MAX)
        _device_call(self, lib.pwn_trace_views_hide_device if hide is not None else lib.pwn_trace_views_device, stream, dev,
                     (n, _ptr(cams), _ptr(secs), _lib.PWN_VIEWS_HAS_W if has_w else 0, _ptr(work), _ptr(sbuf), _ptr(zbuf)), hide, 3)

    def trace_viewports(self, rects, cams, secs, want_z=True, sbuf=None, zbuf=None):
        """pwn_trace_viewports: n views of their own sizes composited into ONE frame of this context's size in one call.  rects
        (n,4) int (x, y, w, h), cams (n,4,4) or (n,16), secs (n,).  Returns (h,w) uint32 colour and, with want_z, (h,w) float32
        depth (else None): rectangle i as trace_screen_centred(cams[i], secs[i]) renders it on a context of w_i x h_i.
        sbuf / zbuf: the caller's own frame buffers (host_register makes their copies plain DMA)."""
        rects = _rect_records(rects, "trace_viewports")
        n = rects.shape[0]
        cams = _cam_records(cams, "trace_viewports", n)
        secs = np.asarray(secs)
        if secs.shape != (n,):
            raise ValueError("trace_viewports: secs must have shape (%d,), not %s" % (n, secs.shape))
        secs = np.ascontiguousarray(secs, np.float32)
        if sbuf is None:
            sbuf = np.empty((self.h, self.w), np.uint32)
        if not want_z:
            zbuf = None
        elif zbuf is None:
            zbuf = np.empty((self.h, self.w), np.float32)
        self._chk(lib.pwn_trace_viewports(self._ctx, n, rects.ctypes.data, cams.ctypes.data, secs.ctypes.data, sbuf.ctypes.data,
                                          zbuf.ctypes.data if want_z else None), "pwn_trace_viewports")
        return sbuf, zbuf

    def viewports_layout(self, W, H, rects):
        """pwn_viewports_layout: the part of trace_viewports_device that is known beforehand -- a frame of W x H (any size, not
        this context's) and rects (n,4) int (x, y, w, h) inside it, no two overlapping.  Made once (blocks, allocates), used by any
        number of calls.  Returns a ViewportsLayout with .info() and .free(); closing the renderer frees what is left."""
        rects = _rect_records(rects, "viewports_layout")
        ptr = C.c_void_p()
        self._chk(lib.pwn_viewports_layout(self._ctx, int(W), int(H), rects.shape[0], rects.ctypes.data, C.byref(ptr)), "pwn_viewports_layout")
        lay = ViewportsLayout(self, ptr, int(W), int(H), rects.shape[0])
        if getattr(self, "_layouts", None) is None:
            self._layouts = []
        self._layouts.append(lay)
        return lay

    def trace_viewports_device(self, layout, cams, secs, sbuf, zbuf, work=None, has_w=False, stream=None, hide=None):
        """pwn_trace_viewports_device: the views of a viewports_layout from cameras on the GPU into ONE frame of the layout's W x H on
        the GPU, stream-ordered, no synchronisation and no host copy.  All torch tensors on this context's GPU, contiguous and
        16-byte aligned: cams (n,16) or (n,4,4) float32, camera i for rectangle i; secs (n,) float32; sbuf (H,W) int32 or uint32
        (rectangle i as trace_screen_centred renders it on a context of w_i x h_i; nothing outside the rectangles is written);
        zbuf (H,W) float32 (in / out: a primary ray that runs out of steps keeps what it holds); work (H,W) int32 or uint32 scratch,
        needed with blur on.  has_w and stream as trace_views_device takes them.
        hide: None, or an (n,) int32 tensor on the same GPU (pwn_trace_viewports_hide_device): rectangle i does not see sphere hide[i]
        of the table in force; PWN_HIDE_NONE (-1) and every other value that is no sphere's index hide nothing."""
        who = "trace_viewports_device"
        _live_layout(who, self, layout)
        cams, plane = _cams16(cams), (layout.H, layout.W)
        _, dev = _check(who, [("cams", cams, _F32, (None, 16), 16), ("secs", secs, _F32, (None,), 16),
                              ("sbuf", sbuf, _WORDS, plane, 16), ("zbuf", zbuf, _F32, plane, 16)],
                        [("work", work, _WORDS, plane, 16), ("hide", hide, _I32, (None,), 4)], n=layout.n)
        _device_call(self, lib.pwn_trace_viewports_hide_device if hide is not None else lib.pwn_trace_viewports_device, stream, dev,
                     (layout._ptr, _ptr(cams), _ptr(secs), _lib.PWN_VIEWS_HAS_W if has_w else 0, _ptr(work), _ptr(sbuf), _ptr(zbuf)), hide, 3)

    # -- caller-supplied rays (pwn_trace_rays) --------------------------------
    def pixel_rays(self, cam, xy=None, order="rows"):
        """pixel_rays() at this context's size"""
        return pixel_rays(self.w, self.h, cam, xy, order)

    def trace_rays(self, rays, seeds=None, sec_current=0.0, depth=None):
        """pwn_trace_rays: trace_ray (trace.h:186) for n rays of the caller's on this context's level and objects.  rays: (n,8)
        records (origin x y z w, direction x y z w) or a pair (origins, directions) of (n,3) or (n,4) arrays, missing w lanes
        1 and 0; seeds (n,) uint32 or None (0); depth (n,) the depth each ray keeps if it runs out of steps, or None (0).
        Returns (colour (n,) uint32 BGRA8, depth (n,) float32): the pre-blur pixel and primary depth of each ray."""
        rays = _ray_records(rays, "trace_rays")
        n = rays.shape[0]
        if seeds is not None:
            seeds = np.asarray(seeds)
            if seeds.shape != (n,):
                raise ValueError("trace_rays: seeds must have shape (%d,), not %s" % (n, seeds.shape))
            seeds = np.ascontiguousarray(seeds.astype(np.uint32, copy=False))
        if depth is None:
            z = np.zeros(n, np.float32)
        else:
            z = np.array(depth, np.float32)
            if z.shape != (n,):
                raise ValueError("trace_rays: depth must have shape (%d,), not %s" % (n, z.shape))
        col = np.empty(n, np.uint32)
        self._chk(lib.pwn_trace_rays(self._ctx, n, rays.ctypes.data, seeds.ctypes.data if seeds is not None else None,
                                     float(sec_current), col.ctypes.data, z.ctypes.data), "pwn_trace_rays")
        return col, z

    def trace_rays_device(self, rays, col, depth, seeds=None, sec_current=0.0, has_w=False, stream=None, n=None, hide=None):
        """pwn_trace_rays_device: one trace launch, stream-ordered, no synchronisation.  rays / col / depth / seeds are torch
        tensors on this context's GPU -- rays (n,8) float32 16-byte aligned, col (n,) int32 or uint32, depth (n,) float32 (in / out),
        seeds (n,) int32 or uint32 or None -- or raw device pointers, with n given.  has_w: honour the records' w lanes
        (PWN_RAYS_HAS_W; else they are taken as 1 and 0).  stream: a torch.cuda.Stream or a raw hipStream_t; None = torch's
        current stream on this device for tensors, the default stream for pointers.
        hide: None, or an (n,) int32 tensor on the same GPU (pwn_trace_rays_hide_device): ray i does not see sphere hide[i] of the
        table in force, on any of its segments; PWN_HIDE_NONE (-1) and every other value that is no sphere's index hide nothing."""
        who, hidden = "trace_rays_device", ("hide", hide, _I32, (None,), 4)
        if _tensors_given(who, [a for a in (rays, col, depth, seeds) if a is not None]):
            n, dev = _check(who, [("rays", rays, _F32, (None, 8), 16), ("col", col, _WORDS, (None,), 4), ("depth", depth, _F32, (None,), 4)],
                            [("seeds", seeds, _WORDS, (None,), 4), hidden], None if n is None else int(n))
            rays, col, depth, seeds = _ptr(rays), _ptr(col), _ptr(depth), _ptr(seeds)
        else:
            n, dev = _check(who, (), [hidden], _rays_n(who, n))
        _rays_n(who, n)
        _device_call(self, lib.pwn_trace_rays_hide_device if hide is not None else lib.pwn_trace_rays_device, stream, dev,
                     (n, rays, seeds, float(sec_current), _lib.PWN_RAYS_HAS_W if has_w else 0, col, depth), hide, 3)

    # -- first hits of caller-supplied rays (pwn_trace_hits) -------------------
    def trace_hits(self, rays):
        """pwn_trace_hits: what the primary segment of each ray ends on.  rays as trace_rays takes them: (n,8) records or a pair
        (origins, directions).  Returns (n,) HIT_DTYPE records: kind (PWN_HIT_NONE / WALL / SPHERE), face, object (index into
        get_objects() / object_ids()), portals crossed, dist, the point x y z, the walked direction dx dy dz, the cell."""
        rays = _ray_records(rays, "trace_hits")
        n = rays.shape[0]
        hits = np.zeros(n, HIT_DTYPE)
        self._chk(lib.pwn_trace_hits(self._ctx, n, rays.ctypes.data if n else None, hits.ctypes.data if n else None), "pwn_trace_hits")
        return hits

    def trace_hits_device(self, rays, hits, has_w=False, stream=None, n=None, hide=None):
        """pwn_trace_hits_device: one trace launch, stream-ordered, no synchronisation.  rays (n,8) float32 and hits -- (n,12) int32
        or float32, or (n,48) uint8: n records of HIT_DTYPE -- are torch tensors on this context's GPU, both 16-byte aligned, or
        raw device pointers with n given.  has_w and stream as trace_rays_device takes them.
        hide: None, or an (n,) int32 tensor on the same GPU (pwn_trace_hits_hide_device): ray i does not see sphere hide[i] of the
        table in force; PWN_HIDE_NONE (-1) and every other value that is no sphere's index hide nothing."""
        who, hidden = "trace_hits_device", ("hide", hide, _I32, (None,), 4)
        if _tensors_given(who, (rays, hits)):
            n, dev = _check(who, [("rays", rays, _F32, (None, 8), 16), _hits_spec(hits)], [hidden], None if n is None else int(n))
            rays, hits = _ptr(rays), _ptr(hits)
        else:
            n, dev = _check(who, (), [hidden], _rays_n(who, n))
        _rays_n(who, n)
        _device_call(self, lib.pwn_trace_hits_hide_device if hide is not None else lib.pwn_trace_hits_device, stream, dev,
                     (n, rays, _lib.PWN_RAYS_HAS_W if has_w else 0, hits), hide, 2)

    # -- rays that stop after a given distance (pwn_trace_reach) ---------------
    def trace_reach(self, rays, reach):
        """pwn_trace_reach: trace_hits with a reach per ray -- (n,) float32, in the unit of the records' dist.  A ray that travels
        its reach and meets nothing gets kind PWN_HIT_FREE (3): face = object = -1, dist = reach, x y z the point it got to, dx dy dz
        the direction to fly on along (without a ramp's skew), portals and cell those of the step it stopped in.  +inf and NaN
        give trace_hits.  Returns (n,) HIT_DTYPE records."""
        rays = _ray_records(rays, "trace_reach")
        n = rays.shape[0]
        reach = np.ascontiguousarray(reach, np.float32)
        if reach.shape != (n,):
            raise ValueError("trace_reach: reach must be (%d,), not %s" % (n, reach.shape))
        hits = np.zeros(n, HIT_DTYPE)
        self._chk(lib.pwn_trace_reach(self._ctx, n, rays.ctypes.data if n else None, reach.ctypes.data if n else None,
                                      hits.ctypes.data if n else None), "pwn_trace_reach")
        return hits

    def trace_reach_device(self, rays, reach, hits, hide=None, has_w=False, stream=None):
        """pwn_trace_reach_device: one trace launch, stream-ordered, no synchronisation.  rays (n,8) float32, reach (n,) float32 and
        hits -- (n,12) int32 or float32, or (n,48) uint8: n records of HIT_DTYPE -- are torch tensors on this context's GPU, rays and
        hits 16-byte aligned.  has_w and stream as trace_hits_device takes them.
        hide: None, or an (n,) int32 tensor on the same GPU (pwn_trace_reach_hide_device): ray i does not see sphere hide[i] of the
        table in force; PWN_HIDE_NONE (-1) and every other value that is no sphere's index hide nothing."""
        who = "trace_reach_device"
        n, dev = _check(who, [("rays", rays, _F32, (None, 8), 16), ("reach", reach, _F32, (None,), 4), _hits_spec(hits)],
                        [("hide", hide, _I32, (None,), 4)])
        _rays_n(who, n)
        _device_call(self, lib.pwn_trace_reach_hide_device if hide is not None else lib.pwn_trace_reach_device, stream, dev,
                     (n, _ptr(rays), _ptr(reach), _lib.PWN_RAYS_HAS_W if has_w else 0, _ptr(hits)), hide, 3)

    def object_ids(self):
        """pwn_get_object_ids: per live sphere, in get_objects()' order (what a hit's `object` indexes), the obj_new handle"""
        n = self._chk(lib.pwn_get_object_ids(self._ctx, None, 0), "pwn_get_object_ids")
        ids = np.zeros(n, np.int32)
        if n:
            self._chk(lib.pwn_get_object_ids(self._ctx, ids.ctypes.data, n), "pwn_get_object_ids")
        return ids

    # -- first-hit planes of a batch of views (pwn_trace_view_hits) -------------
    def trace_view_hits(self, cams, want_cell=True, want_dist=True):
        """pwn_trace_view_hits: what is under every pixel of n views of this context's size.  cams (n,4,4) or (n,16).  Returns
        (label, cell, dist): label (n,h,w) uint32 packed words (unpack_labels takes them apart), cell (n,h,w,2) int16 cell x, z
        and dist (n,h,w) float32 -- cell / dist None where not wanted.  Pixel (x, y) of view i is the record trace_hits returns
        for pixel_rays(cams[i])'s ray of that pixel; a primary segment that ran out of steps gives 0 in all three."""
        cams = _cam_records(cams, "trace_view_hits")
        n = _count("trace_view_hits", "views (cams' rows)", cams.shape[0], 1, _lib.PWN_VIEWS_MAX)
        label = np.empty((n, self.h, self.w), np.uint32)
        cell = np.empty((n, self.h, self.w, 2), np.int16) if want_cell else None
        dist = np.empty((n, self.h, self.w), np.float32) if want_dist else None
        self._chk(lib.pwn_trace_view_hits(self._ctx, n, cams.ctypes.data, label.ctypes.data, cell.ctypes.data if want_cell else None,
                                          dist.ctypes.data if want_dist else None), "pwn_trace_view_hits")
        return label, cell, dist

    def trace_view_hits_device(self, cams, label, cell=None, dist=None, has_w=False, stream=None, hide=None):
        """pwn_trace_view_hits_device: the planes of trace_view_hits from cameras on the GPU into planes on the GPU, stream-ordered,
        no synchronisation and no host copy.  All torch tensors on this context's GPU, contiguous and 16-byte aligned: cams (n,16)
        or (n,4,4) float32, label (n,h,w) int32 or uint32, cell (n,h,w) int32 or uint32 -- or (n,h,w,2) int16 -- or None, dist
        (n,h,w) float32 or None.  Every pixel of every plane given is written.  has_w and stream as trace_views_device takes them.
        hide: None, or an (n,) int32 tensor (pwn_trace_view_hits_hide_device): view i does not see sphere hide[i] of the table in
        force (object numbers stay those of the whole table); values that are no sphere's index hide nothing."""
        who = "trace_view_hits_device"
        cams, plane = _cams16(cams), (None, self.h, self.w)
        n, dev = _check(who, [("cams", cams, _F32, (None, 16), 16), ("label", label, _WORDS, plane, 16)],
                        [_cell_spec(cell, plane), ("dist", dist, _F32, plane, 16), ("hide", hide, _I32, (None,), 4)])
        _count(who, "views (cams' rows)", n, 1, _lib.PWN_VIEWS_MAX)
        _device_call(self, lib.pwn_trace_view_hits_hide_device if hide is not None else lib.pwn_trace_view_hits_device, stream, dev,
                     (n, _ptr(cams), _lib.PWN_VIEWS_HAS_W if has_w else 0, _ptr(label), _ptr(cell), _ptr(dist)), hide, 2)

    # -- the players' step (pwn_players_step) ---------------------------------
    def players_step(self, keys, cams, gravity, traversals=None, tdiff=1 / 60, ticks=1):
        """pwn_players_step: `ticks` ticks of the reference's player motion (main.c:188-379, host/player.c) for n players on the level
        in force.  keys (n,) uint8 of PWN_MOVE_* bits, cams (n,16) or (n,4,4) float32, gravity (n,4) float32, traversals (n,) int32 or
        None.  Returns new arrays (cams, gravity, traversals) -- traversals None where none was given; the arguments are not changed."""
        who = "players_step"
        keys = np.asarray(keys)
        shape = np.shape(cams)
        cams_in = _cam_records(cams, who)
        n = cams_in.shape[0]
        gravity = np.asarray(gravity)
        if keys.shape != (n,) or keys.dtype != np.uint8:
            raise ValueError("%s: keys must be (%d,) uint8, not %s %s" % (who, n, keys.dtype, keys.shape))
        if gravity.shape != (n, 4):
            raise ValueError("%s: gravity must have shape (%d,4), not %s" % (who, n, gravity.shape))
        if traversals is not None and np.asarray(traversals).shape != (n,):
            raise ValueError("%s: traversals must have shape (%d,), not %s" % (who, n, np.asarray(traversals).shape))
        _players_numbers(who, n, tdiff, ticks)
        keys = np.ascontiguousarray(keys)
        out_c = np.array(cams_in, np.float32, order="C")
        out_g = np.array(gravity, np.float32, order="C")
        out_t = np.array(traversals, np.int32, order="C") if traversals is not None else None
        self._chk(lib.pwn_players_step(self._ctx, n, keys.ctypes.data if n else None, float(tdiff), int(ticks), out_c.ctypes.data if n else None,
                                       out_g.ctypes.data if n else None, out_t.ctypes.data if out_t is not None and n else None), "pwn_players_step")
        return out_c.reshape(shape), out_g, out_t

    def players_step_device(self, keys, cams, gravity, traversals=None, tdiff=1 / 60, ticks=1, stream=None):
        """pwn_players_step_device: the same on the GPU, in place, one launch on `stream` (a torch stream or a raw hipStream_t; None =
        torch's current stream), no synchronisation.  Torch tensors on this context's GPU, contiguous: keys (n,) uint8, cams (n,16) or
        (n,4,4) float32 and gravity (n,4) float32, both 16-byte aligned, traversals (n,) int32 or None.  cams is the tensor
        trace_views_device takes: step, then observe, on one stream."""
        who = "players_step_device"
        cams = _cams16(cams)
        n, dev = _check(who, [("cams", cams, _F32, (None, 16), 16), ("keys", keys, _U8, (None,), 1), ("gravity", gravity, _F32, (None, 4), 16)],
                        [("traversals", traversals, _I32, (None,), 4)])
        _players_numbers(who, n, tdiff, ticks)
        _device_call(self, lib.pwn_players_step_device, stream, dev,
                     (n, _ptr(keys), float(tdiff), int(ticks), _ptr(cams), _ptr(gravity), _ptr(traversals)))

    # -- pixel rays from cameras on the GPU (pwn_pixel_rays_device) ------------
    def pixel_rays_device(self, cams, xy=None, *, width=None, height=None, shared=None, rays=None, seeds=None, work=None, stream=None):
        """pwn_pixel_rays_device: pixel_rays for n cameras on the GPU, at most two launches on `stream` (a torch stream or a raw
        hipStream_t; None = torch's current stream), no synchronisation.  Torch tensors on this context's GPU, contiguous: cams (n,16)
        or (n,4,4) float32 -- the tensor players_step_device steps; xy (m,2) int32, pixels that every camera uses, or (n,m,2), each
        camera's own, or None: the whole width x height frame, row-major.  width / height: the frame the pixels belong to (default:
        the renderer's).  shared: None = what xy's shape says; given, it has to agree with it.  rays (n*m,8) or (n,m,8) float32,
        seeds (n*m,) or (n,m) int32 / uint32 -- or False: none is written -- and work (n,20) float32 scratch are made when not given.
        cams, work and rays 16-byte aligned, xy 8-byte aligned.  Returns (rays, seeds); ray i * m + j is camera i's pixel j, and
        trace_rays_device / trace_hits_device take them as they are (has_w for cameras with w components)."""
        import torch
        who = "pixel_rays_device"
        cams = _cams16(cams)
        n, dev = _check(who, [("cams", cams, _F32, (None, 16), 16)])
        _count(who, "cameras (cams' rows)", n, 0, _lib.PWN_PLAYERS_MAX)
        width, height = self.w if width is None else width, self.h if height is None else height
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v > 32768:
                raise ValueError("%s: %s must be an integer 1 ... 32768, not %r" % (who, name, v))
        width, height = int(width), int(height)
        if shared is not None and not isinstance(shared, (bool, np.bool_)):
            raise ValueError("%s: shared must be None, True or False, not %r" % (who, shared))
        if xy is None:
            if shared is not None and not shared:
                raise ValueError("%s: the whole frame (xy=None) is shared by every camera" % who)
            shared, m = True, width * height
        else:
            if getattr(xy, "ndim", 0) not in (2, 3):
                raise ValueError("%s: xy must be a GPU tensor of shape (m,2) or (n,m,2), or None" % who)
            m = int(xy.shape[-2])
            _check(who, [("xy", xy, _I32, (m, 2) if xy.ndim == 2 else (n, m, 2), 8)], device=dev)
            if shared is not None and bool(shared) != (xy.ndim == 2):
                raise ValueError("%s: shared=%s does not go with xy of shape %s" % (who, bool(shared), tuple(xy.shape)))
            shared = xy.ndim == 2
        total = _count(who, "cameras x pixels", n * m, 0, _lib.PWN_RAYS_MAX)
        _check(who, (), [("rays", rays, _F32, (n, m, 8) if getattr(rays, "ndim", 2) == 3 else (total, 8), 16),
                         ("seeds", None if seeds is False else seeds, _WORDS, (n, m) if getattr(seeds, "ndim", 1) == 2 else (total,), 4),
                         ("work", work, _F32, (n, _lib.PWN_PIXEL_WORK_BYTES // 4), 16)], device=dev)
        if rays is None:
            rays = torch.empty((total, 8), dtype=torch.float32, device=cams.device)
        if seeds is None:
            seeds = torch.empty(total, dtype=torch.int32, device=cams.device)
        elif seeds is False:
            seeds = None
        if work is None:
            work = torch.empty((n, _lib.PWN_PIXEL_WORK_BYTES // 4), dtype=torch.float32, device=cams.device)
        _device_call(self, lib.pwn_pixel_rays_device, stream, dev, (width, height, n, _ptr(cams), m, _ptr(xy), _lib.PWN_PIXELS_SHARED if shared else 0,
                                                                    _ptr(work), _ptr(rays), _ptr(seeds)))
        return rays, seeds

    # -- first-hit planes of views of their own sizes (pwn_trace_viewport_hits) --
    def trace_viewport_hits(self, rects, cams, want_cell=True, want_dist=True):
        """pwn_trace_viewport_hits: what is under every pixel of n views of their own sizes, in ONE frame of this context's size.
        rects (n,4) int (x, y, w, h), cams (n,4,4) or (n,16).  Returns (label, cell, dist): label (h,w) uint32 packed words
        (unpack_labels takes them apart), cell (h,w,2) int16 cell x, z and dist (h,w) float32 -- cell / dist None where not wanted.
        Pixel (x, y) of rectangle i is the record trace_hits returns for pixel_rays(w_i, h_i, cams[i])'s ray of that pixel; 0 in
        all three where the primary segment ran out of steps, and outside the rectangles."""
        rects = _rect_records(rects, "trace_viewport_hits")
        n = rects.shape[0]
        cams = _cam_records(cams, "trace_viewport_hits", n)
        label = np.empty((self.h, self.w), np.uint32)
        cell = np.empty((self.h, self.w, 2), np.int16) if want_cell else None
        dist = np.empty((self.h, self.w), np.float32) if want_dist else None
        self._chk(lib.pwn_trace_viewport_hits(self._ctx, n, rects.ctypes.data, cams.ctypes.data, label.ctypes.data,
                                              cell.ctypes.data if want_cell else None, dist.ctypes.data if want_dist else None),
                  "pwn_trace_viewport_hits")
        return label, cell, dist

    def trace_viewport_hits_device(self, layout, cams, label, cell=None, dist=None, has_w=False, stream=None, hide=None):
        """pwn_trace_viewport_hits_device: the planes of trace_viewport_hits for the views of a viewports_layout, from cameras on the
        GPU into ONE frame of the layout's W x H on the GPU, stream-ordered, no synchronisation and no host copy.  All torch tensors
        on this context's GPU, contiguous and 16-byte aligned: cams (n,16) or (n,4,4) float32, camera i for rectangle i; label (H,W)
        int32 or uint32; cell (H,W) int32 or uint32 -- or (H,W,2) int16 -- or None; dist (H,W) float32 or None.  Every pixel of
        every rectangle is written in every plane given, nothing outside them.  has_w and stream as trace_views_device takes them.
        hide as trace_viewports_device takes it (pwn_trace_viewport_hits_hide_device); object numbers in the labels stay those of the
        full table."""
        who = "trace_viewport_hits_device"
        _live_layout(who, self, layout)
        cams, plane = _cams16(cams), (layout.H, layout.W)
        _, dev = _check(who, [("cams", cams, _F32, (None, 16), 16), ("label", label, _WORDS, plane, 16)],
                        [_cell_spec(cell, plane), ("dist", dist, _F32, plane, 16), ("hide", hide, _I32, (None,), 4)], n=layout.n)
        _device_call(self, lib.pwn_trace_viewport_hits_hide_device if hide is not None else lib.pwn_trace_viewport_hits_device, stream, dev,
                     (layout._ptr, _ptr(cams), _lib.PWN_VIEWS_HAS_W if has_w else 0, _ptr(label), _ptr(cell), _ptr(dist)), hide, 2)

    def set_call_strips(self, n):
        """PWN_OPT_CALL_STRIPS: -1 = by frame size (default), 0 = one launch per pass, 2..32 = that many row strips"""
        self._chk(lib.pwn_set_option(self._ctx, _lib.PWN_OPT_CALL_STRIPS, int(n)), "pwn_set_option(CALL_STRIPS)")

    def call_strips_state(self):
        v = (C.c_ulonglong * 6)()
        self._chk(lib.pwn_call_strips_state(self._ctx, v), "pwn_call_strips_state")
        opt = int(v[0])
        return {"option": opt - (1 << 64) if opt >= (1 << 63) else opt, "strips_last": int(v[1]), "calls_in_strips": int(v[2]), "redone": int(v[3]),
                "copy_streams": int(v[4]), "reach_depth": int(v[5])}

    def host_register(self, arr):
        """pwn_host_register: the host's frame buffer (main.c:395-400), made known to the device once"""
        self._chk(lib.pwn_host_register(self._ctx, arr.ctypes.data, arr.nbytes), "pwn_host_register")

    def host_unregister(self, arr):
        self._chk(lib.pwn_host_unregister(self._ctx, arr.ctypes.data), "pwn_host_unregister")

    # -- frames in flight (main.c:93-109 with the hand-over to the host overlapped) ----------
    def frames_config(self, nslots, sbuf=True, zbuf=False, surface_scale=0, pitch_bytes=0):
        flags = (_lib.PWN_FRAME_SBUF if sbuf else 0) | (_lib.PWN_FRAME_ZBUF if zbuf else 0) | \
                (_lib.PWN_FRAME_SURFACE if surface_scale else 0)
        self._chk(lib.pwn_frames_config(self._ctx, int(nslots), flags, int(surface_scale), int(pitch_bytes)), "pwn_frames_config")
        self._frame_scale = int(surface_scale)

    def submit_frame(self, cam, sec_current, slot):
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        self._chk(lib.pwn_submit_frame(self._ctx, cam.ctypes.data, float(sec_current), int(slot)), "pwn_submit_frame")

    def frame_ready(self, slot):
        return bool(self._chk(lib.pwn_frame_ready(self._ctx, int(slot)), "pwn_frame_ready"))

    def wait_frame(self, slot):
        """Blocks until the slot's frame is on the host.  Returns a dict of numpy VIEWS of the
        library's pinned buffers (valid until the next submit on that slot) and device times."""
        fr = _lib.Frame()
        self._chk(lib.pwn_wait_frame(self._ctx, int(slot), C.byref(fr)), "pwn_wait_frame")
        out = {"seq": fr.seq, "sec": fr.sec_current, "timed": bool(fr.timed),
               "trace_ms": fr.trace_ms, "blur_ms": fr.blur_ms, "sink_ms": fr.sink_ms,
               "d_sbuf": fr.d_sbuf, "d_zbuf": fr.d_zbuf, "d_surface": fr.d_surface}
        n = self.w * self.h

        def view(ptr, ctype, count, shape):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,)).reshape(shape)
        if fr.sbuf:
            out["sbuf"] = view(fr.sbuf, C.c_uint32, n, (self.h, self.w))
        if fr.zbuf:
            out["zbuf"] = view(fr.zbuf, C.c_float, n, (self.h, self.w))
        if fr.surface:
            pw = fr.surface_pitch_bytes // 4
            out["surface"] = view(fr.surface, C.c_uint32, pw * self.h * self._frame_scale, (self.h * self._frame_scale, pw))
        return out

    def read_plane(self, d_ptr, dtype=np.uint32):
        """Host copy of a (h, w) device plane of a waited-for frame (wait_frame()["d_sbuf"] ...)."""
        out = np.empty((self.h, self.w), dtype)
        self._chk(lib.pwn_read_plane(self._ctx, C.c_void_p(d_ptr), out.ctypes.data, out.nbytes), "pwn_read_plane")
        return out

    def trace_rows_device(self, cam, sec_current, y0, y1, d_sbuf, d_zbuf, stream=0):
        """Rows [y0,y1) into device frames given as raw device pointers."""
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        self._chk(lib.pwn_trace_rows_device(self._ctx, cam.ctypes.data, float(sec_current), int(y0), int(y1),
                                            C.c_void_p(d_sbuf), C.c_void_p(d_zbuf), C.c_void_p(stream)),
                  "pwn_trace_rows_device")

    def blur_rows_device(self, y0, y1, d_pre, d_zbuf, d_out, stream=0):
        self._chk(lib.pwn_blur_rows_device(self._ctx, int(y0), int(y1), C.c_void_p(d_pre), C.c_void_p(d_zbuf),
                                           C.c_void_p(d_out), C.c_void_p(stream)), "pwn_blur_rows_device")

    def blur_rows_device_bounded(self, y0, y1, d_pre, d_zbuf, d_out, avail_y0, avail_y1, d_miss, stream=0):
        """blur_rows_device when only rows [avail_y0, avail_y1) of d_pre are this frame's;
        taps outside add to the uint32 at d_miss."""
        self._chk(lib.pwn_blur_rows_device_bounded(self._ctx, int(y0), int(y1), C.c_void_p(d_pre), C.c_void_p(d_zbuf),
                                                   C.c_void_p(d_out), int(avail_y0), int(avail_y1), C.c_void_p(d_miss),
                                                   C.c_void_p(stream)), "pwn_blur_rows_device_bounded")

    # -- row tiling over the GPUs of a node (one process per GPU; RCCL inside the library) ----
    @staticmethod
    def tiled_unique_id(transport="rccl"):
        """rank 0: 128 bytes to hand to the other ranks"""
        buf = C.create_string_buffer(_lib.PWN_TILED_ID_BYTES)
        rc = lib.pwn_tiled_unique_id(buf, _lib.PWN_TRANSPORT_SHM if transport == "shm" else _lib.PWN_TRANSPORT_RCCL)
        if rc != 0:
            raise PwnError(rc, "pwn_tiled_unique_id(%s)" % transport)
        return buf.raw

    def tiled_init(self, rank, world, uid, transport="rccl", halo_rows=-1):
        self._chk(lib.pwn_tiled_init(self._ctx, int(rank), int(world), C.c_char_p(uid),
                                     _lib.PWN_TRANSPORT_SHM if transport == "shm" else _lib.PWN_TRANSPORT_RCCL, int(halo_rows)),
                  "pwn_tiled_init(rank %d of %d, %s)" % (rank, world, transport))

    def tiled_submit(self, cam, sec_current=0.0):
        cam = np.ascontiguousarray(cam, np.float32).reshape(16)
        self._chk(lib.pwn_tiled_submit(self._ctx, cam.ctypes.data, float(sec_current)), "pwn_tiled_submit")

    def tiled_wait(self, host=False):
        """Oldest frame in flight.  The frame's root (rank 0, or rank (seq - 1) mod world after tiled_gather_root(True)):
        dict with d_sbuf (device pointer) and, with host=True, sbuf (numpy view of the pinned copy); other ranks: dict
        without them ("root" says which rank has it).  With a host sink
        (tiled_host_sink) every rank gets sbuf, a view of the frame in the shared host memory."""
        fr = _lib.TiledFrame()
        self._chk(lib.pwn_tiled_wait(self._ctx, _lib.PWN_TILED_HOST if host else 0, C.byref(fr)), "pwn_tiled_wait")
        out = {"seq": fr.seq, "redone": bool(fr.redone), "d_sbuf": fr.d_sbuf, "timed": bool(fr.timed),
               "trace_ms": fr.trace_ms, "frame_ms": fr.frame_ms, "blur_ms": fr.blur_ms, "halo_ms": fr.halo_ms,
               "gather_ms": fr.gather_ms, "enqueue_us": fr.enqueue_us, "y0": fr.y0, "y1": fr.y1, "cost": fr.cost, "root": fr.root}
        if fr.sbuf:
            out["sbuf"] = np.ctypeslib.as_array(C.cast(fr.sbuf, C.POINTER(C.c_uint32)), shape=(self.w * self.h,)).reshape(self.h, self.w)
        return out

    def tiled_host_sink(self, buf):
        """Deliver frames to the host from every rank: `buf` is writable host memory for PWN_TILED_SLOTS whole
        frames (a numpy array, an mmap of POSIX shared memory ...), the same memory in every rank."""
        arr = np.frombuffer(buf, np.uint8)
        self._host_sink = (buf, arr)                      # keep it mapped for as long as the context lives
        self._chk(lib.pwn_tiled_host_sink(self._ctx, arr.ctypes.data, arr.size), "pwn_tiled_host_sink")

    def tiled_gather_root(self, rotate):
        """pwn_tiled_gather_root: frames gathered on rank 0 (False, the default) or on rank f mod world in turn (True);
        the same call on every rank, with no frame in flight."""
        self._chk(lib.pwn_tiled_gather_root(self._ctx, 1 if rotate else 0), "pwn_tiled_gather_root")

    def tiled_info(self):
        inf = _lib.TiledInfo()
        self._chk(lib.pwn_tiled_get_info(self._ctx, C.byref(inf)), "pwn_tiled_get_info")
        return {n: getattr(inf, n) for n, _ in _lib.TiledInfo._fields_}

    def tiled_shutdown(self):
        lib.pwn_tiled_shutdown(self._ctx)

    def tiled_set_timeouts(self, init_s=None, wait_s=None):
        """pwn_tiled_set_timeouts: how long pwn_tiled_init / pwn_tiled_wait may wait for the other ranks before they
        return PWN_ETIMEDOUT (seconds; None keeps a value, a negative number restores the default)."""
        ms = [0 if v is None else (-1 if v < 0 else max(1, int(v * 1000))) for v in (init_s, wait_s)]
        self._chk(lib.pwn_tiled_set_timeouts(self._ctx, ms[0], ms[1]), "pwn_tiled_set_timeouts")

    def tiled_preflight(self):
        """pwn_tiled_preflight as a dict: visible devices, peer access from this context's device, the librccl that
        dlopen resolved and its version, how the communicator will be driven, the deadlines."""
        import json
        buf = C.create_string_buffer(2048)
        self._chk(lib.pwn_tiled_preflight(self._ctx, buf, len(buf)), "pwn_tiled_preflight")
        return json.loads(buf.value.decode())

    def tiled_balance(self, every_frames):
        """Moving cuts: re-cut the strips every `every_frames` delivered frames from what they cost (0: leave them)."""
        self._chk(lib.pwn_tiled_balance(self._ctx, int(every_frames)), "pwn_tiled_balance")

    def tiled_set_cuts(self, cuts):
        """world + 1 row boundaries for the next submitted frames; the same call on every rank."""
        a = np.ascontiguousarray(cuts, np.int32)
        self._chk(lib.pwn_tiled_set_cuts(self._ctx, a.ctypes.data, len(a)), "pwn_tiled_set_cuts")

    def tiled_get_cuts(self):
        """(cuts of the next frame [world + 1], every rank's cost word of the last delivered frame [world])"""
        cuts = np.zeros(_lib.PWN_TILED_MAX_WORLD + 1, np.int32)
        cost = np.zeros(_lib.PWN_TILED_MAX_WORLD, np.uint32)
        n = self._chk(lib.pwn_tiled_get_cuts(self._ctx, cuts.ctypes.data, cost.ctypes.data), "pwn_tiled_get_cuts")
        return cuts[:n].copy(), cost[:n - 1].copy()

    def tiled_set_reserve(self, workgroups):
        """workgroups the persistent trace grid leaves free for RCCL's kernels (this rank, between frames)"""
        self._chk(lib.pwn_tiled_set_reserve(self._ctx, int(workgroups)), "pwn_tiled_set_reserve")

    # -- sink (screen.h:126-149) ----------------------------------------------
    def screen_upscale(self, sbuf, scale, pitch_bytes=None, pixels=None):
        scale = int(scale)
        if pitch_bytes is None:
            pitch_bytes = self.w * scale * 4
        if pixels is None:
            pixels = np.zeros((self.h * scale, pitch_bytes // 4), np.uint32)
        src = None
        if sbuf is not None:
            sbuf = np.ascontiguousarray(sbuf, np.uint32)
            src = sbuf.ctypes.data
        self._chk(lib.pwn_screen_upscale(self._ctx, src, scale, int(pitch_bytes), pixels.ctypes.data),
                  "pwn_screen_upscale")
        return pixels

    def upscale_device(self, d_src, scale, pitch_bytes, d_dst, stream=0):
        self._chk(lib.pwn_upscale_device(self._ctx, C.c_void_p(d_src), int(scale), int(pitch_bytes),
                                         C.c_void_p(d_dst), C.c_void_p(stream)), "pwn_upscale_device")

    # -- stats / probes --------------------------------------------------------
    def stats(self):
        st = _lib.Stats()
        self._chk(lib.pwn_get_stats(self._ctx, C.byref(st)), "pwn_get_stats")
        out = {n: getattr(st, n) for n, _ in _lib.Stats._fields_ if n != "reserved_"}
        out["wave_paths"] = list(st.wave_paths)
        out["regions"] = list(st.regions)
        return out

    def probe(self, op, words):
        words = np.ascontiguousarray(words).view(np.uint32).ravel()
        per = {_lib.PROBE_DIV: 2, _lib.PROBE_FTOINT: 4}.get(op, 1)
        n = words.size // per
        out = np.zeros(n, np.uint32)
        self._chk(lib.pwn_probe(self._ctx, int(op), words.ctypes.data, out.ctypes.data, n), "pwn_probe")
        return out


def _tables_dict(out):
    return {"form": int(out[0]), "lds_bytes": int(out[1]), "device_bytes": int(out[2]), "pairs": int(out[3]),
            "cells": int(out[4]), "longest": int(out[5])}


def sphere_tables_plan(spheres):
    """pwn_sphere_tables_plan: what an upload of these spheres would do -- the form of the per-cell lists (0 indexed, 1 inline,
    2 in device memory), LDS bytes per workgroup, bytes in device memory, (cell, sphere) pairs, non-empty cells, the longest
    list.  No context, no device.  Raises PwnError(PWN_ETOOBIG) for tables that no form holds."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    out = (C.c_uint64 * 6)()
    buf = spheres if len(spheres) else np.zeros(1, SPHERE_DTYPE)
    rc = lib.pwn_sphere_tables_plan(buf.ctypes.data, len(spheres), out)
    if rc < 0:
        raise PwnError(rc, "pwn_sphere_tables_plan")
    return _tables_dict(out)


def sphere_bounds_plan(spheres):
    """pwn_sphere_bounds_plan: the bounding balls the next upload of these spheres would make for its longest per-cell lists (the
    trace kernels skip a list whose ball no ray of a wave can meet).  No context, no device.  A list of dicts, longest list first:
    cell (z * 64 + x), records, id (the list's id in its cell's word), centre (x, y, z), r_eff, rr."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    out = np.zeros((4, 8), np.float64)
    buf = spheres if len(spheres) else np.zeros(1, SPHERE_DTYPE)
    rc = lib.pwn_sphere_bounds_plan(buf.ctypes.data, len(spheres), out.ctypes.data)
    if rc < 0:
        raise PwnError(rc, "pwn_sphere_bounds_plan")
    return [{"cell": int(o[0]), "records": int(o[1]), "id": int(o[2]), "centre": (float(o[3]), float(o[4]), float(o[5])),
             "r_eff": float(o[6]), "rr": float(o[7])} for o in out[:rc]]


class ViewportsLayout:
    """A layout of Renderer.viewports_layout (pwn_vp_layout): frame size W x H and n rectangles, for trace_viewports_device."""

    def __init__(self, renderer, ptr, W, H, n):
        self._renderer, self._ptr, self.W, self.H, self.n = renderer, ptr, W, H, n

    def info(self):
        """pwn_viewports_layout_info: dict(W, H, n, units, pixels, blur_ok)"""
        if self._ptr is None:
            raise ValueError("ViewportsLayout.info: the layout was freed")
        out = (C.c_uint64 * 6)()
        rc = lib.pwn_viewports_layout_info(self._ptr, out)
        if rc != 0:
            raise PwnError(rc, "pwn_viewports_layout_info")
        d = dict(zip(("W", "H", "n", "units", "pixels"), (int(v) for v in out)))
        d["blur_ok"] = bool(out[5])
        return d

    def free(self):
        """pwn_viewports_layout_free: waits for the last launches that read the layout, then frees it (once; later calls do nothing)"""
        if self._ptr is None:
            return
        ptr, self._ptr = self._ptr, None
        r = self._renderer
        if self in (getattr(r, "_layouts", None) or []):
            r._layouts.remove(self)
        r._chk(lib.pwn_viewports_layout_free(r._ctx, ptr), "pwn_viewports_layout_free")


def _rect_records(rects, who):
    """(n,4) int32 rectangles (x, y, w, h), the layout of pwn_viewport"""
    rects = np.asarray(rects)
    if rects.ndim != 2 or rects.shape[1] != 4 or rects.shape[0] < 1:
        raise ValueError("%s: rects must have shape (n,4) with n >= 1, not %s" % (who, rects.shape))
    if rects.shape[0] > _lib.PWN_VIEWS_MAX:
        raise ValueError("%s: %d rectangles, at most %d" % (who, rects.shape[0], _lib.PWN_VIEWS_MAX))
    return np.ascontiguousarray(rects, np.int32)


def _cam_records(cams, who, n=None):
    """(n,16) float32 cameras from an (n,4,4) or (n,16) array; n given: exactly so many"""
    cams = np.asarray(cams)
    if cams.ndim == 3 and cams.shape[1:] == (4, 4):
        cams = cams.reshape(cams.shape[0], 16)
    if cams.ndim != 2 or cams.shape[1] != 16 or (n is not None and cams.shape[0] != n):
        raise ValueError("%s: cams must have shape (n,4,4) or (n,16)%s, not %s" % (who, "" if n is None else " with n = %d" % n, cams.shape))
    return np.ascontiguousarray(cams, np.float32)


def viewports_plan(W, H, rects, blur):
    """pwn_viewports_plan: what pwn_trace_viewports would make of these rectangles (n,4: x, y, w, h) in a W x H frame under `blur`
    passes.  No context, no device.  Returns a dict: ok (the call would accept them), units (16 x 4 units of the launch), pixels
    (covered), largest (units of the largest view), offender (index of the first rectangle that breaks a rule, or n)."""
    rects = _rect_records(rects, "viewports_plan")
    out = (C.c_uint64 * 4)()
    rc = lib.pwn_viewports_plan(int(W), int(H), int(blur), rects.shape[0], rects.ctypes.data, out)
    if rc not in (_lib.PWN_OK, _lib.PWN_EINVAL):
        raise PwnError(rc, "pwn_viewports_plan")
    return {"ok": rc == _lib.PWN_OK, "units": int(out[0]), "pixels": int(out[1]), "largest": int(out[2]), "offender": int(out[3])}


def _ray_records(rays, who):
    """(n,8) float32 records from an (n,8) array or a pair (origins, directions) of (n,3) / (n,4) arrays (w lanes 1 and 0)"""
    if isinstance(rays, (tuple, list)) and len(rays) == 2:
        o, d = np.asarray(rays[0]), np.asarray(rays[1])
        if o.ndim != 2 or d.ndim != 2 or o.shape[0] != d.shape[0] or o.shape[1] not in (3, 4) or d.shape[1] not in (3, 4):
            raise ValueError("%s: origins and directions must be (n,3) or (n,4) with the same n, not %s and %s" % (who, o.shape, d.shape))
        rec = np.zeros((o.shape[0], 8), np.float32)
        rec[:, 3] = 1.0
        rec[:, :o.shape[1]] = o
        rec[:, 4:4 + d.shape[1]] = d
        return rec
    rays = np.asarray(rays)
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError("%s: rays must have shape (n,8) or be a pair (origins, directions), not %s" % (who, rays.shape))
    if rays.shape[0] > _lib.PWN_RAYS_MAX:
        raise ValueError("%s: %d rays, at most %d" % (who, rays.shape[0], _lib.PWN_RAYS_MAX))
    return np.ascontiguousarray(rays, np.float32)


def unpack_labels(label):
    """The fields of trace_view_hits' label words (PWN_LABEL_* of pwnhip.h): (kind, face, object, portals), int32 arrays of
    label's shape.  0 = nothing hit: kind PWN_HIT_NONE, face and object -1, portals 0."""
    l = np.asarray(label).astype(np.uint32)
    return ((l & 3).astype(np.int32), ((l >> 2) & 7).astype(np.int32) - 1, ((l >> 5) & 0x3fff).astype(np.int32) - 1,
            (l >> 19).astype(np.int32))


def pack_labels(hits):
    """unpack_labels' inverse, from HIT_DTYPE records (trace_hits): kind | (face + 1) << 2 | (object + 1) << 5 | portals << 19,
    uint32 of hits' shape"""
    hits = np.asarray(hits)
    if hits.dtype != HIT_DTYPE:
        raise ValueError("pack_labels: records of HIT_DTYPE, not %s" % (hits.dtype,))
    u = lambda f, add=0: (hits[f].astype(np.int64) + add).astype(np.uint32)
    return u("kind") | (u("face", 1) << np.uint32(2)) | (u("object", 1) << np.uint32(5)) | (u("portals") << np.uint32(19))


def _players_numbers(who, n, tdiff, ticks):
    if n > _lib.PWN_PLAYERS_MAX:
        raise ValueError("%s: %d players, at most %d" % (who, n, _lib.PWN_PLAYERS_MAX))
    if int(ticks) != ticks or not 1 <= ticks <= _lib.PWN_TICKS_MAX:
        raise ValueError("%s: ticks must be 1..%d, not %r" % (who, _lib.PWN_TICKS_MAX, ticks))
    with np.errstate(over="ignore"):
        tdiff32 = np.float32(tdiff)
    if not np.isfinite(tdiff32):
        raise ValueError("%s: tdiff must be finite, not %r" % (who, tdiff))


def players_spawn(spawn, n):
    """pwn_player_init's state (main.c:59-64) for n players: (cams (n,16) float32, gravity (n,4) float32, traversals (n,) int32) --
    the identity camera at the centre of the spawn cell, height 0.5, no gravity, no portal walked through."""
    cams = np.zeros((int(n), 16), np.float32)
    cams[:, 0] = cams[:, 5] = cams[:, 10] = cams[:, 15] = 1.0
    cams[:, 12] = np.float32(0.5) + np.float32(int(spawn[0]))
    cams[:, 13] = 0.5
    cams[:, 14] = np.float32(0.5) + np.float32(int(spawn[1]))
    return cams, np.zeros((int(n), 4), np.float32), np.zeros(int(n), np.int32)


# -- the device forms' argument checks and calls: a method is its specs, _check, _device_call ----------------
_F32, _I32, _I16, _U8, _WORDS = ("float32",), ("int32",), ("int16",), ("uint8",), ("int32", "uint32")


def _cams16(cams):
    """a contiguous (n,4,4) camera tensor seen as (n,16), what the library reads; anything else as it is, for _check to judge"""
    import torch
    if isinstance(cams, torch.Tensor) and cams.dim() == 3 and tuple(cams.shape[1:]) == (4, 4) and cams.is_contiguous():
        cams = cams.view(cams.shape[0], 16)
    return cams


_DTYPE_NAMES = {}         # torch.dtype -> "float32" ..., filled as dtypes are met (str(dtype) costs more than the rest of a check)


def _check(who, required, optional=(), n=None, device=None):
    """The argument check of a device form.  A spec is (name, tensor, dtype names, shape, alignment in bytes); a shape that begins
    with None has n rows, and the first such tensor sets n where none is given.  ValueError unless every tensor -- of `optional`,
    those that are not None -- is a contiguous GPU tensor of one of its dtypes and exactly its shape, starts at a multiple of its
    alignment and is on GPU `device` (none given: the first tensor's).  Refuses nothing else; returns (n, device)."""
    import torch
    for specs, needed in ((required, True), (optional, False)):
        for name, t, dtypes, shape, align in specs:
            if t is None and not needed:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError("%s: %s must be a GPU tensor" % (who, name))
            if shape[0] is None:
                if n is None and t.dim():
                    n = t.shape[0]
                shape = (n,) + shape[1:]
            dtype = _DTYPE_NAMES.get(t.dtype) or _DTYPE_NAMES.setdefault(t.dtype, str(t.dtype)[6:])
            if dtype not in dtypes or t.shape != shape or not t.is_contiguous():
                raise ValueError("%s: %s must be a contiguous %s tensor of shape %s, not %s %s" % (
                    who, name, "/".join(dtypes), shape, dtype, tuple(t.shape)))
            if t.data_ptr() % align != 0:
                raise ValueError("%s: %s is not %d-byte aligned" % (who, name, align))
            if device is None:
                device = t.get_device()
            elif t.get_device() != device:
                raise ValueError("%s: %s is on GPU %d, not on GPU %d" % (who, name, t.get_device(), device))
    return n, device


def _count(who, what, n, lo, hi):
    if not lo <= n <= hi:
        raise ValueError("%s: %s = %d, %d ... %d" % (who, what, n, lo, hi))
    return n


def _rays_n(who, n):
    """the ray count of a form that also takes raw pointers: given -- by the caller or by rays' rows -- and 0 ... PWN_RAYS_MAX"""
    if n is None:
        raise ValueError("%s: n is needed with device pointers" % who)
    return _count(who, "n", int(n), 0, _lib.PWN_RAYS_MAX)


def _cell_spec(cell, shape):
    """a cell plane: a word per pixel, or -- elements of two bytes -- a pair of int16 per pixel"""
    if getattr(cell, "itemsize", 4) == 2:
        return ("cell", cell, _I16, shape + (2,), 16)
    return ("cell", cell, _WORDS, shape, 16)


def _hits_spec(hits):
    """n records of HIT_DTYPE: (n,12) int32 or float32, or (n,48) uint8"""
    return ("hits", hits, ("int32", "float32", "uint8"), (None, HIT_DTYPE.itemsize // (getattr(hits, "itemsize", 4) or 4)), 16)


def _live_layout(who, r, layout):
    if not isinstance(layout, ViewportsLayout) or layout._ptr is None or layout._renderer is not r:
        raise ValueError("%s: layout must be a live ViewportsLayout of this renderer" % who)


def _tensors_given(who, args):
    """device arrays come as tensors or as raw device pointers (ints): True for tensors, False for pointers, ValueError for both"""
    raw = len([a for a in args if isinstance(a, int)])
    if 0 < raw < len(args):
        raise ValueError("%s: give all tensors or all device pointers" % who)
    return raw < len(args)


def _ptr(t):
    """the pointer of a tensor as the library takes it: None for no tensor and for an empty one"""
    return None if t is None else t.data_ptr() or None


def _stream_handle(stream, device):
    """a raw hipStream_t of a torch stream, of a raw handle, or of None: torch's current stream on GPU `device` (no device: stream 0)"""
    if stream is None:
        if device is None:
            return 0
        import torch
        stream = torch.cuda.current_stream(device)
    return stream if isinstance(stream, int) else stream.cuda_stream


def _device_call(r, fn, stream, device, args, hide=None, at=None):
    """fn(ctx, *args, stream) on the renderer r, checked; with hide, fn is the _hide_device form: hide's pointer goes in at args[at]"""
    if hide is not None:
        args = args[:at] + (_ptr(hide),) + args[at:]
    r._chk(fn(r._ctx, *args, _stream_handle(stream, device)), fn.__name__)


def unit_order_xy(width, height):
    """every pixel of a width x height frame in the trace kernel's 16x4-pixel units, units row by row, a unit's pixels row by row
    (pixels outside the frame left out): (w*h, 2) int32 x, y"""
    uy, ux, r, c = np.meshgrid(np.arange((height + 3) // 4), np.arange((width + 15) // 16), np.arange(4), np.arange(16), indexing="ij")
    x, y = (ux * 16 + c).ravel(), (uy * 4 + r).ravel()
    keep = (x < width) & (y < height)
    return np.stack([x[keep], y[keep]], 1).astype(np.int32)


def pixel_rays(width, height, cam, xy=None, order="rows"):
    """pwn_pixel_rays (no context, no GPU): (rays (n,8) float32, seeds (n,) uint32, xy (n,2) int32) of pixels xy of camera cam's
    width x height frame, exactly as the frame kernel makes them; trace_rays on them gives that frame's pre-blur colour and depth.
    xy=None: every pixel, row-major (order="rows") or in the frame kernel's 16x4-pixel units (order="units", unit_order_xy)."""
    cam = np.asarray(cam)
    if cam.size != 16:
        raise ValueError("pixel_rays: cam must have 16 elements, not %s" % (cam.shape,))
    cam = np.ascontiguousarray(cam, np.float32).reshape(16)
    width, height = int(width), int(height)
    if xy is None:
        if order == "rows":
            yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
            xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)
        elif order == "units":
            xy = unit_order_xy(width, height)
        else:
            raise ValueError('pixel_rays: order must be "rows" or "units", not %r' % (order,))
    else:
        xy = np.asarray(xy)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("pixel_rays: xy must have shape (n,2), not %s" % (xy.shape,))
        xy = np.ascontiguousarray(xy, np.int32)
    n = xy.shape[0]
    rays = np.empty((n, 8), np.float32)
    seeds = np.empty(n, np.uint32)
    rc = lib.pwn_pixel_rays(width, height, cam.ctypes.data, n, xy.ctypes.data, rays.ctypes.data, seeds.ctypes.data)
    if rc < 0:
        raise PwnError(rc, "pwn_pixel_rays(%dx%d)" % (width, height))
    return rays, seeds, xy


# camera helpers the host uses to pose the view (util.h:61-110; outside the
# kernel path, restated for drivers and tests)
def mat4_iden():
    return np.eye(4, dtype=np.float32)


def mat4_roty(m, ang):
    m = np.array(m, np.float32).reshape(4, 4).copy()
    vs, vc = np.float32(np.sin(np.float32(ang))), np.float32(np.cos(np.float32(ang)))
    vxx, vxz, vzx, vzz = m[0, 0], m[0, 2], m[2, 0], m[2, 2]
    m[0, 0] = vc * vxx + vs * vxz
    m[0, 2] = vc * vxz - vs * vxx
    m[2, 0] = vc * vzx + vs * vzz
    m[2, 2] = vc * vzz - vs * vzx
    return m


def mat4_rotx(m, ang):
    m = np.array(m, np.float32).reshape(4, 4).copy()
    vs, vc = np.float32(np.sin(np.float32(ang))), np.float32(np.cos(np.float32(ang)))
    vyy, vyz, vzy, vzz = m[1, 1], m[1, 2], m[2, 1], m[2, 2]
    m[1, 1] = vc * vyy + vs * vyz
    m[1, 2] = vc * vyz - vs * vyy
    m[2, 1] = vc * vzy + vs * vzz
    m[2, 2] = vc * vzz - vs * vzy
    return m


def spawn_camera(spawn, ang_y=0.0, ang_x=0.0):
    """mainloop's camera (main.c:61-64): identity at the spawn cell centre,
    optionally turned like the arrow keys do (main.c:188-193)."""
    cam = mat4_iden()
    if ang_y:
        cam = mat4_roty(cam, ang_y)
    if ang_x:
        cam = mat4_rotx(cam, ang_x)
    cam[3, 0], cam[3, 1], cam[3, 2] = spawn[0] + 0.5, 0.5, spawn[1] + 0.5
    return cam
