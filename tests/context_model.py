"""The contract of a context (include/pwnhip.h: `depth`, `left alone`, `not followed`, `ordering`) as code, and random call
sequences to hold the library to it.  CPU only: the oracle (tests/oracle.py), hard_scenes.Plane's rule, tests/hit_chain.py and
tests/big_scenes.py; nothing here needs a GPU.

    Model(W, H)                  what a context of W x H holds, every operation a method of the oracle's alone:
                                   the level, the object table and the live spheres, the options;
                                   one depth plane of the blocking call and its last colour (pwn_screen_upscale(NULL));
                                   a growing list of view slots' depth planes; one W x H depth plane of the viewports;
                                   one depth plane per frame slot, zero after EVERY pwn_frames_config, and the frame each slot
                                   was submitted (traced from the tables in force at its submit);
                                   nothing for rays, hits and view-hits;
                                   for the device forms the caller's planes, which are the state: dev_z (pwn_trace_views_device)
                                   and rows_pre / rows_z / rows_out (the strip forms) stand for the test's tensors.
    generate(seed, n_ops, profile)   a deterministic list of operation records: plain data (dicts of numbers, strings and lists)
    Model.inputs(rec)            the record's cameras, pixels and spheres as arrays (both sides are given the same ones)
    Model.apply(rec, inputs)     the expected outputs, bit for bit, or {"err": code}; Model.log has one entry per operation for
                                 the coverage conditions of tests/test_context_model.py
    SEEDS                        the sequences tests/test_gpu_context_model.py runs: (seed, profile, n_ops)

Where the header was silent the model says what the code does, and the header now says it too: a frame slot's depth plane is its
own and starts from zero with every pwn_frames_config; a frame in flight under two or more blur passes leaves its first pass in
the plane pwn_screen_upscale(NULL) reads.

What is compared by sample, not in full: the label and cell planes of pwn_trace_view_hits.  The oracle gives a first-hit record
only through its event chain (hit_chain.Reader), a pixel at a time; so the distance plane and "label == 0 exactly where the primary
ray runs out of steps" are compared at every pixel, no pixel may keep the poison, and label and cell bit for bit at SAMPLE pixels
a view.  The five counters: where the oracle cannot give one (sphere tests of primary segments, steps of whole first-hit planes)
the model leaves it out.
"""
import os

import numpy as np

import big_scenes as BS
import hit_chain as HC
import oracle
from conftest import GOLD, level_path, load_spheres
from handout import POISON_S, POISON_Z

OK, EINVAL, ENOLEVEL, EBUSY = 0, -1, -6, -8
LEVELS = ("pwnfps_level", "synth64", "synth256")
OWN = {"pwnfps_level": ("t0", 0, 14), "synth64": ("synth64", 100, 64), "synth256": ("synth256", 200, 128)}   # table, first uid, spheres
BIG, BIG_UID, BIG_N = "swarm_near", 1000, 2100      # (2 100 spheres: more than 2 047, so the lists go to device memory, form 2)
NEW_UID = 5000
W_LANES = (0.03, -0.01, 0.05, 0.8)                  # the w column of a camera "with w components" (tests/test_gpu_views_device.py)
SAMPLE = 24                                         # pixels a view whose label and cell are read off the oracle's event chain
SENT = np.uint32(POISON_Z)
FAMILY = {"frame": "a", "views": "b", "views_dev": "c", "viewports": "d", "rays": "e", "hits": "f", "view_hits": "g",
          "config": "h", "submit": "h", "wait": "h", "rows": "i", "upscale": "j"}
FAMILIES = "abcdefghij"
LAUNCHING = "abcdefghi"
BLURRED = "abcdh"
PLANE_OWNERS = "abdh"
# one workgroup per CU (tests/test_gpu_handout.py): at 336 x 208 a frame has 1 092 units, more than the 1 024 waves of that grid
PROFILES = {
    "small": {"w": 96, "h": 64, "env": {}},                                   # as tests/test_gpu_frames.py against the oracle
    "odd": {"w": 50, "h": 20, "env": {}},                                     # w % 4 != 0: every blurred call with passes > 0 is refused
    "strips": {"w": 48, "h": 160, "env": {}},                                 # forced call strips cut 2 or 3 strips of 64 / 96 rows
    "one_per_cu": {"w": 336, "h": 208, "env": {"PWN_DBG_BLOCKS_PER_CU": "1"}},
}
SEEDS = [(1, "small", 160), (2, "small", 160), (3, "odd", 160), (4, "strips", 160), (5, "small", 160), (6, "small", 160), (7, "odd", 160),
         (8, "strips", 160), (9, "small", 160), (10, "small", 160), (11, "one_per_cu", 96), (12, "small", 160)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def strips_of(h, k):
    """strips of a blocking call under PWN_OPT_CALL_STRIPS = k: whole 32-row blur tiles (tests/test_gpu_variants.py _strips)"""
    per = ((h + k - 1) // k + 31) // 32 * 32
    return (h + per - 1) // per


def layouts(W, H):
    """the viewport layouts: rectangles (x, y, w, h) that touch; x and w multiples of 4 where W is, heights that are not.
    0 the whole frame, 1 and 3 cover it, 2 leaves the bottom right uncovered"""
    a, b = (W // 2) & ~3, H // 2 - 3
    return [[(0, 0, W, H)],
            [(0, 0, a, H), (a, 0, W - a, b), (a, b, W - a, H - b)],
            [(0, 0, a, b), (a, 0, W - a, b), (0, b, a, H - b)],
            [(0, 0, W, b), (0, b, a, H - b), (a, b, W - a, H - b)]]


_tables = {}


def table(spec, level):
    """a sphere table by name, every sphere marked with a uid of its own through its reflectivity, (uid + 1) / 32 (the trick of
    hit_chain.mark_spheres): the oracle's event chain prints the reflectivity of the sphere a ray ends on"""
    key = (spec, level if spec != "big" and spec != "none" else None)
    if key not in _tables:
        if spec == "none":
            s = np.zeros(0, oracle.SPHERE_DTYPE)
        elif spec == "big":
            s = _marked(BS.scene(BIG, oracle).spheres, BIG_UID)
            assert len(s) == BIG_N
        else:
            name, uid, n = OWN[level]
            s = _marked(load_spheres(name), uid)
            assert len(s) == n
            if spec.startswith("trunc:"):
                s = s[:int(spec[6:])]
            else:
                assert spec == "own", spec
        s.setflags(write=False)
        _tables[key] = s
    return _tables[key]


def _marked(sph, uid):
    s = np.ascontiguousarray(sph, oracle.SPHERE_DTYPE).copy()
    s["refl"] = (np.arange(len(s), dtype=np.float32) + np.float32(uid + 1)) / np.float32(32)
    return s


def uids(sph):
    return np.rint(sph["refl"].astype(np.float64) * 32.0).astype(np.int64) - 1


_file_cams = {}


def file_cams(level):
    if level not in _file_cams:
        _file_cams[level] = np.load(os.path.join(GOLD, "levels", level + "_cams.npy")).astype(np.float32).reshape(-1, 4, 4)
    return _file_cams[level]


def pixels_of(pix, W, H):
    """the pixels of a record: ["rand", seed, n] n different pixels, ["rows", [y ...]] whole rows"""
    if pix[0] == "rows":
        return np.array([(x, y) for y in pix[1] for x in range(W)], np.int32).reshape(-1, 2)
    pick = np.random.default_rng(pix[1]).choice(W * H, min(pix[2], W * H), replace=False)
    return np.stack([pick % W, pick // W], 1).astype(np.int32)


def pack_label(rec):
    u = lambda f, add=0: (rec[f].astype(np.int64) + add).astype(np.uint32)
    return u("kind") | (u("face", 1) << np.uint32(2)) | (u("object", 1) << np.uint32(5)) | (u("portals") << np.uint32(19))


def pack_cell(rec):
    return (rec["cell_x"].astype(np.int64) & 0xffff).astype(np.uint32) | ((rec["cell_z"].astype(np.int64) & 0xffff).astype(np.uint32) << np.uint32(16))


def _sum5(parts):
    return tuple(int(sum(p[i] for p in parts)) for i in range(5))


def _st5(st):
    return (st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted)


class Model:
    def __init__(self, W, H, track=False):
        """track: also find, with a second trace over a sentinel plane, the primary rays that run out of steps, and note in
        the log where one keeps a non-zero depth that a different camera left (the CPU test's coverage condition)"""
        self.W, self.H, self.track = W, H, track
        self.O = oracle.Oracle()
        self.level, self.spawn = None, (0, 0)
        self.objs, self.typ = [], []                       # the object table: sphere records, "inval" / "free" / "sphere"
        self.live = np.zeros(0, oracle.SPHERE_DTYPE)       # the table the kernels read, as of the last upload
        self.form2 = False
        self.blur, self.counters, self.sched, self.unit_order, self.strips, self.overlap = 1, False, "units", False, -1, True
        z = lambda: np.zeros((H, W), np.float32)
        self.new_plane = z
        self.block_z, self.block_col = z(), np.zeros((H, W), np.uint32)
        self.view_z = []
        self.vp_z, self.vp_cover = z(), None
        self.slots, self.frame_flags, self.frame_seq = [], (False, False, 0), 0
        self.dev_z = [z() for _ in range(4)]
        self.rows_pre, self.rows_z, self.rows_out = np.zeros((H, W), np.uint32), z(), np.zeros((H, W), np.uint32)
        self.counted = None                                # who made the last counted launch (a frame in flight: its seq)
        self.writers, self.cam_ids = {}, {}
        self.switch = None
        self.log = []
        self._persist = set()

    # ---- inputs ----
    def camera(self, spec):
        import pwnfps_amd
        if spec[0] == "s":
            cam = pwnfps_amd.spawn_camera(self.spawn, ang_y=spec[1], ang_x=spec[2])
        else:
            cam = file_cams(spec[1])[spec[2]].copy()
        cam = np.ascontiguousarray(cam, np.float32).reshape(4, 4)
        if spec[3]:
            cam[:, 3] = W_LANES
        return cam

    def inputs(self, rec):
        inp = {}
        if "cam" in rec:
            inp["cams"] = self.camera(rec["cam"])[None]
        if "cams" in rec:
            inp["cams"] = np.stack([self.camera(c) for c in rec["cams"]])
        if "pix" in rec:
            inp["xy"] = pixels_of(rec["pix"], self.W, self.H)
        if rec["op"] == "objects":
            inp["spheres"] = table(rec["table"], self.level)
        if rec["op"] == "viewports":
            inp["rects"] = np.array(layouts(self.W, self.H)[rec["layout"]], np.int32)
        return inp

    @staticmethod
    def _eff(cam, has_w):
        """the camera a device form sees without its HAS_W flag: the w lanes taken as 0, 0, 0, 1"""
        if has_w:
            return cam
        cam = cam.copy()
        cam[:, 3] = (0, 0, 0, 1)
        return cam

    # ---- the oracle's side of a launch ----
    def _blur(self, pre, z, passes):
        cur = pre
        for _ in range(passes):
            cur = self.O.blur_rows(0, pre.shape[0], cur, z)
        return cur

    def _shoot(self, cam, sec, z, owner=None, wkey=None, wview=None):
        """a whole frame of z's size on depth plane z: (pre-blur colour, depth, the five counters)"""
        h, w = z.shape
        sb, z2, st = self.O.trace_rows(w, h, 0, h, cam, sec=np.float32(sec), zb=z.copy())
        if self.track and owner is not None:
            s = np.full((h, w), SENT, np.uint32).view(np.float32)
            _, s, _ = self.O.trace_rows(w, h, 0, h, cam, sec=np.float32(sec), zb=s)
            ex = bits(s) == SENT
            writer = self.writers.setdefault(wkey, np.full((self.H, self.W), -1, np.int64))
            wv = writer if wview is None else writer[wview]
            cid = self.cam_ids.setdefault(cam.tobytes(), len(self.cam_ids))
            if (ex & (bits(z) != 0) & (wv >= 0) & (wv != cid)).any():
                self._persist.add(owner)
            wv[~ex] = cid
        return sb, z2, _st5(st)

    def _refuse(self, blurs=True):
        if blurs and self.blur > 0 and self.W % 4 != 0:
            return {"err": EINVAL}
        if self.level is None:
            return {"err": ENOLEVEL}
        return None

    def _in_flight(self):
        return [i for i, s in enumerate(self.slots) if s["in_flight"]]

    def _stats(self, out, st5, keys=None):
        """the counters of a launch that is complete when the caller compares: with PWN_OPT_COUNTERS on, and no frame in flight
        (a frame in flight and a launch on a stream of the caller's may run side by side, on one set of counters)"""
        self.counted = None
        if self.counters and not self._in_flight():
            names = ("rays", "steps", "portals", "sphere_tests", "exhausted")
            out["stats"] = {k: int(v) for k, v in zip(names, st5) if keys is None or k in keys}

    # ---- state changes ----
    def _upload(self, sph):
        import pwnfps_amd
        self.live = np.ascontiguousarray(sph, oracle.SPHERE_DTYPE).copy()
        if self.level is not None:
            self.O.set_spheres(self.live)
        form2 = pwnfps_amd.sphere_tables_plan(self.live)["form"] == 2
        if form2 != self.form2:
            self.switch = "to2" if form2 else "from2"
        self.form2 = form2
        return {"form2": form2}

    def op_level(self, rec, inp):
        self.level = rec["level"]
        self.O.load_level(level_path(self.level))
        self.O.set_spheres(self.live)
        self.spawn = tuple(int(v) for v in self.O.get_level()[2])
        return {}

    def op_objects(self, rec, inp):
        self.objs = [tuple(s) for s in inp["spheres"].tolist()]
        self.typ = ["sphere"] * len(self.objs)
        return self._upload(inp["spheres"])

    def op_obj_new(self, rec, inp):
        for i, t in enumerate(self.typ):
            if t == "free":
                self.typ[i] = "inval"
                return {"ret": i}
        self.objs.append(None)
        self.typ.append("inval")
        return {"ret": len(self.typ) - 1}

    def op_obj_set(self, rec, inp):
        self.objs[rec["obj"]] = tuple(np.array(rec["sphere"], np.float64).astype(np.float32).tolist())   # (doubles, narrowed on store)
        self.typ[rec["obj"]] = "sphere"
        return {}

    def op_obj_free(self, rec, inp):
        self.typ[rec["obj"]] = "free"
        return {}

    def op_prepare(self, rec, inp):
        if "inval" in self.typ:
            return {"err": EINVAL}                         # an object created but never set; the tables stay
        live = [o for o, t in zip(self.objs, self.typ) if t == "sphere"]
        return self._upload(np.array(live, oracle.SPHERE_DTYPE) if live else np.zeros(0, oracle.SPHERE_DTYPE))

    def op_blur(self, rec, inp):
        if self._in_flight():
            return {"err": EBUSY}
        self.blur = rec["n"]
        return {}

    def op_overlap(self, rec, inp):
        if self._in_flight():
            return {"err": EBUSY}
        self.overlap = bool(rec["on"])
        return {}

    def op_counters(self, rec, inp):
        self.counters = bool(rec["on"])
        return {}

    def op_sched(self, rec, inp):
        self.sched = rec["which"]
        return {}

    def op_unit_order(self, rec, inp):
        self.unit_order = bool(rec["on"])
        return {}

    def op_strips(self, rec, inp):
        self.strips = rec["n"]
        return {}

    # ---- (a) the blocking call ----
    def op_frame(self, rec, inp):
        no = self._refuse()
        if no:
            return no
        pre, self.block_z, st5 = self._shoot(inp["cams"][0], rec["sec"], self.block_z, "a", "block")
        self.block_col = self._blur(pre, self.block_z, self.blur)
        can = self.blur <= 1 and not self.counters and not self.unit_order
        out = {"sbuf": self.block_col, "zbuf": self.block_z,
               "strips": strips_of(self.H, self.strips) if can and self.strips >= 2 else 1}
        self._stats(out, st5)
        return out

    # ---- (b) view slots ----
    def op_views(self, rec, inp):
        no = self._refuse()
        if no:
            return no
        n = len(inp["cams"])
        while len(self.view_z) < n:
            self.view_z.append(self.new_plane())
        sb, zb, parts = [], [], []
        for i in range(n):
            pre, self.view_z[i], st5 = self._shoot(inp["cams"][i], rec["secs"][i], self.view_z[i], "b", ("view", i))
            sb.append(self._blur(pre, self.view_z[i], self.blur))
            zb.append(self.view_z[i])
            parts.append(st5)
        out = {"sbuf": np.stack(sb), "zbuf": np.stack(zb)}
        self._stats(out, _sum5(parts))
        return out

    # ---- (c) the device form: the caller's planes ----
    def op_views_dev(self, rec, inp):
        no = self._refuse()
        if no:
            return no
        n = len(inp["cams"])
        sb, parts = [], []
        for i in range(n):
            pre, self.dev_z[i], st5 = self._shoot(self._eff(inp["cams"][i], rec["has_w"]), rec["secs"][i], self.dev_z[i])
            sb.append(self._blur(pre, self.dev_z[i], self.blur))
            parts.append(st5)
        out = {"sbuf": np.stack(sb), "zbuf": np.stack(self.dev_z[:n])}
        self._stats(out, _sum5(parts))
        return out

    # ---- (d) viewports ----
    def op_viewports(self, rec, inp):
        rects = [tuple(int(v) for v in r) for r in inp["rects"]]
        if self.blur > 0 and (self.W % 4 != 0 or any(x % 4 or w % 4 for x, _, w, _ in rects)):
            return {"err": EINVAL}
        if self.level is None:
            return {"err": ENOLEVEL}
        col = np.zeros((self.H, self.W), np.uint32)
        cover = np.zeros((self.H, self.W), bool)
        parts = []
        for i, (x, y, w, h) in enumerate(rects):
            sl = (slice(y, y + h), slice(x, x + w))
            pre, z, st5 = self._shoot(inp["cams"][i], rec["secs"][i], np.ascontiguousarray(self.vp_z[sl]), "d", "vp", sl)
            self.vp_z[sl] = z
            col[sl] = self._blur(pre, z, self.blur)
            cover[sl] = True
            parts.append(st5)
        # outside the rectangles colour reads 0 and zbuf is the plane as it stands: seen where the call before covered
        self._entry["vp_outside_after_cover"] = bool(self.vp_cover is not None and (self.vp_cover & ~cover & (bits(self.vp_z) != 0)).any())
        self.vp_cover = cover
        out = {"sbuf": col, "zbuf": self.vp_z.copy()}
        self._stats(out, _sum5(parts))
        return out

    # ---- (e) rays ----
    def op_rays(self, rec, inp):
        no = self._refuse(blurs=False)
        if no:
            return no
        cam = self._eff(inp["cams"][0], rec["has_w"]) if rec["dev"] else inp["cams"][0]
        xy = inp["xy"]
        sb = np.zeros((self.H, self.W), np.uint32)
        z = np.full((self.H, self.W), SENT, np.uint32).view(np.float32)
        if rec["pix"][0] == "rows":
            parts = []
            for y in rec["pix"][1]:
                sb, z, st = self.O.trace_rows(self.W, self.H, y, y + 1, cam, sec=np.float32(rec["sec"]), sb=sb, zb=z)
                parts.append(_st5(st))
            st5 = _sum5(parts)
        else:
            sb, z, _ = self.O.trace_rows(self.W, self.H, 0, self.H, cam, sec=np.float32(rec["sec"]), sb=sb, zb=z)
            st5 = None
        out = {"col": sb[xy[:, 1], xy[:, 0]], "depth": bits(z)[xy[:, 1], xy[:, 0]]}
        if st5 is not None:
            self._stats(out, st5)
        else:
            self.counted = None
        return out

    # ---- (f) hits ----
    def _records(self, cam, xy):
        ref = HC.Reader(self.O).pixels(self.W, self.H, cam, xy)
        want = ref.want.copy()
        sph = want["kind"] == HC.SPHERE
        if sph.any():
            live = uids(self.live)
            for i in np.flatnonzero(sph):
                (at,) = np.flatnonzero(live == want["object"][i])         # (the chain gives the uid; the record wants its place in the live table)
                want["object"][i] = at
        return want, ref

    def op_hits(self, rec, inp):
        no = self._refuse(blurs=False)
        if no:
            return no
        cam = self._eff(inp["cams"][0], rec["has_w"]) if rec["dev"] else inp["cams"][0]
        want, ref = self._records(cam, inp["xy"])
        out = {"hits": want, "cmp_dy": ref.cmp_dy}
        self._stats(out, (len(want), int(ref.steps.sum()), int(want["portals"].sum()), 0, int((want["kind"] == HC.NONE).sum())),
                    keys=("rays", "steps", "portals", "exhausted"))
        return out

    # ---- (g) first-hit planes ----
    def op_view_hits(self, rec, inp):
        no = self._refuse(blurs=False)
        if no:
            return no
        n = len(inp["cams"])
        dist, none, sxy, slabel, scell = [], [], [], [], []
        rng = np.random.default_rng(rec["sample"])
        for i in range(n):
            cam = self._eff(inp["cams"][i], rec["has_w"]) if rec["dev"] else inp["cams"][i]
            s = np.full((self.H, self.W), SENT, np.uint32).view(np.float32)
            _, s, _ = self.O.trace_rows(self.W, self.H, 0, self.H, cam, sec=np.float32(0.0), zb=s)
            ex = bits(s) == SENT
            dist.append(np.where(ex, np.uint32(0), bits(s)))
            none.append(ex)
            pick = rng.choice(self.W * self.H, SAMPLE, replace=False)
            xy = np.stack([pick % self.W, pick // self.W], 1).astype(np.int32)
            want, _ = self._records(cam, xy)
            sxy.append(xy)
            slabel.append(np.where(want["kind"] == HC.NONE, np.uint32(0), pack_label(want)))
            scell.append(np.where(want["kind"] == HC.NONE, np.uint32(0), pack_cell(want)))
        none = np.stack(none)
        out = {"dist": np.stack(dist), "none": none, "sample_xy": np.stack(sxy), "sample_label": np.stack(slabel), "sample_cell": np.stack(scell)}
        self._stats(out, (n * self.W * self.H, 0, 0, 0, int(none.sum())), keys=("rays", "exhausted"))
        return out

    # ---- (h) frames in flight ----
    def op_config(self, rec, inp):
        if self._in_flight():
            return {"err": EBUSY}
        # every configuration allocates its slots afresh: depth planes from zero, nothing submitted
        self.slots = [{"z": self.new_plane(), "in_flight": False, "frame": None, "id": (self.frame_seq, i)} for i in range(rec["n"])]
        self.frame_flags = (bool(rec["sbuf"]), bool(rec["zbuf"]), int(rec["surface"]))
        return {}

    def op_submit(self, rec, inp):
        if rec["slot"] >= len(self.slots):
            return {"err": EINVAL}
        no = self._refuse()
        if no and no["err"] == EINVAL:
            return no
        sl = self.slots[rec["slot"]]
        if sl["in_flight"]:
            return {"err": EBUSY}
        if no:
            return no
        # the frame is the one of the tables, options and level in force NOW, whatever is uploaded before its wait
        pre, sl["z"], st5 = self._shoot(inp["cams"][0], rec["sec"], sl["z"], "h", ("slot",) + sl["id"])
        col = self._blur(pre, sl["z"], self.blur)
        if self.blur >= 2:
            # (the passes take turns on the blocking call's two planes and the last lands in the slot's: the first is left
            # where pwn_screen_upscale(NULL) reads)
            self.block_col = self._blur(pre, sl["z"], 1)
        self.frame_seq += 1
        sl["in_flight"] = True
        sl["frame"] = {"sbuf": col, "zbuf": sl["z"], "seq": self.frame_seq, "sec": bits(np.float32(rec["sec"])).item()}
        if self.frame_flags[2]:
            sl["frame"]["surface"] = self.O.upscale(col, self.frame_flags[2])
        self.counted = (self.frame_seq, st5) if self.counters else None
        return {}

    def op_wait(self, rec, inp):
        if rec["slot"] >= len(self.slots) or self.slots[rec["slot"]]["frame"] is None:
            return {"err": EINVAL}
        sl = self.slots[rec["slot"]]
        sl["in_flight"] = False
        out = dict(sl["frame"])
        if self.counted is not None and self.counted[0] == out["seq"]:
            self._stats(out, self.counted[1])
        return out

    # ---- (i) the strip forms ----
    def op_rows(self, rec, inp):
        if self.level is None:
            return {"err": ENOLEVEL}
        y0, y1 = rec["y0"], rec["y1"]
        cam = inp["cams"][0]
        self.rows_pre, self.rows_z, st = self.O.trace_rows(self.W, self.H, y0, y1, cam, sec=np.float32(rec["sec"]),
                                                           sb=self.rows_pre.copy(), zb=self.rows_z.copy())
        out = {"pre": self.rows_pre, "zbuf": self.rows_z}
        if self.W % 4 != 0:
            out["blur_err"] = EINVAL                       # (the blur stores 16-byte groups: refused whatever PWN_OPT_BLUR_PASSES says)
        else:
            self.rows_out = self.O.blur_rows(y0, y1, self.rows_pre, self.rows_z, out=self.rows_out.copy())
            out["blur_err"] = OK
        out["out"] = self.rows_out
        self._stats(out, _st5(st))
        return out

    # ---- (j) the sink ----
    def op_upscale(self, rec, inp):
        return {"pixels": self.O.upscale(self.block_col, rec["scale"])}

    def apply(self, rec, inp=None):
        if inp is None:
            inp = self.inputs(rec)
        fam = FAMILY.get(rec["op"], "-")              # ("-": a state change)
        self._entry = {"op": rec["op"], "fam": fam, "form2": self.form2, "blur": self.blur, "after_switch": None}
        self._persist = set()
        out = getattr(self, "op_" + rec["op"])(rec, inp)
        err = out.get("err", OK)
        self._entry["err"] = err
        if rec["op"] == "rows" and out.get("blur_err"):
            self._entry["err"] = out["blur_err"]
        if rec["op"] == "overlap" and err == EBUSY:
            self._entry["overlap_busy"] = True
        if rec["op"] == "submit" and err == EBUSY:
            self._entry["slot_busy"] = True
        if err == OK and fam in LAUNCHING and rec["op"] not in ("config", "wait") and self.switch is not None:
            self._entry["after_switch"], self.switch = self.switch, None
        self._entry["persist"] = sorted(self._persist)
        self._entry["ran"] = err == OK and fam != "-" and rec["op"] not in ("config", "wait")
        self.log.append(self._entry)
        return out


# ---------------------------------------------------------------- random sequences ----

EXHAUSTING = ["f", "synth256", 0, 0]          # synth256's first camera: a primary ray runs out of steps (tests/test_gpu_views.py)
BEFORE_IT = ["f", "synth256", 1, 0]           # ... where its second camera sees a wall


def tour():
    """the families in an order in which every ordered pair (A directly followed by B) occurs: an Euler circuit of the complete
    directed graph with loops on the ten families, 101 long"""
    n = len(FAMILIES)
    out, nxt = [], {a: list(range(n)) for a in range(n)}
    stack = [0]
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == n * n + 1
    return [FAMILIES[i] for i in out]


class _Gen:
    """the generator's shadow of a context: just enough to emit records that are legal where they are meant to be"""

    def __init__(self, seed, profile, index, of):
        p = PROFILES[profile]
        self.W, self.H = p["w"], p["h"]
        self.rng = np.random.default_rng(seed)
        self.index, self.of = index, of
        self.ops = []
        self.level = None
        self.blur, self.counters = 1, False
        self.nslots, self.flying, self.submitted = 0, set(), set()
        self.typ = []
        self.big = False

    # -- random pieces
    def r(self, lo, hi):
        return round(float(self.rng.uniform(lo, hi)), 3)

    def cam(self):
        k = self.rng.integers(10)
        w = int(self.rng.integers(4) == 0)
        # (a level's camera file only while that level is loaded: elsewhere its poses stand inside walls)
        if k == 0 and self.level == "synth256":
            return [EXHAUSTING[0], EXHAUSTING[1], EXHAUSTING[2], w]
        if k <= 2 and self.level in ("synth64", "synth256"):
            return ["f", self.level, int(self.rng.integers(4)), w]
        return ["s", self.r(0, 6.283), self.r(-0.6, 0.6), w]

    def sec(self):
        return self.r(0, 50)

    def flip(self):
        return bool(self.rng.integers(2))

    def emit(self, op, **kw):
        self.ops.append(dict(op=op, **kw))

    # -- state changes
    def set_blur(self, n):
        if self.flying:
            self.drain()
        self.emit("blur", n=int(n))
        self.blur = int(n)

    def drain(self):
        for s in sorted(self.flying):
            self.emit("wait", slot=s)
        self.flying.clear()

    def set_level(self, name):
        self.emit("level", level=name)
        self.level = name

    def set_objects(self, spec):
        self.emit("objects", table=spec)
        self.big = spec == "big"
        n = {"none": 0, "big": BIG_N}.get(spec)
        if n is None:
            n = OWN[self.level][2] if spec == "own" else int(spec[6:])
        self.typ = ["sphere"] * n

    def small_table(self):
        k = int(self.rng.integers(3))
        return ("none", "own", "trunc:%d" % self.rng.integers(1, OWN[self.level][2]))[k]

    def state_change(self):
        k = int(self.rng.integers(12))
        if k == 0:
            self.set_blur(0 if (self.W % 4 and self.rng.integers(3)) else self.rng.integers(4))
        elif k == 1:
            self.counters = self.flip()
            self.emit("counters", on=self.counters)
        elif k == 2:
            self.emit("sched", which=("units", "refill")[int(self.rng.integers(2))])
        elif k == 3:
            self.emit("unit_order", on=self.flip())
        elif k == 4:
            self.emit("strips", n=int((0, 2, 3, 4)[self.rng.integers(4)]))
        elif k == 5:
            self.emit("overlap", on=self.flip())           # (PWN_EBUSY while frames are in flight: the model says so)
        elif k == 6:
            self.set_level(LEVELS[int(self.rng.integers(3))])
        elif k == 7 and not self.big:
            self.set_objects(self.small_table())
        elif k >= 8 and not self.big:
            self.edit_objects()

    def new_sphere(self):
        self.uid = getattr(self, "uid", NEW_UID) + 1
        # r, refl, x, y, z, b, g, r -- somewhere around where the levels' spawn cells are; the uid in the reflectivity
        return [self.r(0.05, 0.3), (self.uid + 1) / 32.0, self.r(5, 56), self.r(0.3, 0.6), self.r(1, 26), self.r(0.1, 1), self.r(0.1, 1), self.r(0.1, 1)]

    def edit_objects(self):
        k = int(self.rng.integers(4))
        live = [i for i, t in enumerate(self.typ) if t == "sphere"]
        if k == 0 and live:
            i = int(live[self.rng.integers(len(live))])
            self.emit("obj_free", obj=i)
            self.typ[i] = "free"
        elif k == 1 and live:
            self.emit("obj_set", obj=int(live[self.rng.integers(len(live))]), sphere=self.new_sphere())
        else:
            i = self.typ.index("free") if "free" in self.typ else len(self.typ)
            self.emit("obj_new")
            if i == len(self.typ):
                self.typ.append("inval")
            if k == 3:
                self.emit("prepare")                       # PWN_EINVAL: created but never set
            self.emit("obj_set", obj=i, sphere=self.new_sphere())
            self.typ[i] = "sphere"
        self.emit("prepare")

    # -- one operation of a family
    def family(self, f, cam=None, slot=None, layout=None, views=None):
        rng = self.rng
        c = (lambda: list(cam)) if cam is not None else self.cam
        foreign = self.flip()
        if f == "a":
            self.emit("frame", cam=c(), sec=self.sec())
        elif f in "bc":
            n = views or int(rng.integers(1, 5))
            kw = dict(cams=[c() for _ in range(n)], secs=[self.sec() for _ in range(n)])
            if f == "b":
                self.emit("views", **kw)
            else:
                self.emit("views_dev", has_w=self.flip(), foreign=foreign, **kw)
        elif f == "d":
            lay = int(rng.integers(4)) if layout is None else layout
            n = len(layouts(self.W, self.H)[lay])
            self.emit("viewports", layout=lay, cams=[c() for _ in range(n)], secs=[self.sec() for _ in range(n)])
        elif f == "e":
            if self.counters or rng.integers(3) == 0:
                pix = ["rows", sorted(int(y) for y in rng.choice(self.H, 3, replace=False))]
            else:
                pix = ["rand", int(rng.integers(1 << 30)), int(rng.integers(1, 400))]
            self.emit("rays", cam=c(), sec=self.sec(), pix=pix, dev=self.flip(), has_w=self.flip(), foreign=foreign)
        elif f == "f":
            self.emit("hits", cam=c(), pix=["rand", int(rng.integers(1 << 30)), int(rng.integers(1, 65))], dev=self.flip(), has_w=self.flip(), foreign=foreign)
        elif f == "g":
            n = int(rng.integers(1, 3))
            self.emit("view_hits", cams=[c() for _ in range(n)], sample=int(rng.integers(1 << 30)), dev=self.flip(), has_w=self.flip(), foreign=foreign)
        elif f == "h":
            self.frames_step(c, slot)
        elif f == "i":
            y0 = int(rng.integers(1, self.H - 6))
            y0 += 1 if y0 % 4 == 0 else 0
            y1 = int(rng.integers(y0 + 1, self.H + 1))
            y1 -= 1 if (y1 % 4 == 0 and y1 - 1 > y0) else 0
            self.emit("rows", cam=c(), sec=self.sec(), y0=y0, y1=y1, foreign=foreign)
        elif f == "j":
            self.emit("upscale", scale=int(rng.integers(1, 4)))

    def config(self, n=None):
        self.drain()
        n = int(self.rng.integers(2, 5)) if n is None else n
        self.emit("config", n=n, sbuf=self.flip(), zbuf=self.flip(), surface=int((0, 0, 2)[self.rng.integers(3)]))
        self.nslots, self.submitted = n, set()

    def frames_step(self, c, slot=None):
        """one record of the frames in flight: a configuration where there is none, a submit where a slot is free, else a wait"""
        free = [s for s in range(self.nslots) if s not in self.flying]
        if self.nslots == 0:
            self.config()
        elif slot is not None or (free and (not self.flying or self.rng.integers(3))):
            s = slot if slot is not None else int(free[self.rng.integers(len(free))])
            if s in self.flying:
                self.emit("wait", slot=s)
                self.flying.discard(s)
            self.emit("submit", slot=s, cam=c(), sec=self.sec())
            if self.level is not None and not (self.blur > 0 and self.W % 4):
                self.flying.add(s)
                self.submitted.add(s)
        else:
            s = int(sorted(self.flying)[self.rng.integers(len(self.flying))])
            self.emit("wait", slot=s)
            self.flying.discard(s)

    def random_op(self):
        if self.rng.integers(4) == 0:
            self.state_change()
        else:
            self.family(FAMILIES[int(self.rng.integers(len(FAMILIES)))])

    # -- the blocks every sequence has (the coverage conditions of tests/test_context_model.py, by construction)
    def block_persist(self):
        """every plane-owning family is shown synth256's second camera and then its first, whose exhausted primary ray keeps the
        second's depth; the families' calls in one another's way, and neighbouring planes shown something else in between so
        that a plane taken for another shows: view slot 1 and frame slot 0 a camera of their own, and, before a third round of
        one view, one viewport and frame slot 1, the blocking plane a third camera -- which its own last frame then keeps"""
        self.set_level("synth256")
        if self.big:
            self.set_objects("own")
        self.set_blur(0 if self.W % 4 else self.rng.integers(4))
        self.drain()
        if self.nslots < 2:
            self.config()
        other = lambda: ["s", self.r(0, 6.283), self.r(-0.3, 0.3), 0]
        for rnd, cam in enumerate((BEFORE_IT, EXHAUSTING, EXHAUSTING)):
            if rnd == 2:
                self.emit("frame", cam=other(), sec=self.sec())
            for f in self.rng.permutation(list(PLANE_OWNERS)):
                if f == "h":
                    self.family("h", cam=cam, slot=1)
                    if rnd < 2:
                        self.family("h", cam=(other() if rnd == 0 else cam), slot=0)
                elif f == "d":
                    self.family("d", cam=cam, layout=0)
                elif f == "b" and rnd == 0:
                    self.emit("views", cams=[list(cam), other()], secs=[self.sec(), self.sec()])
                elif f == "b":
                    self.family("b", cam=cam, views=(2 if rnd == 1 else 1))
                elif rnd < 2:
                    self.family("a", cam=cam)
            if rnd == 0 and self.flip():
                self.family("efgij"[int(self.rng.integers(5))])
        self.family("a", cam=EXHAUSTING)
        self.drain()

    def block_restart(self):
        """pwn_frames_config(0) and a new configuration: the slots' depth planes start from zero again"""
        self.set_level("synth256")
        self.set_blur(0 if self.W % 4 else self.blur)
        if self.nslots == 0:
            self.config()
        self.family("h", cam=BEFORE_IT, slot=0)
        self.config(0)
        self.config()
        self.family("h", cam=EXHAUSTING, slot=0)
        self.drain()

    def block_blur(self, combos):
        for f, p in combos:
            self.set_blur(p)
            if f == "h" and self.nslots == 0:
                self.config()
            self.family(f, slot=(0 if f == "h" else None))
            if f == "h" and 0 in self.flying and self.flip():
                self.family("abcdefgij"[int(self.rng.integers(9))])      # another family's call between the submit and its wait
        self.drain()

    def block_form(self, to_fam, in_fams, from_fam):
        """the tables into device memory and back, a given family right behind each switch"""
        if self.level is None:
            self.set_level("pwnfps_level")
        if self.W % 4:
            self.set_blur(0)
        for f in (to_fam, from_fam) + tuple(in_fams):
            if f == "h" and self.nslots == 0:
                self.config()
        self.set_objects("big")
        self.one_that_runs(to_fam)
        for f in in_fams:
            self.one_that_runs(f)
            if self.flip():
                self.random_family_op()
        if self.flip():
            self.emit("level", level=LEVELS[int(self.rng.integers(3))])      # (the level changes under tables in device memory)
            self.level = self.ops[-1]["level"]
        self.set_objects(self.small_table() if self.flip() else "own")
        self.one_that_runs(from_fam)

    def one_that_runs(self, f):
        if f == "h":
            if 0 in self.flying:
                self.emit("wait", slot=0)
                self.flying.discard(0)
            self.family("h", slot=0)
        else:
            self.family(f)

    def random_family_op(self):
        self.family(FAMILIES[int(self.rng.integers(len(FAMILIES)))])

    def block_errors(self):
        """a busy slot, and PWN_OPT_FRAME_OVERLAP while a frame is in flight"""
        if self.level is None:
            self.set_level("synth64")
        if self.W % 4:
            self.set_blur(0)
        if self.nslots == 0:
            self.config()
        if 0 not in self.flying:
            self.family("h", slot=0)
        self.emit("submit", slot=0, cam=self.cam(), sec=self.sec())          # PWN_EBUSY
        self.emit("overlap", on=self.flip())                                   # PWN_EBUSY
        self.random_family_op()                                                # behind the frame in flight
        self.drain()
        self.emit("overlap", on=self.flip())

    def block_outside(self):
        """viewports that cover the frame, then the layout that leaves its bottom right uncovered"""
        if self.level is None:
            self.set_level("pwnfps_level")
        if self.W % 4:
            self.set_blur(0)
        self.family("d", layout=int((1, 3)[self.rng.integers(2)]))
        if self.flip():
            self.family("abcefgij"[int(self.rng.integers(8))])
        self.family("d", layout=2)

    def block_refusals(self):
        """w % 4 != 0: every family that blurs is refused while the passes are on, and runs again when they are off"""
        if self.level is None:
            self.set_level("synth64")
        if self.nslots == 0:
            self.config()
        self.drain()
        self.set_blur(int(self.rng.integers(1, 4)))
        for f in self.rng.permutation(list(BLURRED + "i")):
            self.family(str(f), slot=(0 if f == "h" else None))
        self.set_blur(0)
        for f in self.rng.permutation(list(BLURRED + "i")):
            self.family(str(f), slot=(0 if f == "h" else None))
        self.drain()

    def block_tour(self):
        """this sequence's stretch of the tour of all ordered pairs: family operations with nothing between them"""
        t = tour()
        per = -(-(len(t) - 1) // self.of)
        part = t[self.index * per: self.index * per + per + 1]
        if self.level is None:
            self.set_level("synth64")
        for f in part:
            self.family(f)


def generate(seed, n_ops, profile):
    """the operation records of sequence `seed`: its blocks in a random order, random operations between them, n_ops at least
    (the blocks are never cut short: n_ops is where the random filling stops)"""
    index = [s for s, _, _ in SEEDS].index(seed) if seed in [s for s, _, _ in SEEDS] else seed % len(SEEDS)
    g = _Gen(seed, profile, index, len(SEEDS))
    nine = LAUNCHING
    combos = [(f, p) for p in range(4) for f in BLURRED]
    even = [s for s, prof, _ in SEEDS if PROFILES[prof]["w"] % 4 == 0]
    mine = []
    if PROFILES[profile]["w"] % 4 == 0:
        k = even.index(seed) if seed in even else seed % len(even)
        mine = [combos[(3 * k + j) % len(combos)] for j in range(3)]
    # before a level: PWN_ENOLEVEL, whatever the family
    g.family("abcdefgi"[index % 8])
    if g.W % 4 == 0 or g.rng.integers(2):
        g.family("h")
        g.family("h", slot=0)
    g.set_level(LEVELS[int(g.rng.integers(3))])
    g.set_objects("own")
    blocks = [g.block_persist, g.block_restart, g.block_errors, g.block_outside, g.block_tour,
              lambda: g.block_form(nine[index % 9], (nine[(index + 1) % 9], nine[(index + 2) % 9]), nine[(index + 4) % 9])]
    if mine:
        blocks.append(lambda: g.block_blur(mine))
    else:
        blocks.append(g.block_refusals)
    forced = 0
    for b in g.rng.permutation(len(blocks)):
        before = len(g.ops)
        blocks[int(b)]()
        forced += len(g.ops) - before
        for _ in range(int(g.rng.integers(0, 3))):
            g.random_op()
    while len(g.ops) < n_ops:
        g.random_op()
    g.drain()
    if g.nslots:
        g.emit("config", n=0, sbuf=False, zbuf=False, surface=0)
    return g.ops
