"""Every hard scene in one corpus, for tests that run them through the library's variants and paths.

The hard scenes are the ones that found bugs here: the edge scenes (tests/edge_scenes.py), the three non-finite
lattice scenes (tests/golden/nonfinite/, -inf depths and NaN colour) and the five far starts
(tests/golden/far_starts.npz).  The expected frame always comes from the oracle (tests/oracle.py); for the
non-finite scenes the oracle is first pinned to the stored rendering of the IEEE build of the reference.
"""
import glob
import os
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NONFINITE = sorted(glob.glob(os.path.join(GOLD, "nonfinite", "*.npz")))
FAR_STARTS = os.path.join(GOLD, "far_starts.npz")
DEFAULT_LEVEL = os.path.join(GOLD, "levels", "pwnfps_level.txt")

# level: a path to a level file, or the level's text.  blur_ok: the blur may be on (w % 4 == 0, screen.h:88).
# pin: for the non-finite scenes, the stored frame of the IEEE build ({"blur", "sb", "z"}), else None.
HardScene = namedtuple("HardScene", "name kind level spheres cam sec w h blur_ok pin")


def _scene(name, kind, level, spheres, cam, sec, w, h, pin=None):
    return HardScene(name, kind, level, spheres, np.ascontiguousarray(cam, np.float32).reshape(4, 4), float(sec),
                     int(w), int(h), int(w) % 4 == 0, pin)


def scenes(sphere_dtype):
    """every hard scene, in a fixed order: edge scenes, non-finite scenes, far starts"""
    import edge_scenes
    out = []
    for sc in edge_scenes.scenes(sphere_dtype):
        out.append(_scene(sc.name, "edge", DEFAULT_LEVEL if sc.text is None else sc.text, sc.spheres, sc.cam,
                          sc.sec, sc.w, sc.h))
    for path in NONFINITE:
        d = np.load(path)
        pin = {"blur": int(d["blur"]), "sb": d["ref_nf"], "z": d["ref_nf_z"]}
        out.append(_scene("nonfinite_" + os.path.basename(path)[:-4], "nonfinite", str(d["text"]),
                          np.ascontiguousarray(d["sph"], sphere_dtype), d["cam"], d["sec"], d["w"], d["h"], pin))
    k = np.load(FAR_STARTS)
    for i, name in enumerate(k["names"]):
        w, h = (int(v) for v in k["wh_%d" % i])
        out.append(_scene("far_" + str(name), "far", str(k["text_%d" % i]),
                          np.ascontiguousarray(k["sph_%d" % i], sphere_dtype), k["cam_%d" % i], k["sec_%d" % i], w, h))
    return out


def is_path(level):
    return "\n" not in level and level.endswith(".txt")


def load_oracle(O, sc):
    (O.load_level if is_path(sc.level) else O.load_level_text)(sc.level)
    O.set_spheres(sc.spheres)


def load_renderer(r, sc):
    (r.level_load if is_path(sc.level) else r.level_load_text)(sc.level)
    r.set_objects(sc.spheres)


def oracle(oracle_mod, sc):
    """an Oracle loaded with the scene; for a non-finite scene, asserts first that it renders the stored frame"""
    O = oracle_mod.Oracle()
    load_oracle(O, sc)
    if sc.pin is not None:
        sb, z = O.render(sc.w, sc.h, sc.cam, sec=sc.sec, blur=sc.pin["blur"])
        assert (~np.isfinite(z)).any(), sc.name
        assert (sb == sc.pin["sb"]).all(), sc.name
        assert (bits(z) == bits(sc.pin["z"])).all(), sc.name
    return O


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stats5(st):
    """(rays, steps, portals, sphere_tests, exhausted) of an oracle Stats or a Renderer.stats() dict"""
    if isinstance(st, dict):
        return (st["rays"], st["steps"], st["portals"], st["sphere_tests"], st["exhausted"])
    return (st.rays, st.steps, st.portals, st.sphere_tests, st.exhausted)


class Plane:
    """The oracle's side of one persistent depth plane (the blocking call's, or one view slot's): depth of pixels
    whose primary ray hits nothing keeps its previous value (trace.h:677), so a frame is judged by the oracle
    carrying the depth this plane's earlier frames left."""

    def __init__(self, O, w, h):
        self.O, self.w, self.h = O, w, h
        self.z = np.zeros((h, w), np.float32)

    def frame(self, cam, sec, blur):
        """(colour, depth, oracle stats) of the next frame on this plane"""
        sb, z, st = self.O.trace_rows(self.w, self.h, 0, self.h, cam, sec=np.float32(sec), zb=self.z.copy())
        self.z = z
        return (self.O.blur_rows(0, self.h, sb, z) if blur else sb), z, st


def fresh(O, w, h, cam, sec, blur):
    """a frame on a plane that starts from zero depth"""
    return Plane(O, w, h).frame(cam, sec, blur)
