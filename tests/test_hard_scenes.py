"""The hard-scene corpus (tests/hard_scenes.py) on the oracle alone: what the GPU variant tests
(tests/test_gpu_variants.py) take as their judge."""
import numpy as np

import hard_scenes as HS


def test_corpus_holds_every_hard_scene(oracle_lib):
    import edge_scenes
    sc = HS.scenes(oracle_lib.SPHERE_DTYPE)
    kinds = [s.kind for s in sc]
    assert kinds.count("edge") == len(edge_scenes.scenes(oracle_lib.SPHERE_DTYPE))
    assert kinds.count("nonfinite") == 3 and kinds.count("far") == 5
    assert len({s.name for s in sc}) == len(sc)
    for s in sc:
        assert s.blur_ok == (s.w % 4 == 0) and s.cam.shape == (4, 4) and s.cam.dtype == np.float32
    # the ragged widths are in: some scenes can only run without the blur
    assert any(not s.blur_ok for s in sc)


def test_nonfinite_scenes_pin_the_oracle(oracle_lib):
    for s in HS.scenes(oracle_lib.SPHERE_DTYPE):
        if s.kind == "nonfinite":
            HS.oracle(oracle_lib, s)          # asserts the stored IEEE-build frame and depth


def test_the_carried_plane_starts_as_a_fresh_frame(oracle_lib):
    """Plane (trace_rows + blur_rows from zero depth) is O.render(stats=True): frame, depth and counters"""
    for s in HS.scenes(oracle_lib.SPHERE_DTYPE):
        O = HS.oracle(oracle_lib, s)
        blur = 1 if s.blur_ok else 0
        a, za, sa = HS.Plane(O, s.w, s.h).frame(s.cam, s.sec, blur)
        b, zb, sb = O.render(s.w, s.h, s.cam, sec=s.sec, blur=blur, stats=True)
        assert (a == b).all() and (HS.bits(za) == HS.bits(zb)).all(), s.name
        assert HS.stats5(sa) == HS.stats5(sb), s.name


def test_a_carried_plane_differs_where_rays_exhaust(oracle_lib):
    """The carried depth is what a reused context must reproduce: on the scenes whose rays exhaust, a second camera
    on the same plane leaves depth that a fresh frame does not have."""
    seen = 0
    for s in HS.scenes(oracle_lib.SPHERE_DTYPE):
        O = HS.oracle(oracle_lib, s)
        p = HS.Plane(O, s.w, s.h)
        _, _, st = p.frame(s.cam, s.sec, 0)
        if st.exhausted == 0:
            continue
        seen += 1
        z0 = p.z.copy()
        _, z1, _ = p.frame(s.cam, s.sec + 0.5, 0)
        _, zf, _ = HS.fresh(O, s.w, s.h, s.cam, s.sec + 0.5, 0)
        ex = HS.bits(zf) == 0
        assert (HS.bits(z1)[ex] == HS.bits(z0)[ex]).all(), s.name
    assert seen > 0
