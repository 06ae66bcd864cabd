"""The reader of tests/hit_chain.py, pinned on the oracle alone (no GPU): on the three level.txt frames its distances are the
depth plane's bits and its step counts pwno_step_map's segment-0 slots, and the frames hold what the GPU tests need them to hold."""
import ctypes as C

import numpy as np

import hit_chain as HC

SENTINEL = np.uint32(0x7fc12345)          # a NaN pattern no computation makes


def test_reader_is_the_oracle_on_the_level_frames(oracle_lib):
    O, sph, cams, refs = HC.level_frames(oracle_lib)
    w, h = HC.LEVEL_W, HC.LEVEL_H
    O.L.pwno_step_map.argtypes = [C.c_void_p]
    sphere_hits = portals = tall_walls = 0
    seen = set()
    two = False
    for cam, ref in zip(cams, refs):
        smap = np.zeros((h, w, 3), np.uint16)
        zb = np.full((h, w), SENTINEL, np.uint32).view(np.float32)
        O.L.pwno_step_map(smap.ctypes.data)
        try:
            _, zb, st = O.trace_rows(w, h, 0, h, cam, threads=1, zb=zb)
        finally:
            O.L.pwno_step_map(None)
        want = ref.want
        none = want["kind"] == HC.NONE
        z = HC._bits(zb).ravel()
        assert (z[none] == SENTINEL).all() and not (z[~none] == SENTINEL).any()
        assert (HC._bits(want["dist"])[~none] == z[~none]).all()
        assert (ref.steps == smap[:, :, 0].ravel()).all()
        assert int(none.sum()) <= st.exhausted
        # a NONE record is all zero but face and object
        for name in HC.HIT_DTYPE.names:
            assert (want[name][none] == (-1 if name in ("face", "object") else 0)).all(), name
        sph_hit = want["kind"] == HC.SPHERE
        assert (want["face"][sph_hit] == -1).all() and (want["object"][~sph_hit] == -1).all()
        assert ((want["object"][sph_hit] >= 0) & (want["object"][sph_hit] < len(sph))).all()
        wall = want["kind"] == HC.WALL
        assert ((want["face"][wall] >= 0) & (want["face"][wall] <= 5)).all()
        sphere_hits += int(sph_hit.sum())
        seen |= set(want["object"][sph_hit].tolist())
        portals += int(want["portals"].sum())
        two |= bool((want["portals"] >= 2).any())
        tall_walls += int((wall & (want["face"] <= HC.FZN) & np.isin(ref.last_ch, (35, 38))).sum())
    assert sphere_hits >= 250 and len(seen) >= 8, (sphere_hits, sorted(seen))
    assert portals >= 200 and two, portals
    assert tall_walls >= 300, tall_walls


def test_trick_camera_gives_the_pixel_record(oracle_lib):
    """a pixel's ray record (pwn_pixel_rays) through the 1 x 1 trick camera reads as the pixel itself does"""
    import pwnfps_amd
    O, sph, cams, refs = HC.level_frames(oracle_lib)
    rd = HC.Reader(O)
    rng = np.random.default_rng(77)
    xy = np.stack([rng.integers(0, HC.LEVEL_W, 48), rng.integers(0, HC.LEVEL_H, 48)], 1).astype(np.int32)
    for cam, ref in zip(cams, refs):
        rays, _, _ = pwnfps_amd.pixel_rays(HC.LEVEL_W, HC.LEVEL_H, cam, xy)
        keep = ~(np.signbit(rays[:, 4:]) & (rays[:, 4:] == 0)).any(1)       # (the trick gives +0 where the frame's ray has -0)
        assert keep.sum() >= 24
        got = rd.rays(rays[keep])
        idx = (xy[keep, 1] * HC.LEVEL_W + xy[keep, 0])
        assert len(HC.mismatches(got.want, ref.want[idx], ref.cmp_dy[idx])) == 0
        assert (got.steps == ref.steps[idx]).all()
