"""The arena loop once at the agents' own resolutions, on one stream with no host wait in between: four players step on the device,
every player's body is a sphere written where its camera is, the table is built on the device, and ONE atlas of four views of
different sizes is rendered with every view hiding its own body (pwn_trace_viewports_hide_device with hide = 0 .. 3) -- then the
label atlas of the same views (pwn_trace_viewport_hits_hide_device).  Each rectangle equals the blocking call's on a context of
w_i x h_i that holds the other three spheres only: the wrong body hidden, or a hide word that went to the wrong rectangle (the records
are in another order than the rectangles), fails it."""
import numpy as np
import pytest

from conftest import level_path

import hide_vp_scenes as V

pytestmark = pytest.mark.gpu

N = 4
LEVEL = "pwnfps_level"
# a frame of 100 x 40, usable with blur; units 21, 12, 18, 4: the records' order is 3, 1, 2, 0
FW, FH = 100, 40
RECTS = [(0, 0, 40, 26), (40, 0, 44, 14), (0, 26, 96, 12), (84, 0, 16, 13)]


def test_players_do_not_see_their_own_body_in_the_atlas():
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    r = pwnfps_amd.Renderer(V.CW, V.CH)
    r.level_load(level_path(LEVEL))
    r.set_blur_passes(1)
    _, _, spawn = r.get_level()
    cams0, grav0, _ = pwnfps_amd.players_spawn(spawn, N)
    keys0 = np.array([_lib.PWN_MOVE_FORWARD, _lib.PWN_MOVE_FORWARD | _lib.PWN_MOVE_TURN_LEFT, _lib.PWN_MOVE_LEFT | _lib.PWN_MOVE_TURN_RIGHT,
                      _lib.PWN_MOVE_BACK], np.uint8)
    secs0 = np.array([0.5, 1.5, 2.5, 3.5], np.float32)
    lay = r.viewports_layout(FW, FH, RECTS)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams = torch.from_numpy(cams0.copy()).to(dev)
        grav = torch.from_numpy(grav0.copy()).to(dev)
        keys = torch.from_numpy(keys0).to(dev)
        secs = torch.from_numpy(secs0).to(dev)
        planes = [torch.full((FH, FW), -1, dtype=torch.int32, device=dev) for _ in range(6)]
        zs = [torch.zeros((FH, FW), dtype=torch.float32, device=dev) for _ in range(2)]
        hide = torch.arange(N, dtype=torch.int32, device=dev)
        # 1. a few ticks
        r.players_step_device(keys, cams, grav, tdiff=1 / 30, ticks=6)
        # 2. sphere i = the body of player i: r 0.3 at camera i's position (r, refl, x, y, z, cb, cg, cr)
        sph = torch.zeros((N, 8), dtype=torch.float32, device=dev)
        sph[:, 0] = 0.3
        sph[:, 1] = 0.5
        sph[:, 2:5] = cams.view(N, 16)[:, 12:15]
        sph[:, 5:8] = torch.tensor([[1.0, 0.2, 0.2], [0.2, 1.0, 0.2], [0.2, 0.2, 1.0], [1.0, 1.0, 0.2]], device=dev)
        # 3. the table, 4. the atlas without every player's own body -- and, for the teeth, with it -- 5. the label atlas
        r.upload_spheres_device(sph, 1024)
        r.trace_viewports_device(lay, cams, secs, planes[0], zs[0], work=planes[1], hide=hide)
        r.trace_viewports_device(lay, cams, secs, planes[2], zs[1], work=planes[3])
        r.trace_viewport_hits_device(lay, cams, planes[4], hide=hide)
        r.trace_viewport_hits_device(lay, cams, planes[5])
        # (the first host wait)
        got, got_z = planes[0].cpu().numpy().view(np.uint32), zs[0].cpu().numpy().view(np.uint32)
        seen = planes[2].cpu().numpy().view(np.uint32)
        got_lb, seen_lb = planes[4].cpu().numpy().view(np.uint32), planes[5].cpu().numpy().view(np.uint32)
        h_cams, h_sph = cams.cpu().numpy(), sph.cpu().numpy()
    s.synchronize()
    st = r.spheres_device_state()
    assert st["in_force"] == 1 and st["n"] == N and st["reason"] == 0, st
    lay.free()
    r.close()
    assert not np.array_equal(h_cams, cams0.reshape(h_cams.shape))          # (the players moved)
    # the blocking reference: per player, a context of the view's size with the other three spheres
    bodies = np.ascontiguousarray(h_sph).view(pwnfps_amd.SPHERE_DTYPE).reshape(N)
    for i, (x, y, w, h) in enumerate(RECTS):
        ref = pwnfps_amd.Renderer(w, h)
        ref.level_load(level_path(LEVEL))
        ref.set_blur_passes(1)
        ref.set_objects(np.delete(bodies, i))
        want, want_z = ref.trace_views(h_cams[i:i + 1], secs0[i:i + 1])
        want_lb, _, _ = ref.trace_view_hits(h_cams[i:i + 1], want_cell=False, want_dist=False)
        ref.close()
        bad = int((V.rect(got, i, RECTS) != want[0]).sum())
        assert bad == 0, (i, bad)
        assert (V.rect(got_z, i, RECTS) == np.ascontiguousarray(want_z[0]).view(np.uint32)).all(), i
        assert (V.rect(got_lb, i, RECTS) == V.relabel(np.ascontiguousarray(want_lb[0]).view(np.uint32), i)).all(), i
    # nothing outside the rectangles
    m = np.zeros((FH, FW), bool)
    for x, y, w, h in RECTS:
        m[y:y + h, x:x + w] = True
    assert (got[~m] == 0xffffffff).all() and (got_lb[~m] == 0xffffffff).all() and (got_z[~m] == 0).all()
    # (a camera exactly at its body's centre never meets the body on the primary segment, tests/test_gpu_arena_hide.py: what hiding
    # takes out of these views is the body in the mirrors.  Player 0's view is that test's, where its body showed; the smaller views
    # are printed.)
    own = [int((V.rect(got, i, RECTS) != V.rect(seen, i, RECTS)).sum()) for i in range(N)]
    own_lb = [int((V.rect(got_lb, i, RECTS) != V.rect(seen_lb, i, RECTS)).sum()) for i in range(N)]
    print("pixels in which a player's own body showed:", own, "labels:", own_lb)
    assert own[0] > 0, own
