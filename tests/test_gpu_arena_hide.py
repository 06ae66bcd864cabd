"""The arena loop once, on one stream with no host wait in between: players step on the device, every player's body is a sphere
written where its camera is, the table is built on the device, and every player observes the arena WITHOUT its own body
(pwn_trace_views_hide_device with hide = 0 .. n-1).  Each view equals the blocking call's on a context that holds the other three
spheres only: the wrong body hidden, or none of the others shown, fails it."""
import numpy as np
import pytest

from conftest import level_path

pytestmark = pytest.mark.gpu

W, H, N = 40, 26, 4
LEVEL = "pwnfps_level"


def test_players_do_not_see_their_own_body():
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    r = pwnfps_amd.Renderer(W, H)
    r.level_load(level_path(LEVEL))
    _, _, spawn = r.get_level()
    cams0, grav0, _ = pwnfps_amd.players_spawn(spawn, N)
    keys0 = np.array([_lib.PWN_MOVE_FORWARD, _lib.PWN_MOVE_FORWARD | _lib.PWN_MOVE_TURN_LEFT, _lib.PWN_MOVE_LEFT | _lib.PWN_MOVE_TURN_RIGHT,
                      _lib.PWN_MOVE_BACK], np.uint8)
    secs0 = np.array([0.5, 1.5, 2.5, 3.5], np.float32)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams = torch.from_numpy(cams0.copy()).to(dev)
        grav = torch.from_numpy(grav0.copy()).to(dev)
        keys = torch.from_numpy(keys0).to(dev)
        secs = torch.from_numpy(secs0).to(dev)
        planes = [torch.full((N, H, W), -1, dtype=torch.int32, device=dev) for _ in range(4)]
        zs = [torch.zeros((N, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        hide = torch.arange(N, dtype=torch.int32, device=dev)
        # 1. a few ticks
        r.players_step_device(keys, cams, grav, tdiff=1 / 30, ticks=6)
        # 2. sphere i = the body of player i: r 0.3 at camera i's position (r, refl, x, y, z, cb, cg, cr)
        sph = torch.zeros((N, 8), dtype=torch.float32, device=dev)
        sph[:, 0] = 0.3
        sph[:, 1] = 0.5
        sph[:, 2:5] = cams.view(N, 16)[:, 12:15]
        sph[:, 5:8] = torch.tensor([[1.0, 0.2, 0.2], [0.2, 1.0, 0.2], [0.2, 0.2, 1.0], [1.0, 1.0, 0.2]], device=dev)
        # 3. the table, 4. every player's view without its own body -- and, for the teeth, with it
        r.upload_spheres_device(sph, 1024)
        r.trace_views_device(cams, secs, planes[0], zs[0], work=planes[1], hide=hide)
        r.trace_views_device(cams, secs, planes[2], zs[1], work=planes[3])
        # (the first host wait)
        got, got_z = planes[0].cpu().numpy().view(np.uint32), zs[0].cpu().numpy().view(np.uint32)
        seen = planes[2].cpu().numpy().view(np.uint32)
        h_cams, h_sph = cams.cpu().numpy(), sph.cpu().numpy()
    s.synchronize()
    st = r.spheres_device_state()
    assert st["in_force"] == 1 and st["n"] == N and st["reason"] == 0, st
    r.close()
    assert not np.array_equal(h_cams, cams0.reshape(h_cams.shape))          # (the players moved)
    # 5. the blocking reference: per player, a context with the other three spheres
    bodies = np.ascontiguousarray(h_sph).view(pwnfps_amd.SPHERE_DTYPE).reshape(N)
    for i in range(N):
        ref = pwnfps_amd.Renderer(W, H)
        ref.level_load(level_path(LEVEL))
        ref.set_objects(np.delete(bodies, i))
        want, want_z = ref.trace_views(h_cams[i:i + 1], secs0[i:i + 1])
        ref.close()
        bad = int((got[i] != want[0]).sum())
        assert bad == 0, (i, bad)
        assert (got_z[i] == np.ascontiguousarray(want_z[0]).view(np.uint32)).all(), i
    # (A camera exactly at its body's centre never meets the body on the primary segment -- the sphere test wants the centre in front
    # of the ray -- so what hiding takes out of THESE views is the body in the mirrors: walls, floor, the other bodies.  The views test
    # has the camera off the centre; here every player's own body shows in a few dozen pixels.  A hide word that named the wrong body would
    # fail the comparison above: the other bodies are in sight.)
    own = [int((got[i] != seen[i]).sum()) for i in range(N)]
    print("pixels in which a player's own body showed:", own)
    assert all(v > 0 for v in own), own
