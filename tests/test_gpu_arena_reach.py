"""The arena loop with something that flies, once, on one stream with the first host wait at the end: four players step, each fires
along its crosshair, and for T ticks every projectile moves its reach (pwn_trace_reach_hide_device, hide = its shooter's body); bodies
and live projectiles are written as spheres, the table is built on the device and everyone observes without its own body.  The same T
ticks with the blocking pwn_trace_reach and numpy glue, on contexts that hold each shooter's table without its body, give the same
records bit for bit at every tick.
"The final views differ from views without the projectile spheres" is read as: the views of the LAST TICK IN WHICH SOMETHING FLEW.  Every
projectile has to end within the T ticks, and only live projectiles are written as spheres, so the views of tick T - 1 hold none by
construction; the views of every tick are kept, and the last one with a live projectile is held against the bodies alone."""
import numpy as np
import pytest

from conftest import level_path

pytestmark = pytest.mark.gpu

W, H, N, T = 40, 26, 4, 24
REACH = 0.35
LEVEL = "pwnfps_level"
FREE, WALL, SPHERE = 3, 1, 2
# (from the spawn cell's centre the crosshair rays at these yaws cross one portal each and end on a wall 3.9 to 5.9 away: the oracle's
# chains, tests/hit_chain.py)
YAWS = (0.491, 2.847, 3.632, 5.89)
DEAD = (1.5, -50.0, 1.5)          # where the sphere of a projectile that is not flying is kept: below every room, in no cell's list


def _next_rays_numpy(rays, hits, alive):
    """the glue of a tick, in numpy: where the record is FREE the next ray starts at x y z and flies along dx dy dz"""
    free = (hits["kind"] == FREE) & alive
    nxt = rays.copy()
    for k, (p, d) in enumerate(zip(("x", "y", "z"), ("dx", "dy", "dz"))):
        nxt[:, k] = np.where(free, hits[p], rays[:, k])
        nxt[:, 4 + k] = np.where(free, hits[d], rays[:, 4 + k])
    return nxt, free


def test_projectiles_fly_through_the_arena():
    import torch
    import pwnfps_amd
    from pwnfps_amd import _lib
    dev = torch.device("cuda", 0)
    r = pwnfps_amd.Renderer(W, H)
    r.level_load(level_path(LEVEL))
    _, _, spawn = r.get_level()
    cams0 = np.stack([pwnfps_amd.spawn_camera(spawn, ang_y=a).reshape(16) for a in YAWS]).astype(np.float32)
    grav0 = np.zeros((N, 4), np.float32)
    # player 0 stands and aims at its portal; the others walk on along their aim, out of one another's bodies
    keys0 = np.array([0, _lib.PWN_MOVE_FORWARD, _lib.PWN_MOVE_FORWARD, _lib.PWN_MOVE_FORWARD], np.uint8)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        cams = torch.from_numpy(cams0.copy()).to(dev)
        grav = torch.from_numpy(grav0).to(dev)
        keys = torch.from_numpy(keys0).to(dev)
        secs = torch.zeros(N, dtype=torch.float32, device=dev)
        hide = torch.arange(N, dtype=torch.int32, device=dev)
        reach = torch.full((N,), REACH, dtype=torch.float32, device=dev)
        dead = torch.tensor(DEAD, dtype=torch.float32, device=dev)
        hits = torch.zeros((N, 12), dtype=torch.int32, device=dev)
        rec_all = torch.zeros((T, N, 12), dtype=torch.int32, device=dev)
        rays_all = torch.zeros((T, N, 8), dtype=torch.float32, device=dev)
        sph_all = torch.zeros((T, 2 * N, 8), dtype=torch.float32, device=dev)
        sb_all = torch.zeros((T, N, H, W), dtype=torch.int32, device=dev)
        z_all = torch.zeros((T, N, H, W), dtype=torch.float32, device=dev)
        work = torch.zeros((N, H, W), dtype=torch.int32, device=dev)
        # 1. the players step
        r.players_step_device(keys, cams, grav, tdiff=1 / 30, ticks=4)
        # 2. each fires along its crosshair
        xy = torch.tensor([[W // 2, H // 2]], dtype=torch.int32, device=dev)
        rays, _ = r.pixel_rays_device(cams, xy, seeds=False)
        rays = rays.view(N, 8)
        # bodies 0 .. N-1 (r 0.3 where the cameras are), projectiles N .. 2N-1 (r 0.05, not flying yet)
        sph = torch.zeros((2 * N, 8), dtype=torch.float32, device=dev)
        sph[:N, 0], sph[N:, 0], sph[:, 1] = 0.3, 0.05, 0.5
        sph[:N, 2:5] = cams.view(N, 16)[:, 12:15]
        sph[N:, 2:5] = dead
        sph[:, 5:8] = torch.tensor([[1.0, 0.2, 0.2], [0.2, 1.0, 0.2], [0.2, 0.2, 1.0], [1.0, 1.0, 0.2]] * 2, device=dev)
        r.upload_spheres_device(sph, 1024)
        alive = torch.ones(N, dtype=torch.bool, device=dev)
        # 3. T ticks
        for t in range(T):
            rays_all[t].copy_(rays)
            sph_all[t].copy_(sph)
            r.trace_reach_device(rays, reach, hits, hide=hide)
            rec_all[t].copy_(hits)
            # the next tick's rays, the two lines: from the records' x y z / dx dy dz where the kind is FREE
            free = (hits[:, 0] == FREE) & alive
            hf = hits.view(torch.float32)
            rays = torch.cat([torch.where(free[:, None], hf[:, 5:8], rays[:, 0:3]), rays[:, 3:4],
                              torch.where(free[:, None], hf[:, 8:11], rays[:, 4:7]), rays[:, 7:8]], 1).contiguous()
            alive = free
            sph[N:, 2:5] = torch.where(alive[:, None], rays[:, 0:3], dead)
            r.upload_spheres_device(sph, 1024)
            r.trace_views_device(cams, secs, sb_all[t], z_all[t], work=work, hide=hide)
        # (the first host wait)
        h_rec = rec_all.cpu().numpy().view(pwnfps_amd.HIT_DTYPE).reshape(T, N)
        h_rays, h_sph, h_sb, h_cams = rays_all.cpu().numpy(), sph_all.cpu().numpy(), sb_all.cpu().numpy(), cams.cpu().numpy()
    s.synchronize()
    assert r.spheres_device_state()["reason"] == 0

    # what became of the projectiles
    alive_np = np.ones(N, bool)
    portals = np.zeros(N, np.int64)
    ended = [None] * N
    flying = np.zeros((T, N), bool)
    for t in range(T):
        for i in np.flatnonzero(alive_np):
            portals[i] += h_rec[t, i]["portals"]
            if h_rec[t, i]["kind"] != FREE:
                ended[i] = (t, int(h_rec[t, i]["kind"]), int(h_rec[t, i]["object"]))
        alive_np &= h_rec[t]["kind"] == FREE
        flying[t] = alive_np
    print("projectiles ended (tick, kind, object):", ended, "portals crossed:", portals.tolist())
    assert all(e is not None and e[1] in (WALL, SPHERE) for e in ended), ended
    assert all(not (e[1] == SPHERE and e[2] == i) for i, e in enumerate(ended)), ended
    assert (portals > 0).any(), portals
    assert flying.sum() >= 2 * N, flying.sum(0)          # (ticks flown, over all projectiles)

    # 4. the same ticks with the blocking call and numpy glue, per shooter on the table without its body
    refs = []
    for i in range(N):
        ref = pwnfps_amd.Renderer(8, 8)
        ref.level_load(level_path(LEVEL))
        refs.append(ref)
    rays_np, alive_np = h_rays[0].copy(), np.ones(N, bool)
    sph_np = h_sph[0].copy()
    for t in range(T):
        assert rays_np.tobytes() == h_rays[t].tobytes() and sph_np.tobytes() == h_sph[t].tobytes(), t
        table = np.ascontiguousarray(sph_np).view(pwnfps_amd.SPHERE_DTYPE).reshape(2 * N)
        want = np.zeros(N, pwnfps_amd.HIT_DTYPE)
        for i in range(N):
            refs[i].set_objects(np.delete(table, i))
            w = refs[i].trace_reach(rays_np[i:i + 1], np.array([REACH], np.float32))[0]
            if w["kind"] == SPHERE and w["object"] >= i:
                w["object"] += 1                           # (numbered by the full table)
            want[i] = w
        assert want.tobytes() == h_rec[t].tobytes(), (t, want.tolist(), h_rec[t].tolist())
        rays_np, alive_np = _next_rays_numpy(rays_np, want, alive_np)
        sph_np[N:, 2:5] = np.where(alive_np[:, None], rays_np[:, 0:3], np.array(DEAD, np.float32))
    for ref in refs:
        ref.close()

    # the views of the last tick in which something flew show it: the same views from the bodies alone differ
    t_last = int(np.flatnonzero(flying.any(1))[-1])
    with torch.cuda.stream(s):
        bodies = torch.from_numpy(h_sph[t_last].copy()).to(dev)
        bodies[N:, 2:5] = dead
        r.upload_spheres_device(bodies, 1024)
        sb2 = torch.zeros((N, H, W), dtype=torch.int32, device=dev)
        z2 = torch.zeros((N, H, W), dtype=torch.float32, device=dev)
        r.trace_views_device(cams, secs, sb2, z2, work=work, hide=hide)
        without = sb2.cpu().numpy()
    s.synchronize()
    r.close()
    shown = [int((h_sb[t_last, i] != without[i]).sum()) for i in range(N)]
    print("tick %d: pixels in which a projectile showed, per player:" % t_last, shown)
    assert sum(shown) > 0, shown
    assert not np.array_equal(h_cams, cams0)          # (the players moved)
