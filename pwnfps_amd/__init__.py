"""pwnfps_amd -- MI355X-native implementation of pwnfps's portal ray-march
render path (trace.h / screen.h of fanzyflani/pwnfps) behind a C ABI.

The compute lives in libpwnhip.so (hand-written HIP for gfx950, see csrc/);
this package is the thin host mirror used by bench.py and the tests."""
from .render import (Renderer, PwnError, SPHERE_DTYPE, PORTAL_DTYPE, HIT_DTYPE,  # noqa: F401
                     mat4_iden, mat4_roty, mat4_rotx, spawn_camera, pixel_rays, unit_order_xy, sphere_tables_plan, sphere_bounds_plan,
                     viewports_plan, ViewportsLayout, pack_labels, unpack_labels, players_spawn)
from ._lib import (PWN_MOVE_TURN_LEFT, PWN_MOVE_TURN_RIGHT, PWN_MOVE_TURN_UP, PWN_MOVE_TURN_DOWN,  # noqa: F401
                   PWN_MOVE_FORWARD, PWN_MOVE_BACK, PWN_MOVE_LEFT, PWN_MOVE_RIGHT, PWN_PLAYERS_MAX, PWN_TICKS_MAX,
                   PWN_PIXELS_SHARED, PWN_PIXEL_WORK_BYTES)
