// The launch plan (pwnfps_amd/csrc/launch_plan.h) over a sweep of shapes, printed for tests/test_launch_plan.py: plain g++, no HIP.
//   P <the shape's fields> <rc> <the plan's fields>     one line per shape
//   M d magic shift                                      pwn_unit_div_magic for d = 1 .. 4100
#include <stdio.h>
#include "launch_plan.h"

int main(void)
{
	const int widths[] = { 4, 16, 20, 32, 40, 48, 56, 496, 512, 528, 2080, 3840, 32768 };
	const int rows[] = { 1, 4, 5, 9, 36, 160, 2160, 4096 };
	const int grids[] = { 1, 4, 20, 1280 };
	// what is traced: the frame, 1 and 3 views, 65 rays, 3 viewports (their units: a third of the frame's and seven)
	const struct { int kind; uint32_t n; } what[] = { { PWN_LAUNCH_FRAME, 0 }, { PWN_LAUNCH_VIEWS, 1 }, { PWN_LAUNCH_VIEWS, 3 }, { PWN_LAUNCH_RAYS, 65 }, { PWN_LAUNCH_VIEWPORTS, 3 } };
	for(int w : widths) for(int r : rows) for(int g : grids) for(int rv = 0; rv < 3; rv++) for(int tp = 0; tp <= 2; tp++)
	for(int refill = 0; refill <= 1; refill++) for(int cost = 0; cost <= 1; cost++) for(const auto &k : what)
	{
		pwn_launch_shape S = {};
		S.w = w; S.y0 = 4 * (r % 3); S.y1 = S.y0 + r; S.tile_w = 16; S.tile_h = 4;
		S.kind = k.kind; S.n = k.n;
		S.vp_units = k.kind == PWN_LAUNCH_VIEWPORTS ? (uint32_t)(((w + 15) / 16) * ((r + 3) / 4) / 3 + 7) : 0u;
		S.resident = g; S.reserve = rv == 0 ? 0 : rv == 1 ? 4 : g / 2 + 1;
		S.refill = refill != 0; S.want_cost = cost != 0; S.tile_pairs = tp;
		pwn_launch_plan p;
		const int rc = pwn_launch_plan_make(S, &p);
		printf("P %d %d %d %d %u %u %d %d %d %d %d %d %d %d %u %d %u %d %u %d %d %u %d %d %d %u %u\n", S.w, S.y0, S.y1, S.kind, S.n, S.vp_units, S.resident, S.reserve,
			(int)S.refill, (int)S.want_cost, S.tile_pairs, rc, p.tiles_x, p.tiles_total, p.ux_magic, p.ux_shift, p.views_magic, p.views_shift, p.vp_step0,
			p.tile_pairs, p.pair_single_rows, p.tx_magic, p.tx_shift, p.items, p.grid, p.cost_mul, p.cost_div);
	}
	for(uint32_t d = 1; d <= 4100; d++)
	{
		uint32_t m; int s;
		pwn_unit_div_magic(d, &m, &s);
		printf("M %u %u %d\n", d, m, s);
	}
	return 0;
}
