// launch_plan.h -- the geometry of a trace launch as pure integer arithmetic: what is traced and how many workgroups are
// resident in, what the kernel is told about its units and how large its grid is out.  The trace kernel relies on these numbers
// word for word (trace_kernel.hip recomputes the item count from them), so they are made in one function that needs neither a
// context nor a device (pwn_launch.cpp pwn_i_launch_trace calls it; tests/test_launch_plan.py holds it to the kernel's own
// arithmetic).  Host code only: no HIP, no pwn_ctx, and not for the .hip files.
#pragma once
#include <stdint.h>
#include "trace_variants.h"      // PWN_KM_*

// The trace kernel turns a unit number into (row of units, unit in the row): a division by the units per row, which
// is the same number for every unit of a launch.  For d >= 2 and s the largest shift with 2^s < d, M = ceil(2^(32+s) / d)
// fits 32 bits, and with 2^(32+s) = M d - e, 0 <= e < d: n M / 2^(32+s) = n / d + n e / (d 2^(32+s)), whose floor is
// floor(n / d) while n e < 2^(32+s); e < d <= 2^(s+1), so every n < 2^31 divides exactly (a frame has at most 2^24 units).
// d == 1 (frames up to 16 pixels wide): shift -1, the kernel divides.
static inline void pwn_unit_div_magic(uint32_t d, uint32_t *magic, int *shift)
{
	*magic = 0u; *shift = -1;
	if(d < 2u) return;
	int s = 0;
	while((2u << s) < d) s++;                  // 2^s < d <= 2^(s+1)
	const unsigned long long two = 1ull << (32 + s);
	const unsigned long long M = (two + d - 1u) / d;        // < 2^32: 2^s < d
	*magic = (uint32_t)M; *shift = s;
}

// Workgroups of `bytes` of LDS each that a CU holds.  The API counts LDS as 160 KiB / bytes; a census
// (tools/ubench/lds_census.hip) shows one workgroup fewer resident at some sizes (5 x 32 KiB, 3 x 54000 B).  A persistent grid
// that is one workgroup per CU too large runs its surplus at the end at a fraction of the
// occupancy (+40 % frame time), so stay on the safe side: 2 KiB granules in 152 KiB.
static inline uint32_t pwn_lds_fit(uint32_t bytes) { return 155648u / ((bytes + 2047u) & ~2047u); }

enum { PWN_LAUNCH_FRAME = 0, PWN_LAUNCH_VIEWS, PWN_LAUNCH_RAYS, PWN_LAUNCH_VIEWPORTS };

// What a launch is (pwn_internal.h pwn_trace_launch), as far as the choice of the kernel goes: PWN_LAUNCH_* -- the frame, or the batch
// whose n is not 0 -- and, of that batch: label = its d_label / d_hits is given (first hits in the place of colours), hide = its
// `hide` is set / its d_hide is given, reach = its d_reach is given (rays alone have one).
struct pwn_launch_what { int kind; bool label, hide, reach; };
// ... as the trace kernel's MODE argument (PWN_KM_*).  The mode is only NAMED here: whether a kernel of that mode exists is for
// trace_variants.h to say, and for pwn_launch_trace to refuse (a reach without first hits or a hidden sphere in a frame has none).
// -1: no mode at all -- a frame has no planes of labels.
static inline int pwn_launch_mode(const pwn_launch_what &W)
{
	int mode;
	switch(W.kind)
	{
		case PWN_LAUNCH_RAYS: mode = W.label ? PWN_KM_HITS : PWN_KM_RAYS; break;
		case PWN_LAUNCH_VIEWS: mode = W.label ? PWN_KM_VIEW_HITS : PWN_KM_VIEWS; break;
		case PWN_LAUNCH_VIEWPORTS: mode = W.label ? PWN_KM_VIEWPORT_HITS : PWN_KM_VIEWPORTS; break;
		default: if(W.label) return -1; mode = PWN_KM_FRAME;
	}
	return mode | (W.hide ? PWN_KM_HIDE : 0) | (W.reach ? PWN_KM_REACH : 0);
}

struct pwn_launch_shape
{
	int w, y0, y1;                   // the frame's width and the rows [y0, y1) of it
	int tile_w, tile_h;              // a unit's pixels (pwn_trace_tile_w / _h: 16 x 4)
	int kind; uint32_t n;            // PWN_LAUNCH_*: the frame, or a batch of n views, n rays or n viewports ...
	uint32_t vp_units;               // ... whose units over all views are these (pwn_vps_launch.units)
	int resident;                    // workgroups resident at once: CUs x workgroups per CU, after the LDS rule and PWN_DBG_BLOCKS_PER_CU
	int reserve;                     // workgroups the grid leaves free: the greater of the row tiling's and the launch's room
	bool refill, want_cost;          // the refill scheduler's kernel; the launch writes its units' costs (an order, PWN_DBG_UNIT_COST)
	int tile_pairs;                  // PWN_TILE_PAIRS: 0 never, 1 where tickets would go out in pairs, 2 always
};

struct pwn_launch_plan
{
	int tiles_x, tiles_total;        // units per row; units of the launch
	uint32_t ux_magic; int ux_shift;             // unit / tiles_x
	uint32_t views_magic; int views_shift;       // unit / n, a batch of views
	uint32_t vp_step0;                           // where the kernel's search for a ticket's viewport starts
	int tile_pairs, pair_single_rows; uint32_t tx_magic; int tx_shift;      // pwn_trace_params of the same names
	int items;                       // what the queues hold: units, or single units and tiles
	int grid;                        // workgroups to launch
	uint32_t cost_mul, cost_div;     // resident grid / grid after the reserve (pwn_trace_launch)
};

// 0, or -1: no division constant for plan.tiles_x units per row (the plan is then filled up to there)
static inline int pwn_launch_plan_make(const pwn_launch_shape &S, pwn_launch_plan *out)
{
	pwn_launch_plan p = {};
	const bool batch = S.kind != PWN_LAUNCH_FRAME;
	p.tiles_x = (S.w + S.tile_w - 1) / S.tile_w;
	p.tiles_total = p.tiles_x * ((S.y1 - S.y0 + S.tile_h - 1) / S.tile_h);
	pwn_unit_div_magic((uint32_t)p.tiles_x, &p.ux_magic, &p.ux_shift);
	*out = p;
	// (the kernel takes unit / tiles_x = unit where there is no shift: true for one unit per row only)
	if(p.ux_shift < 0 && p.tiles_x != 1) return -1;
	// a batch of views: the frame's units once per view
	if(S.kind == PWN_LAUNCH_VIEWS)
	{
		pwn_unit_div_magic(S.n, &p.views_magic, &p.views_shift);
		p.tiles_total *= (int)S.n;
	}
	// views of their own sizes into this one frame: the units of all of them, found by the kernel from the records
	if(S.kind == PWN_LAUNCH_VIEWPORTS)
	{
		p.tiles_total = (int)S.vp_units;
		// (the kernel's search: strides from the largest power of two below n down to 1)
		p.vp_step0 = 0u;
		if(S.n > 1u) { p.vp_step0 = 1u; while(2u * p.vp_step0 <= S.n - 1u) p.vp_step0 *= 2u; }
	}
	// a batch of rays: 64 to a unit
	if(S.kind == PWN_LAUNCH_RAYS) p.tiles_total = (int)((S.n + 63u) / 64u);
	// persistent grid: as many workgroups as are resident at once, each striding over tiles
	int grid = S.resident;
	// row tiling over RCCL: a persistent grid that fills every CU leaves RCCL's send / recv kernels no registers
	// to start with (5 waves x 96 VGPRs of 512 per SIMD), and the exchange would only run in the gaps between the
	// kernels; a few workgroups fewer leave room on some CUs (pwn_tiled.cpp sets the number)
	// ... and frames on two compute streams: room for the other stream's kernels (PWN_OPT_TRACE_ROOM; the caller says how much)
	p.cost_mul = (uint32_t)grid;
	if(S.reserve > 0 && grid > 2 * S.reserve) grid -= S.reserve;
	p.cost_div = (uint32_t)grid;
	// Tile pairs (trace_kernel.hip): a frame's launch without an order hands out 32-pixel tiles, two units to a ticket -- where its
	// tickets would go out two at a time (16 units or more per wave of the grid: the kernel's rule for draw_n), or always
	// (PWN_TILE_PAIRS=2).  What the queues hold is then a row's tiles, ceil(tiles_x / 2), times the rows of units.
	p.items = p.tiles_total;
	if(!S.refill && !batch && !S.want_cost && (S.tile_pairs == 2 || (S.tile_pairs == 1 && (long long)p.tiles_total >= 16ll * 4 * grid)))
	{
		const int tx = (p.tiles_x + 1) / 2;
		p.tile_pairs = 1;
		pwn_unit_div_magic((uint32_t)tx, &p.tx_magic, &p.tx_shift);
		// The middle rows stay single units, in whole rows: the first round of the launch at least -- one item per wave of the grid, the
		// static first tickets -- and a fifth of the rows.  That is where rays run longest (the middle-out order starts there for the
		// same reason), and in a scene where single units are most of a launch the wave that holds one must not hold its neighbour too:
		// synth256 at 4K has a column of such units down the middle of the frame, the dearest 1 744 wave steps, and a launch is as long
		// as the dearest item: with tiles throughout, two neighbours of 1 295 + 1 069 steps (+37 % launch time); with the first round
		// alone single, still those two (+22 %); outside the middle fifth the dearest tile has 577.  The tiles' saving is lost on that
		// fifth.  PWN_TILE_PAIRS=2: tiles from the first ticket on.
		const int rows = p.tiles_total / p.tiles_x;
		int single = 0;
		if(S.tile_pairs != 2)
		{
			single = (4 * grid + p.tiles_x - 1) / p.tiles_x;
			if(single < (rows + 4) / 5) single = (rows + 4) / 5;
		}
		if(single > rows) single = rows;
		p.pair_single_rows = single;
		p.items = single * p.tiles_x + tx * (rows - single);
	}
	// fewer units (tiles, where they go out in pairs) than resident waves (a 320 x 240 frame is 1200 units for 5120 waves): one
	// per wave, a workgroup per four of them -- a workgroup whose waves find nothing still copies the tables into LDS
	{
		const int wg_waves = 4;          // PWN_BLOCK / 64
		if(!S.refill && grid > (p.items + wg_waves - 1) / wg_waves) grid = (p.items + wg_waves - 1) / wg_waves;
		if(grid > p.items) grid = p.items;
	}
	p.grid = grid;
	*out = p;
	return 0;
}
