// tables.h -- layout of the per-level table blob shared by the host packer
// (pwn_tables.cpp) and the kernels.  The blob is built once per level / sphere
// upload, lives in HBM, and is copied verbatim into LDS by every workgroup.
//
//   [0      .. 4096)   rcp      u16 [2048]        RCPPS table     (trace.h:231), see dev_math.h
//   [4096   .. 8192)   rsqrt    u16 [2048]        RSQRTPS table   (util.h:43)
//   [8192   .. 8448)   faces    f32 [4][4] + [6][8]  constants of the shading step, looked up per lane:
//                       [base] = colour of a wall class, b g r - (trace.h:108-154; BASE_* of trace_common.h);
//                       [face] = what hitting face FXP..FYN does (defs.h:25-33): sign masks that mirror the
//                       ray, its reflectivity; the 0.001 step off the surface per axis (-0.0f where the
//                       axis is not the face's: x + -0 = x), the sign mask of the diffuse term
//   [8448   .. 8704)   exp2     u64 [32]          glibc expf's 2^(i/32) table (dev_math.h), for the fog composites
//   [8704   .. 25604)  cellinfo u32 [65][65]     ONE word per cell for the walk loop.
//                       Row/column 64 repeat row/column 0 WITHOUT the sphere bit:
//                       get_cell's per-axis clamp-to-0 (util.h:151-158) becomes
//                       min(c, 64) and the in-bounds test in front of the sphere
//                       loop (trace.h:252) is folded into the word.
//                       bits 0..7   what the walk's portal arms ask of the cell, baked per level (cell_bake.h):
//                                   PWN_C_LT2 / PWN_C_LTDQ, what a ray leaving a 2-high room sees there (through a
//                                   portal too); bits 2..7 the portal state of a letter: wall, magenta wall, or
//                                   2 + the number of its endpoint record
//                       bit  8      PWN_C_ROOM   ; $ "  #  &   (1-high or 2-high room)
//                       bit  9      PWN_C_ROOM2  # &
//                       bit  10     PWN_C_FOG    $ &
//                       bit  11     PWN_C_DQ     "
//                       bit  12     PWN_C_RAMP   > < , ^
//                       bit  13     PWN_C_RAMPX  > <            (tilt along x)    | in a letter's cell that is an endpoint:
//                       bit  14     PWN_C_RAMPM  > ,            (ray.y -= ramp*tilt) | the rotation from there, 0..3 (cell_bake.h)
//                       bit  15     PWN_C_PORTAL A..Z
//                       bits 16..30 first entry of this cell's sphere list in binidx
//                       bit  31     PWN_C_SPH    the cell holds >= 1 sphere
//   [25616  .. 25824)  eprec    u32 [52]          endpoint records of the portals (cell_bake.h; defs.h:87-94): the way to the other
//                                                 endpoint as two half floats
//   [25824  .. +2*nbin pad 16)  binidx u16        per-cell sphere lists (level.h:64-81),
//                                                 object order, as BYTE offsets into the sphere
//                                                 array (index * 32), each list closed by 0xffff
//   [...    .. +32*nsph)        spheres 8 x f32   x, y, z, r*r | refl, cb, cg, cr: what a test reads is ONE 16-byte
//                                                 load (r only ever enters as r*r, trace.h:262,270; the host squares it
//                                                 in fp32 like the reference does)
// A sphere set whose lists outgrow LDS takes the lists' GLOBAL form (below, PWN_LF_GLOBAL): LDS ends with a u32 per non-empty
// cell at PWN_T_BINIDX; records, "which sphere" and spheres lie in a device-memory buffer of their own.
#pragma once
#include <stdint.h>
#include "cell_bake.h"
#include "sphere_bound.h"

#define PWN_GRID_PITCH 65u
#define PWN_T_RCP      0u
#define PWN_T_RSQ      4096u
#define PWN_T_FACES    8192u
#define PWN_T_EXP2     8448u
#define PWN_T_CELLINFO 8704u
#define PWN_T_EPREC    25616u
#define PWN_T_BINIDX   25824u

// table entry -> fp32 pattern of the result for a zero exponent field (dev_math.h):
// entry = (1 - exponent offset) << 12 | result mantissa bits 22..11
#define PWN_RCP_BASE   0x7e800000u   /* 253 << 23 */
#define PWN_RSQ_BASE   0x5f000000u   /* 190 << 23 */

#define PWN_C_ROOM   0x0100u
#define PWN_C_ROOM2  0x0200u
#define PWN_C_FOG    0x0400u
#define PWN_C_DQ     0x0800u
#define PWN_C_RAMP   0x1000u
#define PWN_C_RAMPX  0x2000u
#define PWN_C_RAMPM  0x4000u
#define PWN_C_PORTAL 0x8000u
#define PWN_C_SPH    0x80000000u
#define PWN_LIST_END 0xffffu

static inline uint32_t pwn_t_sph_offset(uint32_t nbin)
{
	return PWN_T_BINIDX + ((nbin * 2u + 15u) & ~15u);
}
static inline uint32_t pwn_t_total(uint32_t nbin, uint32_t nsph)
{
	return pwn_t_sph_offset(nbin) + nsph * 32u;
}
// The per-cell lists with the sphere records INLINE (round 5; the unit scheduler's kernels, where the blob still leaves five
// workgroups per CU): at PWN_T_BINIDX nrec records of 16 bytes -- x, y, z, r*r of the sphere, one per (cell, sphere) pair in
// object order, the LAST record of a cell's list with the sign bit of r*r set (r*r is never negative) -- then nrec u16 "which
// sphere" (its byte offset in the sphere array: read when a hit is shaded, not per test), then the spheres as before.  A test is
// then ONE LDS read whose address does not depend on another read (level.txt: all 14 spheres sit in one cell, a ray through it
// makes 14 tests in a row).  The cell word's offset field counts records.
static inline uint32_t pwn_t_recsph_offset(uint32_t nrec) { return PWN_T_BINIDX + nrec * 16u; }
static inline uint32_t pwn_t_sph_offset_inl(uint32_t nrec) { return pwn_t_recsph_offset(nrec) + ((nrec * 2u + 15u) & ~15u); }
static inline uint32_t pwn_t_total_inl(uint32_t nrec, uint32_t nsph) { return pwn_t_sph_offset_inl(nrec) + nsph * 32u; }

// The per-cell lists in DEVICE MEMORY (sphere sets whose lists outgrow LDS, up to PWN_OBJ_MAX spheres: pwn_tables_plan, pwn_tables.cpp).
// LDS holds the blob up to and including eprec and, at PWN_T_BINIDX, `liststart`: one u32 per NON-EMPTY cell, the index of that
// cell's first record.  The cell word keeps PWN_C_SPH; its bits 16..30 hold the non-empty cell's ordinal (at most 4096 cells,
// however many records there are).  A buffer apart from the blob, in 16-byte aligned sections, nothing in it 16-bit:
//   nrec + 1 records of 16 bytes, exactly the inline form's (x, y, z, r*r; the sign of r*r set on a cell's last record) -- the one
//            more is what the walk's read-ahead behind the very last record lands on;
//   nrec u32 "which sphere": the sphere's INDEX, read when a hit is shaded or recorded (pwn_hit.object is it);
//   nsph spheres of 32 bytes, as in the blob.
// The units kernel only (trace_kernel.hip, its LISTS parameter); a test is one 16-byte global load, the next record requested first.
enum { PWN_LF_INDEXED = 0, PWN_LF_INLINE = 1, PWN_LF_GLOBAL = 2 };
static inline uint32_t pwn_t_total_glb(uint32_t ncell) { return PWN_T_BINIDX + ((ncell * 4u + 15u) & ~15u); }
static inline uint64_t pwn_g_which_offset(uint64_t nrec) { return (nrec + 1u) * 16u; }
static inline uint64_t pwn_g_sph_offset(uint64_t nrec) { return pwn_g_which_offset(nrec) + ((nrec * 4u + 15u) & ~(uint64_t)15u); }
static inline uint64_t pwn_g_total(uint64_t nrec, uint64_t nsph) { return pwn_g_sph_offset(nrec) + nsph * 32u; }

// glibc 2.35 e_expf.c / exp2f_data: 2^(i/32) as double bit patterns with the exponent adjusted (N = 32)
#define PWN_EXP2F_TAB_INIT { \
	0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, \
	0x3fef72b83c7d517b, 0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1, \
	0x3fef06fe0a31b715, 0x3feef1a7373aa9cb, 0x3feedea64c123422, 0x3feece086061892d, \
	0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429, 0x3feea47eb03a5585, \
	0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13, \
	0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d, \
	0x3feee89f995ad3ad, 0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069, \
	0x3fef5818dcfba487, 0x3fef7c97337b9b5f, 0x3fefa4afa2a490da, 0x3fefd0765b6e4540 }

// the constant shading tables at PWN_T_FACES and PWN_T_EXP2 (host: pwn_i_pack_blob)
static inline void pwn_fill_faces(float *f)
{
	// wall class -> colour factors (BASE_CEIL, BASE_FLOOR, BASE_WALL, BASE_MAGENTA of trace_common.h)
	static const float col[4][4] = { { 30.0f, 30.0f, 0.0f, 0.0f }, { 1.0f, 1.0f, 1.0f, 0.0f }, { 0.8f, 0.8f, 1.0f, 0.0f }, { 5.0f, 0.0f, 5.0f, 0.0f } };
	for(int i = 0; i < 16; i++) f[i] = col[i >> 2][i & 3];
	// face (FXP, FZP, FXN, FZN, FYP, FYN) -> mirror masks x y z, reflectivity | step x y z, diffuse sign mask
	uint32_t *u = (uint32_t *)(f + 16);
	const uint32_t S = 0x80000000u, P = 0x3a83126fu /* 0.001f */, N = 0xba83126fu, Z = 0x80000000u /* -0.0f */;
	const uint32_t R25 = 0x3e800000u /* 0.25f */, R70 = 0x3f333333u /* 0.7f */;
	const uint32_t t[6][8] = {
		{ S, 0, 0, R25,  N, Z, Z, 0 },        // FXP: ray.x = -ray.x, pos.x -= 0.001 (trace.h:50-75)
		{ 0, 0, S, R25,  Z, Z, N, 0 },        // FZP
		{ S, 0, 0, R25,  P, Z, Z, S },        // FXN: pos.x += 0.001, diffuse = -ray.x
		{ 0, 0, S, R25,  Z, Z, P, S },        // FZN
		{ 0, S, 0, R25,  Z, N, Z, 0 },        // FYP (ceiling)
		{ 0, 0, 0, R70,  Z, N, Z, S },        // FYN (floor): pos.y -= 0.001, then the rippled normal mirrors the ray
	};
	for(int i = 0; i < 48; i++) u[i] = t[i >> 3][i & 7];
	static const uint64_t e2[32] = PWN_EXP2F_TAB_INIT;
	uint64_t *e = (uint64_t *)(f + (PWN_T_EXP2 - PWN_T_FACES) / 4u);
	for(int i = 0; i < 32; i++) e[i] = e2[i];
}

// class bits of a cell type (trace.h:300-666 switch labels)
static constexpr inline uint32_t pwn_cell_class(uint32_t c)
{
	switch(c)
	{
		case ';': return PWN_C_ROOM;
		case '$': return PWN_C_ROOM | PWN_C_FOG;
		case '"': return PWN_C_ROOM | PWN_C_DQ;
		case '#': return PWN_C_ROOM | PWN_C_ROOM2;
		case '&': return PWN_C_ROOM | PWN_C_ROOM2 | PWN_C_FOG;
		case '>': return PWN_C_RAMP | PWN_C_RAMPX | PWN_C_RAMPM;
		case '<': return PWN_C_RAMP | PWN_C_RAMPX;
		case ',': return PWN_C_RAMP | PWN_C_RAMPM;
		case '^': return PWN_C_RAMP;
	}
	return (c >= 'A' && c <= 'Z') ? PWN_C_PORTAL : 0u;
}

// kernel arguments of one trace launch (rows [y0,y1) of a w x h frame)
struct pwn_trace_params
{
	float rayb[4], rdx[4], rdy[4], from[4];   // screen.h:43-57
	float sec_current;                        // defs.h:23
	int w, h, y0, y1;
	int tiles_x, tiles_total;                 // 16 x 4 pixel units (one wave64 each): per row, in all
	uint32_t ux_magic; int ux_shift;          // unit / tiles_x = (unit * ux_magic >> 32) >> ux_shift for unit < 2^31; ux_shift < 0: divide
	uint32_t blob_bytes, off_sph;
	uint32_t *sbuf;                           // full frame, pitch w
	float *zbuf;                              // full frame, pitch w
	const uint32_t *blob;
	unsigned long long *counters;             // 24 x u64 (pwn_stats counters, wave_paths, residency) or NULL
	unsigned long long *wave_log;             // counting builds, diagnosis: (start, end) of every wave, 100 MHz ticks; or NULL
	int has_w;                                // camera has w components (general 4-lane path)
	int scheduler;                            // PWN_SCHED_* (pwnhip.h)
	int refill_limit;                         // PWN_SCHED_REFILL: walk on while more lanes than this walk (trace_refill.hip)
	// work queues of the wave scheduler (trace_kernel.hip): PWN_QUEUES counters, one per 128 B,
	// for this launch; the set of the next launch, which this one clears
	uint32_t *tickets, *tickets_next;
	uint32_t *cost_word;                      // NULL, or a word this launch adds the sum of its waves' lifetimes to (100 MHz ticks): what
	                                          // the rows cost, for the row tiling's moving cuts (pwn_tiled.cpp)
	uint16_t *unit_cost;                      // NULL, or one entry per unit: how long the wave that traced it spent on it, in 40 ns (four ticks of the
	                                          // 100 MHz clock, saturating) -- what the NEXT launch of this geometry is ordered by (PWN_OPT_UNIT_ORDER,
	                                          // post_kernels.hip pwn_order_kernel), and what tools/unit_order_sim.py replays
	const uint32_t *perm;                     // NULL (units in arithmetic order: rows from the frame's middle outwards), or the hand-out order of
	uint32_t perm_cap;                        // every queue: perm[q * perm_cap + ticket] = the unit that ticket of queue q stands for
	uint32_t *clear_word;                     // NULL, or a word this launch sets to 0 (the row tiling's miss word of the frame:
	                                          // the blur of the same frame, behind this launch on the stream, counts in it)
	uint32_t off_recsph;                      // != 0: the blob holds the per-cell lists with inline sphere records (above); where their "which sphere" array is
	// A batch of views (pwn_trace_views): NULL, or nviews records below that take the place of rayb ... sec_current per view.  The
	// launch's units are nviews x the units of one frame, handed out interleaved (trace_kernel.hip); view v's planes start at
	// sbuf / zbuf + v * plane.  nviews / views_magic / views_shift: unit / nviews as ux_magic / ux_shift divide by tiles_x.
	const struct pwn_view_rec *views;
	int nviews;
	uint32_t views_magic; int views_shift;
	unsigned long long plane;                 // pixels per view (w * h)
	// A batch of caller-supplied rays (pwn_trace_rays): NULL, or nrays records of 8 fp32 (origin x y z w, direction x y z w; 16-byte
	// aligned) that take the place of the frame: ray i's seed is ray_seeds[i] (NULL: 0), its colour goes to sbuf[i], its depth is
	// zbuf[i] (in / out).  ray_w = 0: the w lanes are taken as 1 and 0 (PWN_RAYS_HAS_W not given).
	const float *rays;
	const uint32_t *ray_seeds;
	uint32_t nrays;
	int ray_w;
	// First-hit records of a batch of rays (pwn_trace_hits): NULL, or nrays records of PWN_HIT_REC_BYTES (pwn_hit of pwnhip.h; 16-byte
	// aligned) that ray i's primary segment is written to.  Then sbuf, zbuf, ray_seeds and sec_current are not read.
	// With `views` (pwn_trace_view_hits): the first-hit planes of a batch of views.  The launch is one of `views` whose units trace the
	// primary segment alone and write, per pixel, one packed word of what it ended on (pwnhip.h PWN_LABEL_*) to `hits`, the label
	// plane (uint32), and -- each unless NULL -- the hit's cell word to sbuf and its distance to zbuf: nviews planes of `plane` words
	// each, view v's at + v * plane.  The records' sec_current is not read.  (No field of its own: the struct, and with it every
	// other kernel's argument block, stays as it was.)
	// With `vps` (pwn_trace_viewport_hits): the same three planes for views of their own sizes -- ONE plane of w x h words each, pitch w,
	// in which view i's pixel (x, y) lies at (rec.y + y) * w + rec.x + x; the launch is one of `vps` otherwise, and the records'
	// sec_current is not read.
	void *hits;
	// The lists' global form (above): NULL, or the three sections of the device-memory part of the tables.  Then blob_bytes is the LDS
	// part alone, and off_sph / off_recsph are not read.
	const float *g_rec;
	const uint32_t *g_which;
	const float *g_sph;
	// Views of their own sizes composited into one frame (pwn_trace_viewports): NULL, or nvp records (pwn_viewport_rec below) that
	// take the place of rayb ... sec_current AND of w, h, y0, y1, tiles_x, ux_magic per view; w is then the pitch of sbuf / zbuf
	// alone.  tiles_total = the units of all views; vp_step0 = the first stride of the kernel's search for a ticket's segment, the
	// largest power of two below nvp (0 for one view).
	const struct pwn_viewport_rec *vps;
	int nvp;
	uint32_t vp_step0;
	// Bounding balls of the longest per-cell lists (sphere_bound.h; pwn_sphere_bounds_build): nbounds of them, made from the lists
	// that THIS launch's copy of the tables was packed from.  By value in the launch's arguments, so that launches in flight on two
	// streams and the copies of the tables stay consistent, and because no form of the tables has room for them (their byte sizes are
	// pinned: pwn_sphere_tables_plan).  The walk reads them with scalar loads from the kernel's arguments (trace_walk.inc): the four ids at
	// once -- bound_ids[k] = bounds[k].id, 0xffffffff where there is none -- then the one record.  nbounds = 0: PWN_SPHERE_BOUNDS=0, or no list
	// long enough.
	int nbounds;
	uint32_t bound_ids[PWN_BOUNDS_MAX];
	pwn_sphere_bound bounds[PWN_BOUNDS_MAX];
	// Tile pairs (trace_kernel.hip, frames without an order; PWN_TILE_PAIRS): != 0: a ticket stands for a 32-pixel tile, whose two
	// units the wave that draws it traces one after the other; tx_magic / tx_shift divide by the tiles per row, ceil(tiles_x / 2),
	// as ux_magic / ux_shift divide by the units per row.  (Behind everything else: no other kernel's argument moves.)
	// pair_single_rows: so many rows of units, the first in the launch's middle-out order, go out as single units in front of the tiles.
	int tile_pairs;
	uint32_t tx_magic; int tx_shift;
	int pair_single_rows;
	// One hidden sphere per ray or view (pwn_trace_hits_hide_device, pwn_trace_views_hide_device, pwn_trace_view_hits_hide_device; the
	// kernel's HIDE parameter).  ray_hide: NULL, or nrays int32 beside `rays`: ray i does not see the sphere whose index in the live table
	// (pwn_hit.object's numbering) is ray_hide[i]; any other value hides nothing -- with `hits` the rays' first hits, without it their
	// colours (pwn_trace_rays_hide_device).  view_hide != 0: a launch of `views` or of `vps` whose records' `hide` words count
	// (pwn_view_rec, pwn_viewport_rec).  Only kernels with the HIDE bit in their mode read ray_hide; NO kernel reads view_hide -- the
	// launch's mode says it (pwn_launch_trace) -- and the word is still set and stays where it is: without it ray_reach would move in
	// every kernel's arguments.  (Behind everything else, as the tile pairs were: no other field moves.)
	const int32_t *ray_hide;
	int view_hide;
	// Rays that stop after a given distance (pwn_trace_reach, pwn_trace_reach_device, pwn_trace_reach_hide_device; the kernel's REACH
	// parameter).  NULL, or nrays floats beside `rays` in a launch of `hits`: ray i's walk stops behind the first step that leaves its
	// distance above ray_reach[i], and a ray that stops so gets a PWN_HIT_FREE record (pwnhip.h).  The value is only ever compared and
	// multiplied.  Only kernels with the REACH bit in their mode read it.  (Behind everything else, as ray_hide was: no other field moves.)
	const float *ray_reach;
};
#define PWN_HIT_REC_BYTES 48u

// kernel arguments of one blur launch (post_kernels.hip; rows [y0,y1) of a w x h frame)
struct pwn_blur_params
{
	int w, h, y0, y1;
	int groups;                    // w / 4 (screen.h:91: cx < dimx-3)
	const uint32_t *pre;           // full pre-blur frame ("tsbuf")
	const float *zbuf;             // full frame depth
	uint32_t *out;                 // full frame
	const uint2 *skip;             // groups x (A_g, C_g)
	// row tiling with a bounded exchange: only rows [avail_y0, avail_y1) of `pre` hold this
	// frame; a tap that lands outside them makes the kernel add to *miss (the caller then
	// repeats the strip with the whole frame present).  miss == NULL: every row is valid.
	int avail_y0, avail_y1;
	uint32_t *miss;
	int tile_h, tile_w, batch;     // a workgroup's tile of output pixels (rows, columns) and the form of its staging loop: pwn_i_launch_blur picks
	                               // them by the size of the launch, pwn_launch_blur has the instantiations
	// row tiling with moving cuts: the trace launch in front of this one on the stream added up what its strip cost
	// in *cost_acc (pwn_trace_params.cost_word); this launch moves the sum to *cost_out, the word that travels with
	// the frame, and clears the accumulator for the stream's next trace.  Both NULL otherwise.
	uint32_t *cost_acc, *cost_out;
	uint32_t cost_mul, cost_div;   // ... scaled on the way: the resident grid over the grid the trace ran with (PWN_OPT_TRACE_ROOM), so that ranks with and without room compare
	// a batch of views (pwn_trace_views): 0 = one frame; else that many frames of w x h, view v's planes at pre / zbuf / out + v * plane
	int views;
	unsigned long long plane;
	// views of their own sizes in one frame (pwn_trace_viewports): NULL, or nvp records -- blockIdx.y = the view, whose rectangle
	// of the pitch-w planes is blurred as a frame of its own; vp_tiles = the tiles of the view that has most (the launch's grid)
	const struct pwn_viewport_rec *vps;
	int nvp, vp_tiles;
};

// what a launch of the trace kernel traces (its MODE parameter, trace_kernel.hip; which modes have kernels, and where: trace_variants.h)
enum { PWN_KM_FRAME = 0, PWN_KM_VIEWS = 1, PWN_KM_RAYS = 2, PWN_KM_HITS = 3, PWN_KM_VIEWPORTS = 4, PWN_KM_VIEW_HITS = 5, PWN_KM_VIEWPORT_HITS = 6 };
// ... or'ed to it: its HIDE parameter -- every view or ray names one sphere it does not see
enum { PWN_KM_HIDE = 8 };
// ... its REACH parameter -- every ray names a distance behind which it stops (pwn_trace_params.ray_reach)
enum { PWN_KM_REACH = 16 };

// One view of a batch: the camera set-up of screen.h:43-57 for that view's camera (pwn_internal.h frame_setup) and its
// sec_current.  80 bytes; the kernel reads a view's record with scalar loads.
// hide (word 17): 0 = the view sees every sphere; k + 1 = it does not see sphere k of the live table (pwn_trace_views_hide_device:
// view_setup.hip writes k + 1 for 0 <= k < PWN_OBJ_MAX and 0 for anything else).  Only the HIDE instantiations read the word; every
// other path that makes records writes 0 there (a float 0.0f before the word had a name: the same bits).
struct pwn_view_rec
{
	float rayb[4], rdx[4], rdy[4], from[4];
	float sec_current;
	uint32_t hide;
	float pad_[2];
};
#define PWN_VIEWS_REC_BYTES 80u

// One view of pwn_trace_viewports: pwn_view_rec's fields for a frame of the view's OWN size, then its rectangle of the context's
// frame and what turns a unit number of the view into a place in it.  128 bytes; scalar loads, as a view record.
// The records are in order of rising `units`.  The launch hands its units out in ROUNDS: round r is unit r of every view that
// has more than r units, so all views advance together, each from its middle row outwards, and a view drops out when it is done.
// Views s .. nvp-1 take part in rounds [units of record s-1, units of record s): "segment" s, whose fields sit in record s --
// seg_first = the launch's first ticket of the segment (rising with s; equal for an empty segment), seg_round = its first round,
// seg_magic / seg_shift = the division by its nvp - s participants (pwn_unit_div_magic; shift < 0: one participant).
// hide (word 30, byte 120): pwn_view_rec's word of that name -- 0 = the view sees every sphere, k + 1 = it does not see sphere k of
// the live table (pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device: viewport_setup.hip writes it from the entry
// of the record's RECTANGLE, d_hide[perm[j]]).  Only the HIDE instantiations read it; every other path that makes records leaves 0.
struct pwn_viewport_rec
{
	float rayb[4], rdx[4], rdy[4], from[4];
	float sec_current;
	int32_t x, y, w, h;                       // the rectangle
	uint32_t units_x; uint32_t ux_magic; int32_t ux_shift;     // ceil(w / 16) and unit / units_x (pwn_trace_params.ux_magic)
	uint32_t rows_u;                          // ceil(h / 4)
	uint32_t units;                           // units_x * rows_u
	uint32_t seg_first, seg_round, seg_magic; int32_t seg_shift;
	uint32_t hide;
	uint32_t pad_;
};
#define PWN_VP_REC_BYTES 128u

// What the players' step (player_step.hip) reads of a level: the raw cell characters (lv->data, defs.h:103) and the portal table
// (lv->pmap, seven int32 a letter: pwn_portal), neither of which the baked cell words hold.  4096 + 728 bytes, padded to whole
// 16-byte words (the upload kernel and the step's LDS staging move those).
struct pwn_walk_table
{
	uint8_t cells[4096];
	int32_t pmap[26 * 7];
	uint32_t pad_[2];
};
#define PWN_WALK_BYTES 4832u

#ifndef PWN_QUEUES
#define PWN_QUEUES 64u                       /* a power of two <= 64: one lane of a wave looks at each */
#endif
#define PWN_QUEUE_STRIDE 32u                  /* uint32 words between two counters (128 B) */
