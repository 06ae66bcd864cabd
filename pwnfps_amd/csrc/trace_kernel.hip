// trace_kernel.hip -- the per-pixel portal ray-march on gfx950 (CDNA4).
//
// Replaces trace_ray_prelude (screen.h:1-28) + trace_ray / trace_ray_through /
// trace_hit_wall / trace_hit_bounce (trace.h) of the reference.
//
// Shape: persistent 256-thread workgroups (4 wave64), exactly as many as are
// resident at once.  Each workgroup copies the level blob (rcp/rsqrt tables,
// per-cell word, portals, per-cell sphere lists, spheres: tables.h) HBM -> LDS
// once; then every wave pulls 16x4-pixel units of the row strip from work
// queues until none are left (rays differ in cost by an order of magnitude
// across a frame; see the kernel body), one thread per pixel.
// The reference's recursion (depth <= REFLECT) is a loop over at most three ray
// segments; the composites of trace.h:91-101 are applied on unwinding.
// Output: BGRA8 colour + fp32 depth, row-major, 4-byte stores.
//
// No MFMA: this is a branchy DDA, not a contraction.  HBM traffic is the two
// output planes only (8 B / pixel); everything the inner loop reads is in LDS.
// Its time follows the number of wave-instructions issued, so the code
// is organised for few instructions per cell step and few scalar mask sequences:
//   - one walk loop with one exit; the cell class is a bit test on ONE LDS
//     word per step (class flags + sphere-list offset, 65x65 clamp-free grid),
//   - the room body (1-high and 2-high share it) is written with selects,
//   - the per-tile ray add-chain is built systolically with DPP row shifts,
//   - rcp/rsqrt table hits cost an index, a ds_read_u16 and a subtract,
//   - cameras without w components (the usual case) take a 3-lane path that
//     is arithmetically identical to the 4-lane SSE code (see HAS_W below),
//   - no device function calls (dev_math.h) and no SLP packing (Makefile).
#include <hip/hip_runtime.h>
// (dev_math.h: the segment's text stands here once per bounce depth, and with it the floor's sine and cosine -- their constants are
// made where they are used, not once in front of the unit loop, where they would be two register pairs more across every walk)
template<unsigned long long BITS> static __device__ __forceinline__ double pwn_f64_here()
{
	unsigned lo, hi;
	asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=v"(lo), "=v"(hi) : "i"((unsigned)BITS), "i"((unsigned)(BITS >> 32)));
	return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}
#define PWN_F64_HERE(c) pwn_f64_here<__builtin_bit_cast(unsigned long long, (double)(c))>()
#include "trace_common.h"
#include "pwnhip.h"      // PWN_OBJ_MAX (hit_store_planes)

// The walk loops of this file count a segment's cell steps in ev itself (trace_pixel: "How the walk loop ends"): below zero while
// the ray walks, and what a ray that made WALK_STEPS steps (trace.h:250) without an event leaves the loop with is this file's
// "out of steps" -- the shared enum's 0, not its EV_EXHAUSTED, which is the refill kernel's.
#define WALK_STEPS 1000
#define EV_OUT_OF_STEPS 0
#define WALK_EV_KEEP ev
#define WALK_EV_OPEN(e) ((e) <= 0)
// The hidden sphere (HIDE, at the kernel): hide1 = 0 for none, k + 1 for sphere k of the live table -- a view's from its record, one
// value for the wave; a ray's from pwn_trace_params.ray_hide, one per lane.  The value is only ever compared with an object number that
// comes out of the tables (trace_walk.inc PWN_ST_OBJECT): no bit pattern of it reaches an address or a loop bound.  Object numbers are
// below PWN_OBJ_MAX, so 0, and whatever a value that is no index turns into, equal none of them.  With HIDE false the test is the
// constant `false` and its argument is not evaluated: no instruction is made for it.
#define WALK_HIDDEN(object) (HIDE && (object) + 1u == hide1)

// One pixel = trace_ray(0, ...) of screen.h:22-24 with the recursion unrolled.
// HIDE: the sphere hide1 stands for (WALK_HIDDEN above) is not there for this ray, on any of its segments.
template<bool COUNT, bool HAS_W, int LISTS, bool HIDE = false>
__device__ __forceinline__ void trace_pixel(const Lds &L, float sec_current, uint32_t seed,
	Vec<HAS_W> from, Vec<HAS_W> iray, float &out_x, float &out_y, float &out_z, float &out_w,
	float *zpix, Counters &cnt, [[maybe_unused]] uint32_t hide1 = 0u)
{
	typedef Vec<HAS_W> V;
	// (trace_walk.inc: nothing is kept for hit records here; the two names it would write are never touched)
	constexpr bool HITREC = false;
	[[maybe_unused]] uint32_t hit_cxz;
	[[maybe_unused]] int hit_portals;
	// icol (screen.h:24).  Its w lane, and the w lane of every surface colour, is
	// x * 0.0f (COL_* have a = 0, defs.h:17-19; spheres get b,g,r only, script.h:30-32):
	// +-0 for any finite input, and the sign of a zero never reaches a pixel, so the
	// w lanes of icol and of the composite stack are not kept.
	// The composite stack (reflectivity, fog, colour of the surfaces the ray bounced off): two entries under names of their
	// own, A for the first surface and B for the second.  The segment's text stands below once per bounce depth
	// (trace_segment.inc), so which entry a copy writes, and which one's colour it is lit with -- the entry of the surface
	// it came off IS the segment's icol (trace.h:90); the primary segment's is 1,1,1 -- is settled where the copy is
	// included: nothing is shifted, copied at a join or tested.
	// (an entry is written when its surface is met and read only by a lane that bounced that often; it has no value before,
	// and so takes no register in the copies in front of the one that writes it)
	float stA_refl, stA_fog, scAx, scAy, scAz;
	float stB_refl, stB_fog, scBx, scBy, scBz;
	// `depth`, the number of surfaces a pixel's ray bounced off, is per lane and set where the lane leaves its copy.
	int depth;
	float vx, vy, vz, vw;
	asm volatile("" : "=v"(vx)); asm volatile("" : "=v"(vy)); asm volatile("" : "=v"(vz));
	// The colour's w lane is not carried: every surface colour has w = 0 (defs.h:16-18, spheres'
	// col.w is never set), so col.w = diffuse * (icol.w * 0) is 0 -- unless the shading factor is
	// not finite (a ray that went through 1/0 in a ramp, trace.h:461), when it is NaN and so is
	// everything composited from it.  One accumulator stands for that lane: w_acc += factor * 0 stays
	// +0 until a factor is NaN or inf and is NaN from then on (a register rather than a flag: a
	// lane-divergent bool carried across the walk loop costs three mask updates per iteration).
	float w_acc = 0.0f;

	// (carried from segment to segment: the position -- a segment starts where the one before ended, trace.h:86-89 -- and the
	// sphere candidate's fields behind aux_dist, which alone is reset per segment)
	V pos = from;
	float aux_diff = 0.0f;
	uint32_t aux_idx = 0;
	V aux_pos, aux_norm;
	aux_pos.x = aux_pos.y = aux_pos.z = aux_pos.w = 0.0f;
	aux_norm = aux_pos;
	// The reference's recursion, one copy of the segment's text per depth (the last one cannot bounce).  One text with the depth in a
	// scalar register was this kernel's form before: its joins, the stack's shift and its tests on the depth were a tenth of a
	// frame's vector moves and more scalar than vector work behind every walk.
	static_assert(REFLECT_MAX == 2, "trace_segment.inc is included once per bounce depth");
#define PWN_SEG 0
#include "trace_segment.inc"
#undef PWN_SEG
#define PWN_SEG 1
#include "trace_segment.inc"
#undef PWN_SEG
#define PWN_SEG 2
#include "trace_segment.inc"
#undef PWN_SEG

ray_done:
	// trace.h:91-101, innermost first: the composite's text (trace_composite.inc) takes the stack's top entry first, and which
	// entry that is depends on the lane -- B for a ray that bounced twice, A for one that bounced once.  So the text is included
	// once per entry, each time as a stack of that one entry: B for the lanes with depth 2, then A for those with depth >= 1 --
	// the same operations in the same order per lane as one pass over a shifted stack.  (The text's second level is dead in both:
	// the stack it sees is one entry deep.  The first inclusion's counters are that level's: RG_COMP2 and RG_COMP2_FOG count entry B's
	// pass, RG_COMP1 and RG_COMP1_FOG entry A's -- the entry counts of the shifted stack's two levels, the fog counts per entry where
	// they were per level: trace_common.h.)
	{
		const int depth_lane = depth;
#define st_refl1 st_refl0
#define st_fog1 st_fog0
#define sc1x sc0x
#define sc1y sc0y
#define sc1z sc0z
		{
			const int depth = depth_lane >= 2 ? 1 : 0;
#define st_refl0 stB_refl
#define st_fog0 stB_fog
#define sc0x scBx
#define sc0y scBy
#define sc0z scBz
#define RG_COMP1 RG_COMP2
#define RG_COMP1_FOG RG_COMP2_FOG
#include "trace_composite.inc"
#undef RG_COMP1
#undef RG_COMP1_FOG
#undef st_refl0
#undef st_fog0
#undef sc0x
#undef sc0y
#undef sc0z
		}
		{
			const int depth = depth_lane >= 1 ? 1 : 0;
#define st_refl0 stA_refl
#define st_fog0 stA_fog
#define sc0x scAx
#define sc0y scAy
#define sc0z scAz
#include "trace_composite.inc"
#undef st_refl0
#undef st_fog0
#undef sc0x
#undef sc0y
#undef sc0z
		}
#undef st_refl1
#undef st_fog1
#undef sc1x
#undef sc1y
#undef sc1z
	}
	//@R p_comp
	out_x = vx; out_y = vy; out_z = vz; out_w = vw + w_acc;
}

// One ray's PRIMARY segment for pwn_trace_hits and pwn_trace_view_hits: the set-up and the walk of trace_pixel's first pass through
// its loop -- the same two texts -- and then, where trace_pixel shades, the walk's state as the twelve words of a record (pwn_hit, pwnhip.h):
//   word 0..3    kind (EV_WALL = PWN_HIT_WALL, EV_SPHERE = PWN_HIT_SPHERE, out of steps = PWN_HIT_NONE), face, object, portals
//   word 4..7    dist (what the frame writes to zbuf), x, y, z (pos, or the sphere candidate's aux_pos)
//   word 8..11   the walked ray x, y, z;  cell x | cell z << 16 (hit_cxz as the walk packs it: two int16)
// No shading, bounce, jitter or composite, no composite stack, no random number, no sec_current.
// trace_hit is the one body; what becomes of the words is its callers': hit_store_record (a batch of rays) writes all twelve,
// hit_store_planes (a batch of views) packs the first four into one and keeps two more.
struct HitWords { uint4 r0, r1, r2; };
// REACH (pwn_trace_reach: tables.h PWN_KM_REACH, the kernel): the walk stops behind the first step that leaves cdist above `reach`, or
// where it returns anyway, and a ray that D -- the distance its record would carry, aux_dist of a sphere, cdist of a wall -- shows
// beyond `reach` gets a PWN_HIT_FREE record read off the step it stopped in: that step's cell, portal count and ray as they were at the
// top of the loop, and the point pos + (reach - cdist) * a of that moment, a = the ray the step advances pos with (in a ramp cell the
// skewed one: WALK_REACH_ADV, trace_walk.inc).  So the loop keeps the top-of-step pos, ray, cdist, cell and portal count, ten registers
// that only these instantiations have; with REACH false none of the names is touched and no instruction is made for them (HITREC's
// rule).  `reach` is only ever compared, subtracted from and multiplied: no bit pattern of it reaches an address or a loop bound.  A NaN
// is never exceeded and +inf neither: the walk, the record and the counters are then pwn_trace_hits'.
#define WALK_REACH_ADV(y) do { if constexpr(REACH) reach_adv_y = (y); } while(0)
template<bool COUNT, bool HAS_W, int LISTS, bool HIDE = false, bool REACH = false>
__device__ __forceinline__ HitWords trace_hit(const Lds &L, Vec<HAS_W> from, Vec<HAS_W> iray, Counters &cnt, [[maybe_unused]] uint32_t hide1 = 0u,
	[[maybe_unused]] float reach = 0.0f)
{
	typedef Vec<HAS_W> V;
	constexpr bool HITREC = true;
	uint32_t hit_cxz;
	int hit_portals = 0;
	V pos = from;
	[[maybe_unused]] float aux_diff = 0.0f;      // (trace_sphere.inc writes the candidate's diffuse factor; nothing here reads it)
	uint32_t aux_idx = 0;
	V aux_pos;
	aux_pos.x = aux_pos.y = aux_pos.z = aux_pos.w = 0.0f;
	//@R p_setup
	// (declared as in trace_pixel: trace_setup.inc writes them, trace_walk.inc walks with them)
	float cdist, fog, aux_dist;
	bool gyp;
	uint32_t cxz, sx, sz, cw;
	float wx, wy, wz;
	int ldy, ldx, ldz;
	V ray;
	float iax, iaz, iay, iay_dn;
	uint32_t iay_up_bits;
	int ldir, ev, base;
	// (REACH: the step's state at the top of the loop)
	[[maybe_unused]] float reach_px, reach_py, reach_pz, reach_rx, reach_ry, reach_rz, reach_cdist, reach_adv_y;
	[[maybe_unused]] uint32_t reach_cxz;
	[[maybe_unused]] int reach_portals;
#include "trace_setup.inc"
	//@R p_walk_ctl
	// (the step limit is carried in ev: trace_pixel)
	ev = -WALK_STEPS;
#pragma unroll 1
	do
	{
		ev++;
		if constexpr(REACH)
		{
			reach_px = pos.x; reach_py = pos.y; reach_pz = pos.z;
			reach_rx = ray.x; reach_ry = ray.y; reach_rz = ray.z;
			reach_cdist = cdist; reach_cxz = cxz; reach_portals = hit_portals;
			reach_adv_y = ray.y;
		}
#include "trace_walk.inc"
		// (behind the step: a portal step adds nothing to cdist, so it ends the walk only for a reach below the set-up's 0)
		if constexpr(REACH) { if(cdist > reach) break; }
	} while(ev < 0);
	asm volatile("" : "+v"(ev));

	//@R p_post
	static_assert(EV_WALL == 1 && EV_SPHERE == 2, "pwnhip.h PWN_HIT_WALL, PWN_HIT_SPHERE");
	static_assert(PWN_HIT_FREE == 3, "the record's kind below");
	uint4 r0, r1, r2;
	// REACH: what the record's dist would be lies beyond the reach -- a walk the stop ended (ev still counts, or is this file's "out of
	// steps" where the last step was the one), a wall met further out in the step that passed the reach, a sphere candidate further out
	bool is_free = false;
	if constexpr(REACH) is_free = (ev == EV_SPHERE ? aux_dist : cdist) > reach;
	if(REACH && is_free)
	{
		// (per lane one subtraction, one product and one sum, each rounded by itself: the Makefile's -ffp-contract=off)
		const float rem = reach - reach_cdist;
		const float fx = reach_px + rem * reach_rx, fy = reach_py + rem * reach_adv_y, fz = reach_pz + rem * reach_rz;
		r0 = make_uint4((uint32_t)PWN_HIT_FREE, 0xffffffffu, 0xffffffffu, (uint32_t)reach_portals);
		r1 = make_uint4(__float_as_uint(reach), __float_as_uint(fx), __float_as_uint(fy), __float_as_uint(fz));
		r2 = make_uint4(__float_as_uint(reach_rx), __float_as_uint(reach_ry), __float_as_uint(reach_rz), reach_cxz);
	}
	else if(ev == EV_OUT_OF_STEPS)
	{
		// trace.h:677: nothing was hit.  face = object = -1, every other field 0
		if(COUNT) cnt.exhausted++;
		r0 = make_uint4(0u, 0xffffffffu, 0xffffffffu, 0u);
		r1 = make_uint4(0u, 0u, 0u, 0u);
		r2 = r1;
	}
	else
	{
		// (the frame kernel's patch of a room's y exit, in front of its shading)
		if(ev == EV_WALL && base == BASE_ROOM_Y) ldir = ldy;
		int object = -1;
		float dist = cdist;
		V at = pos;
		if(ev == EV_SPHERE)
		{
			// which sphere: its byte offset in the blob's sphere array (32 bytes a sphere, in the order of the live table) is what an
			// indexed list holds per entry; an inline record's comes from the "which sphere" array, as trace_shade.inc looks it up
			// (the global form's record index leads to the sphere's index itself, in device memory: tables.h)
			if constexpr(LISTS == PWN_LF_INLINE) aux_idx = L.recsph[(aux_idx - PWN_T_BINIDX) >> 4];
			object = LISTS == PWN_LF_GLOBAL ? (int)L.g_which[aux_idx] : (int)(aux_idx >> 5);
			ldir = -1;
			dist = aux_dist;
			at = aux_pos;
		}
		r0 = make_uint4((uint32_t)ev, (uint32_t)ldir, (uint32_t)object, (uint32_t)hit_portals);
		r1 = make_uint4(__float_as_uint(dist), __float_as_uint(at.x), __float_as_uint(at.y), __float_as_uint(at.z));
		r2 = make_uint4(__float_as_uint(ray.x), __float_as_uint(ray.y), __float_as_uint(ray.z), hit_cxz);
	}
	return HitWords{ r0, r1, r2 };
}
#undef WALK_REACH_ADV

// pwn_trace_hits: the record as it is -- three 16-byte stores (the record is 16-byte aligned: pwn_calls.cpp checks the array)
__device__ __forceinline__ void hit_store_record(const HitWords &h, uint4 *out)
{
	out[0] = h.r0; out[1] = h.r1; out[2] = h.r2;
}

// pwn_trace_view_hits: a pixel's word of each plane that was given (the tests are the same for the whole wave: launch parameters).
//   label   kind | (face + 1) << 2 | (object + 1) << 5 | portals << 19   (pwnhip.h PWN_LABEL_*)
//   cell    the record's word 11;   dist   its word 4
// A segment that ran out of steps has face = object = -1 and every other word 0: all three planes get 0.
// The fields do not run into each other: kind is 0..2, a face 0..5 (ldir of a wall; -1 otherwise), an object an index into the live
// table of at most PWN_OBJ_MAX spheres, and a segment crosses at most one portal per step.
static_assert(EV_SPHERE < 4 && FYN + 1 < 8, "kind in 2 bits, face + 1 in 3");
static_assert(PWN_OBJ_MAX < (1 << 14) - 1, "object + 1 in 14 bits");
static_assert(WALK_STEPS < (1 << 13), "portals in 13 bits");
__device__ __forceinline__ void hit_store_planes(const HitWords &h, uint32_t *label, uint32_t *cell, float *dist)
{
	*label = h.r0.x | ((h.r0.y + 1u) << 2) | ((h.r0.z + 1u) << 5) | (h.r0.w << 19);
	if(cell != NULL) *cell = h.r2.w;
	if(dist != NULL) *dist = __uint_as_float(h.r1.x);
}

// Rounds 1..15 of the add chain of screen.h:12-18 (see the unit loop): in round k the lanes k..15 of every 16-lane row add
// rdx once more, so lane j ends with j adds on top of the row's start value -- the same sequence of fp32 additions for
// every pixel as the reference's "+= rdx" per pixel of the tile.  Written with the execution mask set by hand: a
// v_add_f32 under a mask issues at full rate, the DPP form of the same systolic chain (v[j] = v[j-1] + rdx, round 2) at
// half rate, and this is 45 of a unit's ~170 vector instructions.  All 64 lanes are active on entry (wave-uniform
// control flow); rdx is wave-uniform (kernel argument).
//@R k_chain
#define PWN_CHAIN_ROUND3(m) "s_mov_b32 exec_lo, " m "\n\ts_mov_b32 exec_hi, " m "\n\tv_add_f32 %0, %4, %0\n\tv_add_f32 %1, %5, %1\n\tv_add_f32 %2, %6, %2\n\t"
#define PWN_CHAIN_ROUND4(m) "s_mov_b32 exec_lo, " m "\n\ts_mov_b32 exec_hi, " m "\n\tv_add_f32 %0, %5, %0\n\tv_add_f32 %1, %6, %1\n\tv_add_f32 %2, %7, %2\n\tv_add_f32 %3, %8, %3\n\t"
#define PWN_CHAIN_ALL(R) R("0xfffefffe") R("0xfffcfffc") R("0xfff8fff8") R("0xfff0fff0") R("0xffe0ffe0") R("0xffc0ffc0") R("0xff80ff80") \
	R("0xff00ff00") R("0xfe00fe00") R("0xfc00fc00") R("0xf800f800") R("0xf000f000") R("0xe000e000") R("0xc000c000") R("0x80008000")
template<bool HAS_W> __device__ __forceinline__ void chain_rounds(Vec<HAS_W> &v, const Vec<HAS_W> &rdx)
{
	unsigned long long saved;
	if constexpr(HAS_W)
		asm volatile("s_mov_b64 %4, exec\n\t" PWN_CHAIN_ALL(PWN_CHAIN_ROUND4) "s_mov_b64 exec, %4"
			: "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w), "=&s"(saved) : "s"(rdx.x), "s"(rdx.y), "s"(rdx.z), "s"(rdx.w));
	else
		asm volatile("s_mov_b64 %3, exec\n\t" PWN_CHAIN_ALL(PWN_CHAIN_ROUND3) "s_mov_b64 exec, %3"
			: "+v"(v.x), "+v"(v.y), "+v"(v.z), "=&s"(saved) : "s"(rdx.x), "s"(rdx.y), "s"(rdx.z));
}

// ORDER: the launch writes what every unit cost its wave and / or hands its units out by a table (PWN_OPT_UNIT_ORDER, the
// wave log).  A template parameter, not a test of the two pointers: as dormant code -- two wave-uniform branches and a
// clock read per unit -- it cost launches that do not use it 2.5-3 % (profiles/r4/unit_order_dormant_cost.txt).
// MODE (tables.h PWN_KM_*): what the launch traces.  PWN_KM_FRAME: rows of one frame.  PWN_KM_VIEWS: a batch of P.nviews frames
// of one size (pwn_trace_views): every unit reads its view's camera set-up from P.views and writes that view's planes.
// PWN_KM_RAYS: P.nrays rays of the caller's (pwn_trace_rays): every lane loads its own origin, direction and seed.  PWN_KM_HITS: the
// same batch of rays (pwn_trace_hits), of which every lane traces the primary segment only and writes a first-hit record
// (trace_hit) instead of a colour and a depth.  PWN_KM_VIEWPORTS: P.nvp views of their own sizes, each a frame of its own, into
// rectangles of ONE pitch-P.w frame (pwn_trace_viewports): every unit finds its view and reads that view's set-up, size and
// place from P.vps.  PWN_KM_VIEW_HITS: a batch of views handed out as PWN_KM_VIEWS' (pwn_trace_view_hits), of which every lane traces the
// primary segment only (trace_hit) and writes packed first-hit words to the planes P.hits / sbuf / zbuf (label, cell, distance) instead
// of a colour and a depth.  PWN_KM_VIEWPORT_HITS: views of their own sizes handed out and placed as PWN_KM_VIEWPORTS'
// (pwn_trace_viewport_hits), of which every lane traces the primary segment only and writes the same packed words into ONE plane each
// of the pitch-P.w frame, P.hits / sbuf / zbuf.
// LISTS (tables.h PWN_LF_*): the form of the per-cell sphere lists -- indexed or inline records in LDS, or, for sphere sets whose
// lists outgrow LDS, records in device memory (PWN_LF_GLOBAL).
// HIDE (tables.h PWN_KM_HIDE, a bit of the MODE argument: the names of the kernels without it are as they were, and tests and
// tools/issue_model.py find kernels by name): every view, or every ray, names one sphere of the table that it does not see.
// REACH (tables.h PWN_KM_REACH, a second bit of the MODE argument, valid with PWN_KM_HITS alone): every ray names a distance behind which
// its walk stops.
// Which combinations are instantiated, in which translation unit and under which name (PWN_TRACE_KERNEL_NAME, set by the unit file):
// trace_variants.h, the one table; the host part at the bottom of this file expands it.
#ifndef PWN_TRACE_KERNEL_NAME
#define PWN_TRACE_KERNEL_NAME pwn_trace_kernel
#endif
template<bool COUNT, bool HAS_W, bool ORDER, int LISTS, int MODE_ARG>
__global__ void __launch_bounds__(PWN_BLOCK, PWN_MIN_WAVES)
PWN_TRACE_KERNEL_NAME(pwn_trace_params P)
{
	constexpr int MODE = MODE_ARG & ~(PWN_KM_HIDE | PWN_KM_REACH);
	constexpr bool HIDE = (MODE_ARG & PWN_KM_HIDE) != 0;
	constexpr bool REACH = (MODE_ARG & PWN_KM_REACH) != 0;
	static_assert(!REACH || MODE == PWN_KM_HITS, "REACH: first-hit records of a batch of rays");
	static_assert(!HIDE || (!ORDER && MODE != PWN_KM_FRAME), "HIDE: batches of views, of views of their own sizes and of rays");
	constexpr bool VHITS = MODE == PWN_KM_VIEW_HITS, VIEWS = MODE == PWN_KM_VIEWS || VHITS, HITS = MODE == PWN_KM_HITS, RAYS = MODE == PWN_KM_RAYS || HITS;
	constexpr bool VPHITS = MODE == PWN_KM_VIEWPORT_HITS, VPS = MODE == PWN_KM_VIEWPORTS || VPHITS;
	//@R k_prologue
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

	blob_to_lds(lds_raw, P.blob, P.blob_bytes);
	// one word behind the tables: the workgroup's share of pwn_trace_params.cost_word (bottom of the kernel)
	if(threadIdx.x == 0) *(uint32_t *)(lds_raw + ((P.blob_bytes + 15u) & ~15u)) = 0u;
	__syncthreads();

	// (the tables are addressed from LDS address 0 on, trace_common.h; the launcher checks that this kernel has
	// no static LDS in front of the dynamic allocation)
	const Lds L = LISTS == PWN_LF_GLOBAL ? lds_tables_global(P) : lds_tables(P.off_sph, P.off_recsph);

	typedef Vec<HAS_W> V;
	V rayb, rdx, rdy, from;
	rayb.x = P.rayb[0]; rayb.y = P.rayb[1]; rayb.z = P.rayb[2]; rayb.w = HAS_W ? P.rayb[3] : 0.0f;
	rdx.x = P.rdx[0]; rdx.y = P.rdx[1]; rdx.z = P.rdx[2]; rdx.w = HAS_W ? P.rdx[3] : 0.0f;
	rdy.x = P.rdy[0]; rdy.y = P.rdy[1]; rdy.z = P.rdy[2]; rdy.w = HAS_W ? P.rdy[3] : 0.0f;
	from.x = P.from[0]; from.y = P.from[1]; from.z = P.from[2]; from.w = HAS_W ? P.from[3] : 1.0f;
	float sec_current = P.sec_current;

	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l16 = lane & 15;

	Counters cnt = {};
	// PWN_OPT_WAVE_LOG: when was this wave resident (the GPU's constant 100 MHz clock)
	unsigned long long t_begin = 0ull;
	if(P.wave_log != NULL || P.cost_word != NULL) t_begin = __builtin_amdgcn_s_memrealtime();

	// Work distribution.  A unit is one wave64's 16 x 4 pixels (lane & 15 = column inside one
	// half of the 32-wide tile of screen.h:6-7 = one DPP row, lane >> 4 = row).  Rays differ in
	// cost by an order of magnitude from one part of a frame to another, and with a static split
	// (unit k to wave k mod #waves) the slowest wave ran 1.5x (level.txt) to 2.7x (synth256) as long as
	// the average one: the chip idled a third of the kernel's time.  So waves pull units:
	// PWN_QUEUES counters 128 B apart (same-address atomics serialise at ~4 ns; one counter for a
	// 4K frame's 130 k units would be the bottleneck, as an earlier attempt showed; 8 / 16 / 32 / 64
	// queues measured 0.402 / 0.394 / 0.388 / 0.383 ms at 4K), queue q holds
	// the units u = q (mod PWN_QUEUES); a wave drains its home queue, then helps with the others,
	// and asks for its next unit before it starts on the current one (the ~2 us round trip of
	// the atomic hides behind ~15 us of tracing).  The counters of the NEXT launch of this context
	// are cleared here (launches of a context are stream-ordered, include/pwnhip.h).
	const uint32_t units_x = ((uint32_t)P.w + 15u) >> 4;
	// (a batch of rays: 64 to a unit, P.nrays <= 2^28)
	// (views of their own sizes: the host's sum over the views)
	// Tile pairs (pwn_trace_params.tile_pairs; frames without an order only): the queues hand out whole 32-pixel TILES, and the wave
	// that draws one traces its left half and then its right half (the unit loop).  `units` then counts tiles -- every queue
	// length, QBASE, the help path's test and the host's grid rule with it -- and a draw takes one of them.
	constexpr bool PAIRABLE = MODE == PWN_KM_FRAME && !ORDER;
	const bool pairs = PAIRABLE && P.tile_pairs != 0;
	const uint32_t tiles_x = (units_x + 1u) >> 1;
	// (the setting as the unit loop reads it: 1 or 0, held in a scalar register -- left to itself the compiler keeps it as a lane
	// value next to the unit's column, one register more than the 4-lane variants have)
	uint32_t pair_shift = (uint32_t)__builtin_amdgcn_readfirstlane(pairs ? 1 : 0);
	asm volatile("" : "+s"(pair_shift));
	// The launch's FIRST items stay single units: the units of the first pair_single_rows rows of units in the middle-out order (the
	// host makes that one item per wave of the grid or more).  Those are the static first tickets, started at the launch's first
	// instant on the rows where rays run longest; where one unit is most of a launch (a hall of mirrors walked to the step limit),
	// the wave that holds it must not hold its neighbour as well.  Items [0, pair_first) are those units, the rest are tiles.
	const uint32_t rows_all = ((uint32_t)(P.y1 - P.y0) + 3u) >> 2;
	// (both in scalar registers, as pair_shift below: as lane values they are kept in scratch memory across the unit loop)
	const uint32_t single_rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pairs ? min((uint32_t)P.pair_single_rows, rows_all) : rows_all));
	const uint32_t pair_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(single_rows * units_x));
	const uint32_t units = VPS ? (uint32_t)P.tiles_total : RAYS ? (P.nrays + 63u) >> 6 : (pair_first + tiles_x * (rows_all - single_rows)) * (VIEWS ? (uint32_t)P.nviews : 1u);
	if(blockIdx.x == 0 && threadIdx.x < PWN_QUEUES) P.tickets_next[threadIdx.x * PWN_QUEUE_STRIDE] = 0u;
	if(blockIdx.x == 0 && threadIdx.x == PWN_QUEUES && P.clear_word != NULL) *P.clear_word = 0u;
	uint32_t q = (blockIdx.x * (PWN_BLOCK / 64) + (uint32_t)wave) % PWN_QUEUES;
	uint32_t ticket;
	// The first ticket of a wave is its place among the home waves of its queue: nobody draws it, and the counters
	// hand out the tickets after those (QBASE).  With a drawn first ticket every wave of the grid waits for a
	// returning atomic at the start of the launch, 80 of them per counter at once on a full grid (a draw that a wave
	// waits for costs it 0.7 us on average at 4K and 2.7 us in a strip of an 8-way tiling, tools/r3/draw_probe.py);
	// static first tickets measured +1.3 % at 4K, +2.5 % at 720p, -0.8 % on the strips' kernel time
	// (profiles/r3_strips/static_first.txt).
	const uint32_t nwaves_all = gridDim.x * (PWN_BLOCK / 64);
#define QBASE(qq) ((nwaves_all + PWN_QUEUES - 1u - (qq)) / PWN_QUEUES)
	ticket = (blockIdx.x * (PWN_BLOCK / 64) + (uint32_t)wave) / PWN_QUEUES;
	// A wave that keeps finding queues empty although they looked open stops helping after a
	// few rounds: every queue is drained by its home waves anyway (a wave leaves its home queue
	// only when that is empty), so this costs parallelism at the very end at worst and makes
	// sure every wave's loop ends whatever the loads return.
	int misses = 0;
#ifdef PWN_DRAW_PROBE
	unsigned long long probe_ticks = 0ull, probe_n = 0ull;
#endif
	// (Without tile pairs:) Tickets are drawn two at a time when the launch is long (>= 16 units per wave): the returning atomic is a
	// 32-byte write at the memory side, 4 MB per 4K frame with one per unit, 2 MB with pairs.  Strips and small
	// frames keep single tickets for the balance of their tail; three per draw measured 2.5 % slower at 4K (the
	// tail) for another 0.6 MB.  `left` = tickets in hand after the current one (wave-uniform).
	// (a tile is two units in one ticket: the same commitment and as many returning atomics as a pair of tickets)
	const uint32_t draw_n = !pairs && units >= 16u * (PWN_BLOCK / 64u) * gridDim.x ? 2u : 1u;
	uint32_t left = 0u;
	for(;;)
	{
		//@R k_unit
		// units of queue q: q, q + Q, ...  below `units`
		const uint32_t qlen = (units + PWN_QUEUES - 1u - q) / PWN_QUEUES;
		if(ticket >= qlen)
		{
			//@R k_help
			RG(RG_HELP);
			if(++misses > 2 * (int)PWN_QUEUES) break;
			left = 0u;
			// this queue is empty: find one that is not (plain loads; a stale value can only
			// look fuller than the queue is, and then the atomic below says so)
			uint32_t seen = 0xffffffffu;
			// (the lane number recomputed and made opaque here: otherwise the address and the queue length
			// below are computed once at the top of the kernel and live in scratch memory until this rare
			// block: 20 B per lane written by every wave of every launch, 6.5 MB per 4K frame)
			uint32_t ql = 0u;
			asm volatile("" : "+v"(ql));
			ql = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, ql));     // = lane
			if(ql < PWN_QUEUES)
				seen = __hip_atomic_load(&P.tickets[ql * PWN_QUEUE_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const uint32_t len_l = (units + PWN_QUEUES - 1u - (ql & (PWN_QUEUES - 1u))) / PWN_QUEUES;
			const unsigned long long open = __ballot(ql < PWN_QUEUES && seen < len_l - min(len_l, QBASE(ql & (PWN_QUEUES - 1u))));
			if(open == 0ull) break;
			q = next_open_queue(q, open);
			uint32_t t = 0;
			if(lane == 0) t = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], 1u);
			ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)t) + QBASE(q);
			continue;
		}
		//@R k_unit
		misses = 0;
		// Which unit a ticket stands for: ticket * 64 + q in arithmetic order, or -- PWN_OPT_UNIT_ORDER, off by default -- what
		// the table says: every queue's units sorted by what they cost in the last launch of this geometry, dearest first
		// (pwn_order_kernel), so that the units handed out last are the cheap ones.  The reference's answer to uneven rows
		// is OpenMP's static schedule (screen.h:63-64).  Never changes a pixel: any permutation of the units does.
		// (the 4-lane variant is out of registers: loop-invariant lane values -- the lane number, "am I lane 0" -- end in
		// scratch memory there unless they are made afresh per unit, from mbcnt behind an opaque zero)
		uint32_t ln;
		if constexpr(HAS_W)
		{
			ln = 0u;
			asm volatile("" : "+v"(ln));
			ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, ln));
		}
		else ln = (uint32_t)lane;
		uint32_t unit = ticket * PWN_QUEUES + q;
		// (a SCALAR load: the address is the same for the whole wave, and the scalar cache answers in a fraction of the
		// microsecond a vector load takes here -- every unit waits for this word before it can do anything)
		if(ORDER && P.perm != NULL)
		{
			const uint32_t *pp = P.perm + (uint32_t)__builtin_amdgcn_readfirstlane((int)(q * P.perm_cap + ticket));
			asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(unit) : "s"(pp) : "memory");
		}
		const bool draw = left == 0u;
		// The next unit is asked for BEFORE this one is traced, which commits the wave to two units -- near the end of a
		// launch that is the tail: the last ticket of a queue goes to a wave that still has a whole unit in front of it
		// while its neighbours find the queues empty and leave.  Drawing only when a unit is done, throughout or for the
		// last tickets of a queue, was built and measured in round 3 (profiles/r3_strips/late_draws.txt, commit 5a68fef):
		// slower everywhere (a strip of an 8-way tiling 64 -> 65..77 us, 720p 58 -> 62..75 us, 4K equal), also with the
		// draw issued in front of the unit's colour store.  tools/r3/draw_probe.py times the wait in place: 0.7 us per
		// draw at 4K (4.7 % of a wave's life), 2.7 us in a strip of an 8-way tiling (13.8 %: its 5 120 waves draw
		// in step, 80 per counter), profiles/r3_strips/draw_probe.txt.
		uint32_t next_raw = ticket + 1u;
#ifndef PWN_DRAW_PROBE
		if(draw && ln == 0u) next_raw = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], draw_n) + QBASE(q);
#else
		if(RAYS && draw && ln == 0u) next_raw = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], draw_n) + QBASE(q);      // (the probe is of frames)
#endif
		if constexpr(RAYS)
		{
			// A batch of rays (pwn_trace_rays): unit u is rays [64u, 64u + 64), lane j ray 64u + j, handed out in plain order (the
			// caller's order is the coherence there is: pwn_pixel_rays can lay a frame's pixels out in the units of a frame).  No add
			// chain: every lane loads its ray record -- origin x y z w, direction x y z w, two 16-byte loads -- and its seed.
			//
			// Any bit pattern in any lane (NaN, +-inf, 1e30, a zero direction, an origin far outside the grid) keeps every address in
			// range.  Global: i < nrays <= 2^28 and 64-bit offsets, so rays + 32 i, seeds + 4 i, sbuf + 4 i and zbuf + 4 i lie in the
			// caller's buffers of n entries (pwn_calls.cpp checks n and the alignment).  LDS, in trace_pixel: the ray is never an index
			// by itself.  The table reads take (bits >> 12 or 13) & 2047 of a float (dev_math.h: in range for every bit pattern).  The
			// starting cell is (int)pos, which saturates (NaN converts to 0), pinned to [-16384, 16383] per axis (cxz_pack_start); a
			// walk step moves it by one; the cell word is read at min(c, 64) per axis as unsigned 16-bit fields (cellword_pk: a negative
			// coordinate is a large unsigned one), inside the 65 x 65 table.  Portal, sphere-list and sphere offsets come out of that
			// word and the blob, never out of the ray.  These are the inputs a frame's reflected segments already start from (a
			// bounce off a NaN or far-away hit): the frame path meets them at a few pixels of the hard scenes, every lane here.
			const uint32_t i = unit * 64u + ln;
			if(i < P.nrays)
			{
				const pwn_f4 *rec = (const pwn_f4 *)P.rays + 2u * (size_t)i;
				const pwn_f4 o = rec[0], d = rec[1];
				uint32_t seed = 0u;
				if constexpr(!HITS)
				{
					seed = P.ray_seeds != NULL ? P.ray_seeds[i] : 0u;
					seed <<= 1;                           // the generator runs on the doubled state (lcg2_fs, dev_math.h)
				}
				// (without PWN_RAYS_HAS_W the w lanes are those of an ordinary camera's rays, 1 and 0, whichever variant runs)
				V org, dir;
				org.x = o.x; org.y = o.y; org.z = o.z; org.w = HAS_W && P.ray_w ? o.w : 1.0f;
				dir.x = d.x; dir.y = d.y; dir.z = d.z; dir.w = HAS_W && P.ray_w ? d.w : 0.0f;
				if constexpr(HITS)
				{
					// First-hit records (pwn_trace_hits): the same lane, the same record, the same argument as above for every LDS address --
					// trace_hit runs trace_pixel's set-up and walk texts and reads one more table, the inline lists' "which sphere" array,
					// at the index trace_shade.inc reads it at (aux_idx is a list record's LDS address, written by the walk from the cell
					// word's list offset; never the ray's; in the lists' global form a record's index in device memory, which the walk counts up
					// from the cell's liststart entry to the record with the end mark: inside the nrec records the host packed).
					// Global: hits + 48 i for i < nrays <= 2^28 in 64-bit arithmetic lies in the
					// caller's array of n records; a lane with i >= nrays stores nothing.  No seed, colour or depth is touched.
					// HIDE: the ray's hidden sphere, ray_hide[i] for i < nrays in the caller's array of n int32 (pwn_calls.cpp checks it), as
					// k + 1 (WALK_HIDDEN: only ever compared)
					// REACH (pwn_trace_reach): the ray's reach, ray_reach[i] for i < nrays in the caller's array of n floats (pwn_reach.cpp checks
					// it): only ever compared and multiplied (trace_hit)
					if constexpr(REACH)
					{
						uint32_t hide1 = 0u;
						if constexpr(HIDE) hide1 = (uint32_t)P.ray_hide[i] + 1u;
						const HitWords hw = trace_hit<COUNT, HAS_W, LISTS, HIDE, true>(L, org, dir, cnt, hide1, P.ray_reach[i]);
						// (the record's address is made behind the walk, as the HIDE kernels' below)
						uint32_t il = i;
						asm volatile("" : "+v"(il));
						hit_store_record(hw, (uint4 *)((unsigned char *)P.hits + (size_t)il * PWN_HIT_REC_BYTES));
					}
					else if constexpr(HIDE)
					{
						const uint32_t hide1 = (uint32_t)P.ray_hide[i] + 1u;
						const HitWords hw = trace_hit<COUNT, HAS_W, LISTS, true>(L, org, dir, cnt, hide1);
						// (the record's address is made behind the walk, from the ray's number: one register across the walk where the
						// address is two, which is the register hide1 takes)
						uint32_t il = i;
						asm volatile("" : "+v"(il));
						hit_store_record(hw, (uint4 *)((unsigned char *)P.hits + (size_t)il * PWN_HIT_REC_BYTES));
					}
					else
					{
						uint4 *const out = (uint4 *)((unsigned char *)P.hits + (size_t)i * PWN_HIT_REC_BYTES);
						hit_store_record(trace_hit<COUNT, HAS_W, LISTS>(L, org, dir, cnt), out);
					}
				}
				else
				{
					float ox, oy, oz, ow;
					// HIDE (pwn_trace_rays_hide_device): the ray's hidden sphere as the first-hit records' above -- ray_hide[i] for i < nrays,
					// the RAY's index, in the caller's array of n int32, as k + 1 (WALK_HIDDEN: only ever compared)
					if constexpr(HIDE) trace_pixel<COUNT, HAS_W, LISTS, true>(L, sec_current, seed, org, dir, ox, oy, oz, ow, P.zbuf + i, cnt, (uint32_t)P.ray_hide[i] + 1u);
					else trace_pixel<COUNT, HAS_W, LISTS>(L, sec_current, seed, org, dir, ox, oy, oz, ow, P.zbuf + i, cnt);
					P.sbuf[i] = col_pack4(ox, oy, oz, ow);
				}
			}
			ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_raw);
			left = draw ? draw_n - 1u : left - 1u;
			continue;
		}
		// rows from the middle outwards: the horizon band, where rays run longest,
		// is started first and the cheap top and bottom edges make up the tail
		// (this arithmetic is the same for the whole wave, but the compiler does it per lane because q starts
		// from the wave number, which it derives from threadIdx.  Declaring q uniform and dividing by a multiply-high
		// with a host-computed reciprocal moves ~35 VALU instructions per unit to the scalar unit: measured 0.8 %
		// SLOWER at 4K, three runs -- a wave's scalar instructions issue one at a time and in order)
		// unit / units_x by the host's reciprocal (pwn_trace_params.ux_magic: exact for every unit < 2^31, launch_plan.h
		// pwn_unit_div_magic): two instructions where the compiler's division takes thirteen; frames one unit wide divide
		// A batch of views: the units are handed out INTERLEAVED, unit = (unit of the frame) * nviews + view, so that the first
		// tickets of the launch cover every view's middle rows and each view's rows go out middle-out as one frame's do -- the
		// expensive horizon bands of all views are started first and the cheap edges of all views make up the tail.  (View-major
		// order would leave the tail to the last views' horizon bands.)  Any order gives the same pixels.  The view number is the
		// same for the whole wave: its record comes in by scalar loads (constant address space, read-only).
		uint32_t fu = unit;
		uint32_t *sbuf = P.sbuf;
		float *zbuf = P.zbuf;
		[[maybe_unused]] size_t vh_base = 0;              // (first-hit planes: where the view's planes begin, in words)
		[[maybe_unused]] uint32_t hide1 = 0u;             // (HIDE: the view's hidden sphere, WALK_HIDDEN)
		if constexpr(VIEWS)
		{
			fu = P.views_shift >= 0 ? __umulhi(unit, P.views_magic) >> P.views_shift : unit;
			const uint32_t view = (uint32_t)__builtin_amdgcn_readfirstlane((int)(unit - fu * (uint32_t)P.nviews));
			typedef const __attribute__((address_space(4))) float cfloat;
			const cfloat *r = (const cfloat *)((uintptr_t)P.views + (uintptr_t)view * PWN_VIEWS_REC_BYTES);
			rayb.x = r[0]; rayb.y = r[1]; rayb.z = r[2]; rayb.w = HAS_W ? r[3] : 0.0f;
			rdx.x = r[4]; rdx.y = r[5]; rdx.z = r[6]; rdx.w = HAS_W ? r[7] : 0.0f;
			rdy.x = r[8]; rdy.y = r[9]; rdy.z = r[10]; rdy.w = HAS_W ? r[11] : 0.0f;
			from.x = r[12]; from.y = r[13]; from.z = r[14]; from.w = HAS_W ? r[15] : 1.0f;
			// (the record's `hide` word, with the rest of the record: one scalar load, one value for the wave)
			if constexpr(HIDE) hide1 = ((const __attribute__((address_space(4))) uint32_t *)r)[17];
			// (the view's planes: 64-bit offsets, a batch may hold 2^28 pixels per plane array)
			if constexpr(VHITS) vh_base = (size_t)view * (size_t)P.plane;
			else
			{
				sec_current = r[16];
				sbuf += (size_t)view * (size_t)P.plane;
				zbuf += (size_t)view * (size_t)P.plane;
			}
		}
		// The frame this unit belongs to: the launch's -- or, views of their own sizes (pwn_trace_viewports), the view's own, from
		// its record: width and height (bounds, pixel seed, middle row), units per row with their division constant, rows of
		// units, and `org`, where the view's pixel (0, 0) lies in the pitch-P.w planes.  x and y below are LOCAL to the view, so
		// the 32-pixel add chain starts at the view's column 0 and the seed is that of a frame fw wide; only the store adds org.
		int fw = P.w, fh = P.h, fy0 = P.y0, fy1 = P.y1;
		uint32_t fux = units_x, fmagic = P.ux_magic;
		int fshift = P.ux_shift;
		// (tile pairs: behind the launch's single units the ticket stands for a tile, rows of tiles_x of them behind the single rows)
		// (the unit number is the same for the whole wave: the choice is a scalar one)
		uint32_t kbase = 0u, ush = 0u;
		if(PAIRABLE && pair_shift != 0u && (uint32_t)__builtin_amdgcn_readfirstlane((int)unit) >= pair_first) { fu -= pair_first; fux = tiles_x; fmagic = P.tx_magic; fshift = P.tx_shift; kbase = single_rows; ush = 1u; }
		uint32_t rows_u = ((uint32_t)(P.y1 - P.y0) + 3u) >> 2;
		uint32_t org = 0u;
		if constexpr(VPS)
		{
			// Which view, which of its units (tables.h pwn_viewport_rec): the launch goes in rounds -- round r = unit r of every
			// view that has more than r -- so ticket t lies in the segment s with the largest seg_first <= t, is the
			// (t - seg_first) mod (nvp - s)-th of the views s .. nvp-1 there and that view's unit seg_round + (t - seg_first) / (nvp - s),
			// which is below the view's units because the records are in order of rising units.  All of it is the same for the
			// whole wave: scalar arithmetic and scalar loads from the constant address space (read-only), at most ten steps of
			// the search for PWN_VIEWS_MAX views.  Any order gives the same pixels.
			typedef const __attribute__((address_space(4))) uint32_t cu32;
			typedef const __attribute__((address_space(4))) float cfloat;
			const uintptr_t base = (uintptr_t)P.vps;
			const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)unit), nvp = (uint32_t)P.nvp;
			uint32_t s = 0u;
			for(uint32_t step = P.vp_step0; step != 0u; step >>= 1)
			{
				const uint32_t c = min(s + step, nvp - 1u);
				const uint32_t first = ((cu32 *)(base + (uintptr_t)c * PWN_VP_REC_BYTES))[26];
				if(s + step < nvp && first <= t) s += step;
			}
			cu32 *sr = (cu32 *)(base + (uintptr_t)s * PWN_VP_REC_BYTES);
			const uint32_t d = t - sr[26], cnt = nvp - s;
			const int sshift = (int)sr[29];
			const uint32_t rr = sshift >= 0 ? __umulhi(d, sr[28]) >> sshift : d;
			const uint32_t view = s + (d - rr * cnt);
			fu = sr[27] + rr;
			cu32 *ri = (cu32 *)(base + (uintptr_t)view * PWN_VP_REC_BYTES);
			const cfloat *r = (const cfloat *)ri;
			rayb.x = r[0]; rayb.y = r[1]; rayb.z = r[2]; rayb.w = HAS_W ? r[3] : 0.0f;
			rdx.x = r[4]; rdx.y = r[5]; rdx.z = r[6]; rdx.w = HAS_W ? r[7] : 0.0f;
			rdy.x = r[8]; rdy.y = r[9]; rdy.z = r[10]; rdy.w = HAS_W ? r[11] : 0.0f;
			from.x = r[12]; from.y = r[13]; from.z = r[14]; from.w = HAS_W ? r[15] : 1.0f;
			if constexpr(!VPHITS) sec_current = r[16];        // (first-hit planes read no time)
			fw = (int)ri[19]; fh = (int)ri[20]; fy0 = 0; fy1 = fh;
			fux = ri[21]; fmagic = ri[22]; fshift = (int)ri[23]; rows_u = ri[24];
			// (the record's `hide` word, with the rest of the record: one scalar load, one value for the wave)
			if constexpr(HIDE) hide1 = ri[30];
			// (the rectangle lies inside the w x h <= 2^30 pixels of the planes: pwn_viewports_plan)
			org = ri[18] * (uint32_t)P.w + ri[17];
		}
		uint32_t k;
		// (ux_shift < 0 only for units_x == 1, launch_plan.h pwn_unit_div_magic: then k = unit.  A real division here had its
		// reciprocal hoisted to the top of the kernel and, in the 4-lane variant, parked in scratch memory)
		if(fshift >= 0) k = __umulhi(fu, fmagic) >> fshift;
		else k = fu;
		// (tile pairs: the tile's left unit)
		const uint32_t ux = (fu - k * fux) << (PAIRABLE ? ush : 0u);
		if(PAIRABLE) k += kbase;
		// ... of the FRAME: a strip of a row tiling starts at its rows nearest the frame's middle row (the strip of
		// the whole frame at its own middle), not at its own middle
		const int hrow = ((fh >> 1) - fy0) >> 2;
		const uint32_t mid = (uint32_t)min(max(hrow, 0), (int)rows_u - 1);
		// k = 0,1,2,3,... -> mid, mid-1, mid+1, mid-2, ... while there are rows on both sides (a above, b below),
		// then the rest of the longer side in order
		uint32_t uy;
		{
			const uint32_t a = mid, b = rows_u - 1u - mid, m = min(a, b);
			const uint32_t j = (k + 1u) >> 1;
			if(k <= 2u * m) uy = (k & 1u) ? mid - j : mid + j;
			else uy = a > b ? mid - (k - b) : mid + (k - a);
		}
		const int half = (int)(ux & 1u);                  // left / right half of the 32-wide tile
		const int cx0 = (int)(ux >> 1) * 32;              // the 32-pixel tile of screen.h:6-7 this wave is in
		// (this unit's pixel: ux * 16 + lane & 15, fy0 + uy * 4 + lane >> 4 -- below, with what the tile's other half takes over)

		// screen.h:12-18, in the order the reference build evaluates it:
		// rayl = (cx*rdx + rayb) + y*rdy, then one "+= rdx" per pixel of the
		// 32-wide tile up to and including this one.  The chain is sequential
		// in fp32, but every pixel of a row walks the SAME chain, so the lanes of
		// a DPP row build it systolically: after k rounds of
		//     v[j] = v[j-1] + rdx      (lane 0 of the row keeps its value)
		// lanes 0..k hold their final value.  All 64 lanes take part (also those
		// outside the frame), so this sits in front of the bounds test.
		V rayl = vadd<HAS_W>(vadd<HAS_W>(vscale<HAS_W>((float)cx0, rdx), rayb), vscale<HAS_W>((float)(fy0 + (int)uy * 4 + (HAS_W ? (int)(ln >> 4) : (lane >> 4))), rdy));
		if(half)
		{
			//@R k_unit_half
			RG(RG_UNIT_HALF);
#pragma unroll
			for(int k = 0; k < 16; k++) rayl = vadd<HAS_W>(rayl, rdx);
		}
		// Tile pairs: the tile's right half starts its chain where the left half's lane 15 of the same row ended -- base + 16 adds, the
		// same fp32 additions from the same base that `if(half)` above makes -- and shares the tile's rows and columns.  What it needs is
		// put aside behind the left half's chain in the lanes of ONE register (`carry`: lane 4c + r = component c of row r's lane 15;
		// lane 16 and up = the tile's column and the unit's top row, 15 bits each), through the LDS crossbar (ds_bpermute: no LDS
		// memory), because nothing else is free while a unit is traced: the kernel is at its register budget and the scalar registers
		// already spill into lanes.  Both halves run the ONE text below (the chain, the bounds test, the trace, the stores).
		float carry = 0.0f;
		int x = (int)ux * 16 + (HAS_W ? (int)(ln & 15u) : l16), y = fy0 + (int)uy * 4 + (HAS_W ? (int)(ln >> 4) : (lane >> 4));
		// (is there a right half: a frame with an odd number of units per row ends its rows with half a tile)
		bool right_next = PAIRABLE && ush != 0u && (uint32_t)__builtin_amdgcn_readfirstlane((int)ux) + 1u < units_x;
		unsigned long long u_begin = 0ull;
#pragma unroll 1
		for(;;)
		{
			//@R k_chain
			RG(RG_UNIT);
			rayl = vadd<HAS_W>(rayl, rdx);
			chain_rounds<HAS_W>(rayl, rdx);
			if(PAIRABLE && right_next)
			{
				//@R k_unit
				uint32_t lp;
				if constexpr(HAS_W)
				{
					lp = 0u;
					asm volatile("" : "+v"(lp));
					lp = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, lp));
				}
				else lp = (uint32_t)lane;
				const int src = (int)(((lp & 3u) << 6) | 60u);            // byte address of lane 16 r + 15, r = lane & 3
				const int px = __builtin_amdgcn_ds_bpermute(src, __float_as_int(rayl.x));
				const int py = __builtin_amdgcn_ds_bpermute(src, __float_as_int(rayl.y));
				const int pz = __builtin_amdgcn_ds_bpermute(src, __float_as_int(rayl.z));
				int pc = lp < 4u ? px : lp < 8u ? py : pz;
				if constexpr(HAS_W)
				{
					const int pw = __builtin_amdgcn_ds_bpermute(src, __float_as_int(rayl.w));
					pc = lp < 12u ? pc : pw;
				}
				// (x and y are the left half's here: x - column in the half = the tile's first column, y - row in the unit = the top row)
				const int xy = (x - (int)(lp & 15u)) | ((y - (int)(lp >> 4)) << 16);
				carry = __int_as_float(lp < 16u ? pc : xy);
			}
			//@R k_chain
			if(ORDER && P.unit_cost != NULL) u_begin = __builtin_amdgcn_s_memrealtime();
			if constexpr(VHITS)
			{
				// First-hit planes (pwn_trace_view_hits): the pixel's ray as a frame's, through trace_hit in the place of trace_pixel.  Every
				// LDS address: the argument of the hit mode above (trace_hit's set-up and walk are trace_pixel's, and the ray is a frame's,
				// which the frame modes trace).  Global: only lanes with x < w and y < h store, one 4-byte word per plane given, at
				// view * plane + y * w + x with view < nviews and plane = w * h: below nviews * w * h <= 2^28 words, in 64-bit arithmetic,
				// inside planes of that many words (pwn_calls.cpp checks n and allocates the host form's own).  A plane whose pointer is
				// NULL is skipped.  No seed, colour, depth or time is touched.
				if(x < fw && y < fy1)
				{
					const size_t o = vh_base + (size_t)y * (size_t)P.w + (size_t)x;
					// (tables.h: the label plane is P.hits, the cell plane P.sbuf, the distance plane P.zbuf)
					hit_store_planes(trace_hit<COUNT, HAS_W, LISTS, HIDE>(L, from, rayl, cnt, hide1), (uint32_t *)P.hits + o, P.sbuf != NULL ? P.sbuf + o : NULL, P.zbuf != NULL ? P.zbuf + o : NULL);
				}
			}
			else if constexpr(VPHITS)
			{
				// First-hit planes of views of their own sizes (pwn_trace_viewport_hits): the viewports mode up to here -- the view's record,
				// its frame, x and y LOCAL to the view -- then trace_hit in the place of trace_pixel, as the mode above.  Every LDS address
				// comes from trace_hit: the argument of the hit mode (its set-up and walk are trace_pixel's, and the ray is a frame's).
				// Global: only lanes with x < fw and y < fh store (fy1 = fh here), one 4-byte word per plane given, at org + y * P.w + x
				// with org = rec.y * P.w + rec.x; the rectangle lies inside the P.w x P.h <= 2^30 words of a plane (pwn_viewports_plan, by
				// which every record was admitted), so (rec.y + y) * P.w + rec.x + x < P.w * P.h fits 32 bits and lies inside a plane of
				// P.w x P.h words.  A plane whose pointer is NULL is skipped.  No seed, colour, depth or time is touched.
				if(x < fw && y < fy1)
				{
					const uint32_t o = __umul24((uint32_t)y, (uint32_t)P.w) + (uint32_t)x + org;      // w, h <= 32768
					// (tables.h: the label plane is P.hits, the cell plane P.sbuf, the distance plane P.zbuf)
					hit_store_planes(trace_hit<COUNT, HAS_W, LISTS, HIDE>(L, from, rayl, cnt, hide1), (uint32_t *)P.hits + o, P.sbuf != NULL ? P.sbuf + o : NULL, P.zbuf != NULL ? P.zbuf + o : NULL);
				}
			}
			else if(x < fw && y < fy1)
			{
				const uint32_t seed = pixel_seed(x, y, fw);
				float ox, oy, oz, ow;
				const uint32_t o = __umul24((uint32_t)y, (uint32_t)P.w) + (uint32_t)x + org;      // w, h <= 32768 (pwn_init)
				trace_pixel<COUNT, HAS_W, LISTS, HIDE>(L, sec_current, seed, from, rayl, ox, oy, oz, ow, zbuf + o, cnt, hide1);
				sbuf[o] = col_pack4(ox, oy, oz, ow);
			}
			if(!(PAIRABLE && right_next)) break;
			//@R k_unit_right
			// The right half: its lanes' rows' rays from `carry`, its pixels 16 to the right of the left half's.  All 64 lanes are
			// active again here, and the lanes of `carry` that are read were written by active lanes.
			RG(RG_UNIT_RIGHT);
			right_next = false;
			{
				uint32_t lp;
				if constexpr(HAS_W)
				{
					lp = 0u;
					asm volatile("" : "+v"(lp));
					lp = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, lp));
				}
				else lp = (uint32_t)lane;
				const int ci = __float_as_int(carry);
				const int dst = (int)((lp >> 4) << 2);                    // byte address of lane r, r = the lane's row
				rayl.x = __int_as_float(__builtin_amdgcn_ds_bpermute(dst, ci));
				rayl.y = __int_as_float(__builtin_amdgcn_ds_bpermute(dst + 16, ci));
				rayl.z = __int_as_float(__builtin_amdgcn_ds_bpermute(dst + 32, ci));
				if constexpr(HAS_W) rayl.w = __int_as_float(__builtin_amdgcn_ds_bpermute(dst + 48, ci));
				const int xy = __builtin_amdgcn_readlane(ci, 16);
				x = (xy & 0xffff) + 16 + (int)(lp & 15u);
				y = (xy >> 16) + (int)(lp >> 4);
			}
		}
		// what this unit cost its wave (the add chain and the ticket arithmetic in front of it are the same for every unit)
		if(ORDER && P.unit_cost != NULL && ln == 0u)
		{
			const unsigned long long d = (__builtin_amdgcn_s_memrealtime() - u_begin) >> 2;
			P.unit_cost[unit] = (uint16_t)(d > 65535ull ? 65535ull : d);
		}
#ifdef PWN_DRAW_PROBE
		// experiment build (tools/r3/draw_probe.py): the draw AFTER the unit, and how long the wave waits for it
		{
			const unsigned long long p0 = __builtin_amdgcn_s_memrealtime();
			if(draw && lane == 0) next_raw = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], draw_n) + QBASE(q);
			ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_raw);
			asm volatile("" : "+s"(ticket));
			probe_ticks += __builtin_amdgcn_s_memrealtime() - p0;
			probe_n++;
		}
#else
		ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_raw);
#endif
		left = draw ? draw_n - 1u : left - 1u;
	}

	//@R k_epilogue
	if(COUNT)
	{
		// (the issue model's region counts go behind the first 16)
#define PWN_CNT_REGIONS RG_N
#include "trace_counters.inc"
#undef PWN_CNT_REGIONS
		// (waves of this launch: the prologue and the epilogue of the issue model)
		if(lane == 0) atomicAdd(&P.counters[16 + RG_N], 1ull);
	}
	// PWN_OPT_WAVE_LOG: every wave's lifetime
	if(P.wave_log != NULL && wave_first_lane())
	{
		unsigned long long *wl = wave_log_slot(P.wave_log);
#ifdef PWN_DRAW_PROBE
		wl[0] = probe_ticks | (probe_n << 40); wl[1] = __builtin_amdgcn_s_memrealtime() - t_begin;
#else
		wl[0] = t_begin; wl[1] = __builtin_amdgcn_s_memrealtime();
#endif
	}
	// Row tiling with moving cuts (pwn_tiled.cpp): what this strip COST, as the sum of its waves' lifetimes in ticks of
	// the constant 100 MHz clock -- a wave lives exactly as long as it finds units, so the sum is the strip's work
	// in wave-time, whatever the tail of the launch looked like.  The four waves of a workgroup add up in LDS (one
	// ds_add_rtn: lifetime in the low 28 bits, a count in the high four) and the last one to leave adds the
	// workgroup's sum to the word: ~1300 no-return atomics per launch, spread over its tail.
	if(P.cost_word != NULL && wave_first_lane())
	{
		static_assert(PWN_BLOCK == 256, "four waves per workgroup");
		const uint32_t life = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_begin) & 0x03ffffffu;
		PWN_LDS uint32_t *wg = (PWN_LDS uint32_t *)(uintptr_t)((P.blob_bytes + 15u) & ~15u);
		const uint32_t old = __hip_atomic_fetch_add(wg, life + (1u << 28), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		if((old >> 28) == 3u) (void)__hip_atomic_fetch_add(P.cost_word, (old + life) & 0x0fffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// (ORDER, LISTS, MODE) -> the four kernels a launch's count and has_w pick from (trace_common.h)
template<bool ORDER, int LISTS, int MODE>
using Units = TraceKernels<PWN_TRACE_KERNEL_NAME<true, true, ORDER, LISTS, MODE>, PWN_TRACE_KERNEL_NAME<true, false, ORDER, LISTS, MODE>,
	PWN_TRACE_KERNEL_NAME<false, true, ORDER, LISTS, MODE>, PWN_TRACE_KERNEL_NAME<false, false, ORDER, LISTS, MODE>>;

// The host part.  The unit file that includes this text says which unit of trace_variants.h it is (PWN_TRACE_UNIT; this file by
// itself is MAIN) and compiles that unit's rows of the table: one function that launches them, whose uses of Units<> are what
// instantiates the unit's kernels -- templates are instantiated where they are used, so no unit compiles another's.
#include "trace_variants.h"
#ifndef PWN_TRACE_UNIT
#define PWN_TRACE_UNIT MAIN
#define PWN_TRACE_MAIN_UNIT
#endif

// One row: its kernels over the (ORDER, LISTS) the table gives every row, and those it gives the rows with ORDER variants.  Anything
// else is no kernel, and a missing kernel is an error.
template<int MODE, bool HAS_ORDER>
static hipError_t launch_row(int lists, bool order, const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream)
{
#define PWN_FORM(ORDER, LISTS) if(order == ORDER && lists == LISTS) return Units<ORDER, LISTS, MODE>::launch(P, grid, lds_bytes, count, stream);
#define PWN_FORM_ORDER(ORDER, LISTS) if constexpr(HAS_ORDER) PWN_FORM(ORDER, LISTS)
	PWN_TRACE_ROW_FORMS(PWN_FORM, PWN_FORM_ORDER)
#undef PWN_FORM
#undef PWN_FORM_ORDER
	return hipErrorInvalidValue;
}
extern "C" hipError_t PWN_TRACE_UNIT_LAUNCH(PWN_TRACE_UNIT)(int mode, int lists, bool order, const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream)
{
	switch(mode)
	{
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) case (MODE): return launch_row<(MODE), HAS_ORDER>(lists, order, P, grid, lds_bytes, count, stream);
	PWN_TRACE_UNIT_VARIANTS(PWN_TRACE_UNIT)(PWN_ROW)
#undef PWN_ROW
	}
	return hipErrorInvalidValue;
}

#ifdef PWN_TRACE_MAIN_UNIT
// The launcher: the unit that holds the mode's row launches it.  A mode without a row is no kernel.
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) extern "C" hipError_t PWN_TRACE_UNIT_LAUNCH(UNIT)(int, int, bool, const pwn_trace_params *, int, size_t, bool, hipStream_t);
PWN_TRACE_VARIANTS(PWN_ROW)
#undef PWN_ROW
extern "C" hipError_t pwn_launch_trace(int mode, int lists, bool order, const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream)
{
	switch(mode)
	{
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) case (MODE): return PWN_TRACE_UNIT_LAUNCH(UNIT)(mode, lists, order, P, grid, lds_bytes, count, stream);
	PWN_TRACE_VARIANTS(PWN_ROW)
#undef PWN_ROW
	}
	return hipErrorInvalidValue;
}

extern "C" int pwn_trace_tile_h(void) { return TILE_H; }
extern "C" int pwn_trace_tile_w(void) { return TILE_W; }
// LDS a workgroup needs beyond the table blob
extern "C" unsigned pwn_trace_lds_extra(void)
{
	return 16u;        // the workgroup's cost word (pwn_trace_params.cost_word)
}

// resident 256-thread workgroups per CU for this variant and LDS size
extern "C" int pwn_trace_blocks_per_cu(size_t lds_bytes, bool count, bool has_w)
{
	return Units<false, PWN_LF_INDEXED, PWN_KM_FRAME>::blocks_per_cu(lds_bytes, count, has_w);
}
// ... for the variants that read the lists from device memory
extern "C" int pwn_trace_global_blocks_per_cu(size_t lds_bytes, bool count, bool has_w)
{
	return Units<false, PWN_LF_GLOBAL, PWN_KM_FRAME>::blocks_per_cu(lds_bytes, count, has_w);
}
#endif
