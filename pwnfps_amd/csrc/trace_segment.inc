// trace_segment.inc -- one ray segment of trace_pixel (trace_kernel.hip): set-up, walk, shading and, where the ray goes on, the
// bounce, the jitter and the composite stack's new entry.  Textually included once per bounce depth, with PWN_SEG = 0, 1, ...
// REFLECT_MAX a constant of the preprocessor's: the copies are different programs.
//   - Copy 0 is the only one that writes the depth plane, and the colour it is lit with (icol, screen.h:24) is the constant 1, 1, 1.
//   - A copy's composite-stack entry is a set of names of its own (PWN_SEG_ST: copy 0 writes A, copy 1 writes B): nothing is
//     shifted, and the colour the next copy is lit with (trace.h:90) is that entry's.
//   - The last copy can never bounce: the mirror's effect on the ray apart, nothing that only a bounce reads is made there -- no
//     floor normal, no sphere reflection, no jitter, no stack entry.
// A lane whose ray ends here sets `depth` to the copy's number and leaves for trace_pixel's ray_done; the others fall out of the
// bottom into the next copy.
// Names it uses from the including scope:
//   L (Lds), COUNT, HAS_W, LISTS, HIDE, V, cnt;  sec_current, seed, zpix, hide1;  carried from copy to copy: pos, iray, w_acc and the
//   sphere candidate (aux_*);  the entries stA_*, scA*, stB_*, scB*.
// Names it writes: vx, vy, vz, vw, depth for a lane that leaves;  pos, iray, seed and its entry for one that goes on.
// Line numbers: copy d's lines are numbered d * 1000 + the line in this file (the #line directives below), so that the line tables
// of a build say which copy an instruction belongs to (tools/issue_model.py region_of_copy; it checks the directives against the
// file).  Nothing but line tables and diagnostics reads them.
#if PWN_SEG == 0
#define icx 1.0f
#define icy 1.0f
#define icz 1.0f
#define PWN_SEG_ST(refl_, fog_, x_, y_, z_) do { stA_refl = (refl_); stA_fog = (fog_); scAx = (x_); scAy = (y_); scAz = (z_); } while(0)
#elif PWN_SEG == 1
#define icx scAx
#define icy scAy
#define icz scAz
#define PWN_SEG_ST(refl_, fog_, x_, y_, z_) do { stB_refl = (refl_); stB_fog = (fog_); scBx = (x_); scBy = (y_); scBz = (z_); } while(0)
#line 1029
#elif PWN_SEG == 2
#define icx scBx
#define icy scBy
#define icz scBz
#line 2034
#else
#error "trace_segment.inc: a copy per bounce depth, REFLECT_MAX = 2 (trace_common.h)"
#endif
{
	//@R p_setup
	RG(RG_SEG);
#if PWN_SEG == 1
	RG(RG_SEG1);
#elif PWN_SEG == 2
	RG(RG_SEG2);
#endif
	// ------------------------------------------------ trace.h:186-248 (trace_setup.inc)
	// the segment's ray and what the walk keeps of it.  Declared here, without values, because the set-up's text is shared
	// with the refill kernel, where they outlive the segment.  The ORDER of these declarations is that of the set-up's
	// first writes and is not a matter of style: in another order the compiler numbers registers differently.
	float cdist, fog, aux_dist;
	bool gyp;
	uint32_t cxz, sx, sz, cw;
	float wx, wy, wz;
	int ldy, ldx, ldz;
	V ray;
	float iax, iaz, iay, iay_dn;
	uint32_t iay_up_bits;
	int ldir, ev, base;
#include "trace_setup.inc"

	// ------------------------------------------------ trace.h:250-675 (trace_walk.inc)
	//@R p_walk_ctl
	// How the walk loop ends: ev is the step count and the event in one register.  It starts a segment at -WALK_STEPS, is counted up
	// at the top of every iteration, and a step without an event leaves it as it is (trace_walk.inc WALK_EV_KEEP: the room body's two
	// selects -- sphere hit / floor-ceiling / neither); the loop runs while ev < 0, one compare.  A lane that leaves with ev == 0 has made
	// WALK_STEPS steps without an event: out of steps (trace.h:250,677); an event in the last step still wins.  The limit in a counter
	// of its own, folded into ev at the bottom, was three more VALU and one more scalar instruction per step
	// (profiles/walk_exit/ab.txt, with both latches as compiled).
	// Two other forms were built and measured in round 3 (profiles/r3_walk_exit.txt; the code is in commit 2b36426):
	// the step limit as a scalar count with a branch of its own (-3 VALU, +2 scalar per step: +3.9 % time at 4K), and a
	// lane mask `done` = hit || ymin with WHICH of the two read off cdist against aux_dist after the walk (-4 VALU,
	// +10 scalar mask instructions per step as compiled: +5.3 %).  Scalar instructions are not free here.
	ev = -WALK_STEPS;
#pragma unroll 1
	do
	{
		ev++;
#if PWN_SEG == 1
		RG(RG_WSTEPS1);
#elif PWN_SEG == 2
		RG(RG_WSTEPS2);
#endif
#include "trace_walk.inc"
	} while(ev < 0);
	// what the ray ended on is read back from the register: without this the compiler keeps
	// "ev == EV_OUT_OF_STEPS" as a lane mask that it updates in every iteration of the walk
	// (5 of ~85 instructions per step)
	asm volatile("" : "+v"(ev));

	//@R p_post
	if(ev == EV_OUT_OF_STEPS)
	{
		//@R p_exhausted
		RG(RG_EXHAUSTED);
		// trace.h:677-678: out of steps -- the walked ray is the colour
		if(COUNT) cnt.exhausted++;
		vx = ray.x; vy = ray.y; vz = ray.z; vw = HAS_W ? ray.w : 0.0f;
		depth = PWN_SEG;
		goto ray_done;
	}
	//@R p_post
	if(ev == EV_WALL && base == BASE_ROOM_Y) { ldir = ldy; base = (gyp ? BASE_CEIL : BASE_FLOOR); }
#if PWN_SEG == 0
	// zbuf = the PRIMARY ray's hit distance (trace.h:102-105); a primary ray that ran out of steps
	// leaves the old depth in place (trace.h:677)
	*zpix = (ev == EV_SPHERE ? aux_dist : cdist);
#endif

	// (the segment's colour is computed into the pixel's own registers: a segment that ends the ray has nothing to copy)
	float refl;
#define colx vx
#define coly vy
#define colz vz
	// trace.h:108-154 / 283-291: the wall's or the sphere's colour, the ray mirrored at a wall
#include "trace_shade.inc"

	//@R p_post
	// trace.h:3-7
#if PWN_SEG >= REFLECT_MAX
	(void)refl;
	vw = 0.0f; depth = PWN_SEG;
	goto ray_done;
#else
	if(refl == 0.0f) { vw = 0.0f; depth = PWN_SEG; goto ray_done; }

	// trace.h:9-84: off the rippled floor or a sphere, then the jitter (straight into the next segment's direction)
#include "trace_bounce.inc"
#include "trace_jitter.inc"

	//@R p_jitter
	PWN_SEG_ST(refl, fog, colx, coly, colz);
#undef PWN_SEG_ST
#endif
#undef colx
#undef coly
#undef colz
}
#undef icx
#undef icy
#undef icz
