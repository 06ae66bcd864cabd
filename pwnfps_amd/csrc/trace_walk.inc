// trace_walk.inc -- ONE cell step of the walk (trace.h:250-675), textually included by both
// trace kernels inside their walk loop.  Names it uses from the including scope:
//   L (Lds), COUNT, HAS_W, LISTS (the form of the per-cell lists, PWN_LF_*: tables.h), V, cnt;  the ray: pos, ray, cxz (cell x | z << 16), sx, sz (the steps (gx, 0) and
//   (0, gz) in the same packing: trace_common.h), ldx, ldz, ldy, gyp,
//   wx, wy, wz, iax, iay, iaz, iay_dn, iay_up_bits, cw, cdist, fog, ldir, ev, base;
//   how the including loop spells "no event yet" in ev, which it alone reads for its exit: WALK_EV_KEEP, the value a step without an
//   event leaves in ev, and WALK_EV_OPEN(ev), true while none has been recorded (trace_refill.hip: 0 and == 0; trace_kernel.hip
//   carries its step count in ev below zero: ev itself and <= 0);
//   the nearest sphere candidate: aux_dist, aux_diff, aux_idx, aux_pos;
//   HITREC (compile-time; false in every kernel that shades): the walk also keeps what a first-hit record needs and the
//   shading never asks for -- hit_cxz, the reference's cx, cz when the segment returns, and hit_portals, the portals
//   this lane crossed.  With HITREC false the two names are not touched and no instruction is made for them.
//   WALK_HIDDEN(object): optional.  True where the sphere with that index in the live table is one this lane's ray does not see
//   (trace_kernel.hip's HIDE instantiations: a compare with a value of the lane's or the wave's).  An including file that does not
//   define it -- the refill kernel -- gets the default, `false`, which does not evaluate its argument: no instruction is made.
//   WALK_REACH_ADV(y): optional.  Where a ramp step has skewed the ray it advances pos with, it hands that ray's y to an including loop that
//   has to know it (trace_kernel.hip's REACH instantiations: the point a given distance along the step).  An including file that does
//   not define it gets the default, which does not evaluate its argument: no instruction is made.
// One cell per iteration, one loop exit at the bottom.  The cell class is a bit test on the
// LDS word (tables.h).  The room body - by far the most frequent - is written with selects;
// lanes whose ray ended in it carry on through the (then meaningless) cell advance and leave
// at the bottom.
//@R w_head
#define AUX_HIT() (cdist > aux_dist)
#ifndef WALK_HIDDEN
#define WALK_HIDDEN(object) false
#define WALK_HIDDEN_DEFAULTED
#endif
#ifndef WALK_REACH_ADV
#define WALK_REACH_ADV(y) ((void)0)
#define WALK_REACH_ADV_DEFAULTED
#endif
if(COUNT)
{
	cnt.steps++;
	// once per wave and iteration: the lowest active lane
	if((__ffsll((long long)__ballot(1)) - 1) == (int)(threadIdx.x & 63)) cnt.wsteps++;
}

// HITREC: the cell this step begins in.  Behind the walk cxz is not it: the room body's ended lanes have advanced, a portal
// step has crossed, a ramp step has moved on before trace.h:668 sees the sphere.
if constexpr(HITREC) hit_cxz = cxz;

#ifdef PWN_PLAIN_STATS
// measurement build: in how many wave iterations is no lane in a special cell?
if(COUNT)
{
	const bool sp1 = ((int)cw < 0) || !(cw & PWN_C_ROOM);
	const bool sp2 = sp1 || (cw & (PWN_C_ROOM2 | PWN_C_DQ)) != 0u;
	const bool low = (__ffsll((long long)__ballot(1)) - 1) == (int)(threadIdx.x & 63);
	if(__ballot(sp1) == 0ull && low) cnt.apasses++;
	if(__ballot(sp2) == 0ull && low) cnt.apass_lanes++;
}
#endif

// trace.h:252-296: spheres binned to this cell (the test itself: trace_sphere.inc, included once per list form)
if((int)cw < 0)
{
	//@R w_sphlist
	WAVE_PATH(0);
	// A list that no lane of the wave can hit is not run (sphere_bound.h: the ball of a long list, the predicate and why a miss of
	// the ball is a miss of every member).  The balls come with the launch's arguments (tables.h) and are read from there with scalar
	// loads where they are needed: the id of the first active lane's list; all active lanes on that list (one ballot); that list one
	// of the launch's few (scalar compares with the four ids); then the lanes' test with the ball as scalar operands -- no register
	// holds a ball outside this block.  Lanes that stand on different lists, or on a list without a ball, run theirs as ever.
	// A skipped lane keeps pos, cdist and the candidate aux_* as they are; the sphere-test counter moves on by the list's length, as
	// if the tests had been made (the counters are the reference's counts).
	bool sb_skip = false;
	{
		//@R w_sphbound
		const PWN_KARGS pwn_trace_params *KP = (const PWN_KARGS pwn_trace_params *)__builtin_amdgcn_kernarg_segment_ptr();
		if(KP->nbounds != 0)
		{
			const uint32_t lid = (cw >> 16) & 0x7fffu;
			const uint32_t id0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lid);
			if(__ballot(lid != id0) == 0ull)
			{
				int k = -1;
#pragma unroll
				for(int i = PWN_BOUNDS_MAX - 1; i >= 0; i--) if(KP->bound_ids[i] == id0) k = i;
				if(k >= 0)
				{
					RG(RG_SPHBOUND);
					const PWN_KARGS pwn_sphere_bound *sb = &KP->bounds[k];
					const int pass = pwn_sb_pass(HAS_W, pos.x, pos.y, pos.z, pos.w, ray.x, ray.y, ray.z, ray.w, sb->cx, sb->cy, sb->cz, sb->rr, sb->neg_r);
					if(__ballot(pass) == 0ull)
					{
						RG(RG_SPHSKIP);
						sb_skip = true;
						if(COUNT) cnt.tests += sb->count;
					}
				}
			}
		}
	}
	//@R w_sphlist
	if(sb_skip) { }
	else if constexpr(LISTS == PWN_LF_GLOBAL)
	{
		// The records in device memory (tables.h): as the inline arm below, with one 16-byte GLOBAL load per test where that makes an
		// LDS read.  The cell word names the non-empty cell, liststart (one LDS read per list) the index of its first record;
		// aux_idx = the record's index.  The next record is asked for before this one is tested (behind the very last record lies
		// one more that the host packed for this read).  Plain, cached loads: no copy of the tables is written while a launch
		// reads it (pwn_tables.cpp).  Every index here comes out of the tables the host packed -- the cell word, liststart, the end
		// mark of a list -- and none out of a ray: no input bit pattern reaches an address (as argued at the ray modes' loads,
		// trace_kernel.hip).
		//@R w_sphrun
		uint32_t ri = ((const PWN_LDS uint32_t *)L.binidx)[(cw >> 16) & 0x7fffu];
		pwn_f4 nx = L.g_rec[(size_t)ri];
		for(;;)
		{
			//@R w_sphtest
			RG(RG_SPHTEST);
			const pwn_f4 s0 = nx;
			const uint32_t wb = __float_as_uint(s0.w);
			nx = L.g_rec[(size_t)ri + 1u];
#define PWN_ST_RAD2 __uint_as_float(wb & 0x7fffffffu)
#define PWN_ST_WHICH ri
#define PWN_ST_OBJECT L.g_which[ri]
#include "trace_sphere.inc"
#undef PWN_ST_RAD2
#undef PWN_ST_WHICH
#undef PWN_ST_OBJECT
			if((int)wb < 0) break;
			ri++;
		}
	}
	else if constexpr(LISTS == PWN_LF_INLINE)
	{
		// inline records (tables.h): one 16-byte read per test; the last record of the cell's list carries the sign bit in r*r.
		// aux_idx = the record's LDS address (which sphere: looked up when shaded).  The NEXT record is asked for before this one
		// is tested, so that the read's latency passes during the test (behind a list's last record lie the next list or the
		// "which sphere" array: read, never used).  Two register moves per test more and 0.9 % less launch time at 4K, 2 % at
		// 720p (profiles/r5/sphere_lists_ab.txt) -- the compiler leaves the read where the source has it, in front of its use.
		//@R w_sphrun
		const PWN_LDS pwn_f4 *rp = (const PWN_LDS pwn_f4 *)L.binidx + ((cw >> 16) & 0x7fffu);
		pwn_f4 nx = *rp;
		for(;;)
		{
			//@R w_sphtest
			RG(RG_SPHTEST);
			const pwn_f4 s0 = nx;
			const uint32_t wb = __float_as_uint(s0.w);
			nx = rp[1];
#define PWN_ST_RAD2 __uint_as_float(wb & 0x7fffffffu)
#define PWN_ST_WHICH ((uint32_t)(uintptr_t)rp)
#define PWN_ST_OBJECT ((uint32_t)L.recsph[(PWN_ST_WHICH - PWN_T_BINIDX) >> 4] >> 5)
#include "trace_sphere.inc"
#undef PWN_ST_RAD2
#undef PWN_ST_WHICH
#undef PWN_ST_OBJECT
			if((int)wb < 0) break;
			rp++;
		}
	}
	else
	{
		//@R w_sphrun
		const PWN_LDS uint16_t *lp = L.binidx + ((cw >> 16) & 0x7fffu);
		for(uint32_t si = *lp; si != PWN_LIST_END; si = *++lp)
		{
			//@R w_sphtest
			RG(RG_SPHTEST);
			// (si is the sphere's byte offset; its position and r*r are one 16-byte load: tables.h)
			const pwn_f4 s0 = *(const PWN_LDS pwn_f4 *)((const PWN_LDS unsigned char *)L.sph + si);         // x, y, z, r*r
#define PWN_ST_RAD2 s0.w
#define PWN_ST_WHICH si
#define PWN_ST_OBJECT (si >> 5)
#include "trace_sphere.inc"
#undef PWN_ST_RAD2
#undef PWN_ST_WHICH
#undef PWN_ST_OBJECT
		}
	}
}

//@R w_head
// (ONE test for "a sphere list, or not a room" -- (cw ^ ROOM) & (SPH | ROOM) -- with the sphere list and the room test nested under
// it was built and measured: +1.1 % at 4K, the compiler pays for the nesting in register moves; profiles/r3_walk_exit.txt)
if(cw & PWN_C_ROOM)
{
	//@R w_room
	WAVE_PATH(1);
	// trace.h:302-352 (1-high) and 354-441 (2-high) share this body
	const bool room2 = (cw & PWN_C_ROOM2) != 0u;
	// 2-high: the ceiling is one unit further when looking up (trace.h:357,392)
	// = (room2 && gyp) ? iay : 0: the ROOM2 bit stretched to a mask (one v_bfe_i32)
	// (a sign-extended 1-bit field; written as an instruction because the compiler turns the
	// shift form back into two compares and a select on gyp)
	uint32_t m2;
	asm("v_bfe_i32 %0, %1, 9, 1" : "=v"(m2) : "v"(cw));
	static_assert(PWN_C_ROOM2 == (1u << 9), "v_bfe_i32 above reads bit 9");
	const float up2 = __uint_as_float(iay_up_bits & m2);
	wy += up2;
	const float cdist0 = cdist;
	// trace.h:156-184, then 331-340 on the same comparisons
	const bool xlt = wx < wz;
	const float txz = xlt ? wx : wz;
	// "wy < wx && wy < wz" as ONE comparison with the smaller of the two.  With a NaN among them this is the
	// same except for wx NaN and wz a number -- which no ray has: wx and wz are finite fractions times
	// iax / iaz, these are NaN only when ray.x / ray.z are, and a ray's components come out of one normalise
	// (all NaN or none; the walk only swaps or negates x and z in portals).
	const bool ymin = wy < txz;
	const float t = ymin ? wy : txz;
	cdist += t;
	pos = vadd<HAS_W>(vscale<HAS_W>(t, ray), pos);
	const bool hit = AUX_HIT();
	if(cw & PWN_C_FOG)
	{
		//@R w_fog
		WAVE_PATH(2);
		// fogbeg = distance at entry (trace.h:309,359); sums in the
		// reference build's operation order
		float fn = (fog - cdist0) + cdist;
		if(hit) fn = aux_dist > cdist0 ? (fog + aux_dist) - cdist0 : fog;
		fog = fn;
	}
	//@R w_room
	// (Round 3 tried keeping the STEP taken last instead of selecting ldir here and decoding the face after the walk: one select
	// less per step, ~19 instructions more per segment -- at 4.5 steps per segment a loss, +6 M VALU instructions per 4K frame.)
	// (Round 4: the four selects on `xlt` below as full-rate bit selects under one register mask -- v_bfi_b32 or v_bitop3_b32,
	// the mask made by one v_cndmask -- measured 0.5-1 % slower at 4K: five instructions where there are four.  Code in
	// commit fe41695, profiles/r4/walk_variants.txt.)
	ldir = xlt ? ldx : ldz;                      // a y exit is patched in after the walk
	ev = hit ? EV_SPHERE : (ymin ? EV_WALL : WALK_EV_KEEP);
	wy = (wy - txz) - up2;
	wz = xlt ? wz - txz : iaz;
	wx = xlt ? iax : wx - txz;
	// (fetching both candidate next cells ahead of the decision, to take the LDS round trip off the
	// step's dependent chain, costs five more instructions and was 2.5 % slower)
	cxz = cxz_add(cxz, xlt ? sx : sz);
	const uint32_t ncw = cellword_pk(L, cxz);
	// trace.h:341-351,393-441 do something only when the height changes: from a "-cell
	// into a 2-high one, or out of a 2-high cell into anything else ('#'/'&' are the only
	// 2-high cells, so 2-high -> 2-high neither shifts y nor can be a wall).  One bit:
	// next is 2-high ? current is " : current is 2-high  (DQ sits two bits above ROOM2)
	static_assert(PWN_C_DQ == (PWN_C_ROOM2 << 2), "the shift below lines DQ up with ROOM2");
	const uint32_t height_changes = (((cw >> 2) & ncw) | (cw & ~ncw)) & PWN_C_ROOM2;
	if(height_changes != 0u && !(hit || ymin))          // (no event, from the masks instead of a compare)
	{
		//@R w_height
		WAVE_PATH(3);
		if(!room2)
		{
			if(ncw & PWN_C_ROOM2)        // here cw is the "-cell
			{
				pos.y += 1.0f;
				wy -= iay_dn;
			}
		}
		else
		{
			//@R w_height_r2
			RG(RG_HC_R2);
			if(ncw & PWN_C_DQ)
			{
				pos.y -= 1.0f;
				wy += iay_dn;
			}
			if(pos.y < 0.0f || pos.y > 1.0f)
			{
				//@R w_height_out
				RG(RG_HC_OUT);
				// trace.h:404-413: the cell type there, looked at through a portal where the cell is an endpoint -- decided
				// per level, two bits of the cell word (cell_bake.h)
				if(!(ncw & PWN_C_LT2))
				{
					if(ncw & PWN_C_LTDQ)
					{
						pos.y += 1.0f;
						wy -= iay_dn;
					}
					ev = EV_WALL; base = BASE_WALL;
					// (the one return behind the reference's own cell advance, trace.h:393-441: the wall is the cell stepped into)
					if constexpr(HITREC) hit_cxz = cxz;
				}
			}
		}
	}
	//@R w_room
	cw = ncw;
}
//@R w_else
else
{
	RG(RG_ELSE);
	// Three arms that exclude one another, written as three ifs in a row on the cell word as it came in: an arm that changes
	// nothing (a solid cell) then passes no join with the arm that changes fifteen variables (a portal) -- as one
	// if / else-if / else chain the compiler gave the portal's results registers of their own and copied fifteen values in and
	// fifteen back in EVERY non-room step.
	const uint32_t cw_in = cw;
	if(cw_in & PWN_C_RAMP)
	{
		//@R w_ramp
		WAVE_PATH(4);
		// trace.h:443-505: ramps
		int cx = cxz_x(cxz), cz = cxz_z(cxz);
		const int gx = cxz_x(sx), gz = cxz_z(sz);
		const float ramp = 0.5f;
		const bool alongx = (cw & PWN_C_RAMPX) != 0u;
		const bool minus = (cw & PWN_C_RAMPM) != 0u;
		float tilt = alongx ? ray.x : ray.z;
		if(minus) ray.y -= ramp * tilt; else ray.y += ramp * tilt;
		WALK_REACH_ADV(ray.y);
		wy = pos.y;
		if(ray.y >= 0.0f) wy = 1.0f - wy;
		wy *= 1.0f / (ray.y < 0.0f ? -ray.y : ray.y);
		if(AUX_HIT()) ev = EV_SPHERE;
		else
		{
			// trace.h:470 passes gy where trace_ray_through expects gx; the
			// face is recomputed from the ray signs right after (:474-487)
			const bool ymin = (wy < wx) && (wy < wz);
			const bool xlt = wx < wz;
			const float t = ymin ? wy : (xlt ? wx : wz);
			cdist += t;
			pos = vadd<HAS_W>(vscale<HAS_W>(t, ray), pos);
			if(ymin)
			{
				ldir = (ray.y < 0.0f ? FYN : FYP);
				ev = EV_WALL; base = (ray.y >= 0.0f ? BASE_CEIL : BASE_FLOOR);
			}
			else
			{
				if(xlt)
				{
					ldir = (ray.x < 0.0f ? FXN : FXP);
					wy -= wx; wz -= wx; wx = iax; cx += gx;
				}
				else
				{
					ldir = (ray.z < 0.0f ? FZN : FZP);
					wx -= wz; wy -= wz; wz = iaz; cz += gz;
				}
				tilt = alongx ? ray.x : ray.z;
				if(minus) ray.y += ramp * tilt; else ray.y -= ramp * tilt;
				wy = pos.y;
				if(ray.y >= 0.0f) wy = 1.0f - wy;
				wy *= iay;
				cxz = cxz_pack(cx, cz);
				cw = cellword_pk(L, cxz);
			}
		}
	}
	if((cw_in & (PWN_C_RAMP | PWN_C_PORTAL)) == PWN_C_PORTAL)
	{
		//@R w_portal
		WAVE_PATH(5);
		// trace.h:508-650: portal
		// which endpoint this cell is, or that it is none, is the cell's portal state (cell_bake.h)
		const uint32_t pst = cw_in & PWN_C_PST_MASK;
		if(pst < (PWN_PST_REC0 << PWN_C_PST_SHIFT))
		{
			//@R w_portal_wall
			RG(RG_PORTAL_WALL);
			// unpaired letter, or a letter standing in a cell that is not one
			// of its endpoints (trace.h:514-520,551-559)
			static_assert(BASE_WALL + PWN_PST_WALL == BASE_WALL && BASE_WALL + PWN_PST_MAGENTA == BASE_MAGENTA, "the state is the wall class");
			if(AUX_HIT()) ev = EV_SPHERE;
			else { ev = EV_WALL; base = BASE_WALL + (int)(pst >> PWN_C_PST_SHIFT); }
		}
		else
		{
			//@R w_portal_go
			RG(RG_PORTAL_GO);
			// the way to the other endpoint (its sign applied for THIS endpoint) is one record, the rotation two bits of the cell
			// word.  The other endpoint's cell is this one plus the same whole numbers, in floats: this cell is inside the grid.
			const pwn_h2 er = ep_rec(L, pst);
			const float edx = (float)er.x, edz = (float)er.y;
			int gx = cxz_x(sx), gz = cxz_z(sz);
			pos.x += edx;
			pos.z += edz;
			const int rot = (int)((cw_in >> PWN_C_PROT_SHIFT) & 3u);
			if(COUNT) cnt.portals++;
			if constexpr(HITREC) hit_portals++;

			// trace.h:561-622.  The operation order is the one the reference
			// build executes (its -ffast-math cancels the +-0.5 terms).
			const float trx = pos.x, trz = pos.z, trvx = ray.x, trvz = ray.z;
			const int tgx = gx, tgz = gz;
			const float fcx = (float)cxz_x(cxz) + edx, fcz = (float)cxz_z(cxz) + edz;
			int cx = (int)fcx, cz = (int)fcz;
			ldir = (ldir - rot) & 3;
			if(rot & 1)
			{
				//@R w_portal_odd
				RG(RG_PORTAL_ODD);
				float t = wx; wx = wz; wz = t;
				t = iax; iax = iaz; iaz = t;
				if(rot == 1)
				{
					pos.x = (trz + fcx) - fcz;
					pos.z = (1.0f - trx) + (fcx + fcz);
					ray.x = trvz; ray.z = -trvx;
					gx = tgz; gz = -tgx;
				}
				else
				{
					pos.x = (1.0f - trz) + (fcx + fcz);
					pos.z = (fcz + trx) - fcx;
					ray.x = -trvz; ray.z = trvx;
					gx = -tgz; gz = tgx;
				}
			}
			else if(rot == 2)
			{
				//@R w_portal_rot2
				RG(RG_PORTAL_ROT2);
				pos.x = (fcx + 0.5f) * 2.0f - trx;
				pos.z = (fcz + 0.5f) * 2.0f - trz;
				ray.x = -trvx; ray.z = -trvz;
				gx = -tgx; gz = -tgz;
			}
			//@R w_portal_go
			ldx = (gx < 0 ? FXN : FXP); ldz = (gz < 0 ? FZN : FZP);
			// trace.h:624-647: step out of the far endpoint
			if(ldir == FZP) { cz++; pos.z += 1.0f; }
			else if(ldir == FXN) { cx--; pos.x -= 1.0f; }
			else if(ldir == FZN) { cz--; pos.z -= 1.0f; }
			else { cx++; pos.x += 1.0f; }
			cxz = cxz_pack(cx, cz);
			sx = (uint32_t)gx & 0xffffu; sz = (uint32_t)gz << 16;
			cw = cellword_pk(L, cxz);
		}
	}
	if((cw_in & (PWN_C_RAMP | PWN_C_PORTAL)) == 0u)
	{
		// trace.h:651-664: solid
		//@R w_solid
		WAVE_PATH(6);
		if(AUX_HIT()) ev = EV_SPHERE;
		else { ev = EV_WALL; base = (ldir == FYP ? BASE_CEIL : BASE_WALL); }
	}
	//@R w_else
	// trace.h:668-673 (in the room body the same test sits right after the step)
	if(WALK_EV_OPEN(ev) && AUX_HIT()) ev = EV_SPHERE;
}
// (trace.h:250,677, running out of steps, is the including loop's business)
#undef AUX_HIT
#ifdef WALK_HIDDEN_DEFAULTED
#undef WALK_HIDDEN
#undef WALK_HIDDEN_DEFAULTED
#endif
#ifdef WALK_REACH_ADV_DEFAULTED
#undef WALK_REACH_ADV
#undef WALK_REACH_ADV_DEFAULTED
#endif
