// trace_setup.inc -- a ray segment's set-up (trace.h:186-248): the ray normalised, its starting cell, the walk's
// per-axis distances and reciprocals.  Textually included by both trace kernels in front of their walk.
// Names it uses from the including scope:
//   L (Lds), COUNT, HAS_W, V, cnt;  pos (where the segment starts), iray (its direction, not normalised).
// Names it writes (all declared by the kernel: what trace_walk.inc walks with):
//   ray, cxz, sx, sz, cw, wx, wy, wz, iax, iay, iaz, iay_dn, iay_up_bits, ldx, ldy, ldz, gyp (the ray looks up),
//   cdist, fog, aux_dist (no sphere candidate yet), ldir, ev (EV_NONE), base.
// Its own locals (lb, rsq_e, cx, cz, gx, gz, iay_) stay in the including scope.
//@R p_setup
cdist = 0.0f; fog = 0.0f;
// nearest sphere candidate (trace.h:193-199): distance, hit point, which sphere and
// its diffuse factor; normal, colour and reflectivity are rebuilt from these when
// the hit is committed
// aux_dist: the reference's "none yet" value -1 (trace.h:200) is kept as +inf here, so that
// "a candidate exists and lies behind us" is one comparison; a candidate whose distance is
// exactly -1.0f counts as none there and is stored as +inf here too
// (the candidate's other fields are read only behind aux_dist and the set-up leaves them alone: in the units kernel they
// keep what the segment before left in them -- declared in front of the loop -- instead of five moves per ray)
aux_dist = __builtin_inff();
if(COUNT) cnt.rays++;

// The set-up's table reads (1/sqrt, the first cell's word, three reciprocals) are each issued ahead of work that does not
// need them -- the compiler leaves an LDS read where the source has it, directly in front of its use, and sinks one that
// only a branch uses into that branch: -0.3 % launch time at 4K, -0.5 % on synth64 (profiles/r5/sphere_lists_ab.txt).
const uint32_t lb = __float_as_uint(dot3<HAS_W>(iray, iray));
const uint32_t rsq_e = tab_rsqrt_entry(L.rsq, lb);
int cx = (int)pos.x, cz = (int)pos.z;
// signs of the UN-normalised input (trace.h:225-227)
int gx = (iray.x < 0.0f ? -1 : 1);
int gz = (iray.z < 0.0f ? -1 : 1);
gyp = !(iray.y < 0.0f);          // gy > 0
// cell coordinates and steps in the packed form the walk uses (trace_common.h)
cxz = cxz_pack_start(cx, cz); sx = (uint32_t)gx & 0xffffu; sz = (uint32_t)gz << 16;
cw = cellword_pk(L, cxz);
wx = pos.x - (float)cx; wy = pos.y; wz = pos.z - (float)cz;
ldy = gyp ? FYP : FYN;
ldx = (gx < 0 ? FXN : FXP); ldz = (gz < 0 ? FZN : FZP);
// util.h:32-46
ray = vscale<HAS_W>(tab_rsqrt_finish(lb, rsq_e), iray);
// trace.h:220-222 clamp |ray| to EPSILON, trace.h:230-231 take the three reciprocals.  A normalised ray
// has all three magnitudes in [EPSILON, 2^126) unless it is degenerate: ONE test on the bit patterns
// (a NaN's is above every number's) and one wave-uniform branch; then nothing is clamped and all three
// reciprocals are the one-subtract table path (one LDS round trip, under way while the fractions are turned:
// a table index is in range whatever the bits are)
float iay_;
{
	const uint32_t EPSB = __float_as_uint(EPS);
	const uint32_t bx = __float_as_uint(ray.x) & 0x7fffffffu, by = __float_as_uint(ray.y) & 0x7fffffffu,
		bz = __float_as_uint(ray.z) & 0x7fffffffu;
	uint32_t ex = rcp_entry(L.rcp, bx), ey = rcp_entry(L.rcp, by), ez = rcp_entry(L.rcp, bz);
	const bool plain = max(max(bx - EPSB, by - EPSB), bz - EPSB) < 0x7e800000u - EPSB;
	if(ray.x >= 0.0f) wx = 1.0f - wx;
	if(ray.y >= 0.0f) wy = 1.0f - wy;
	if(ray.z >= 0.0f) wz = 1.0f - wz;
	// (statements the compiler may not reorder: the fractions first, then the wait for the table.  Not in the 4-lane
	// variant: its ordered form would need 12 bytes of scratch per lane for them)
	if constexpr(!HAS_W)
	{
		asm volatile("" : "+v"(wx), "+v"(wy), "+v"(wz));
		asm volatile("" : "+v"(ex), "+v"(ey), "+v"(ez));
	}
	if(__builtin_expect(__ballot(!plain) == 0ull, 1))
	{
		iax = __uint_as_float(ex - (bx & 0x7f800000u)); iay_ = __uint_as_float(ey - (by & 0x7f800000u));
		iaz = __uint_as_float(ez - (bz & 0x7f800000u));
	}
	else
	{
		//@R p_setup_slow
		RG(RG_SETUP_SLOW);
		// (the fractions above were turned by the unclamped signs: the clamp keeps ">= 0" as it was -- -0 counts as +)
		if(fabsf(ray.x) < EPS) ray.x = (ray.x < 0.0f ? -EPS : EPS);
		if(fabsf(ray.y) < EPS) ray.y = (ray.y < 0.0f ? -EPS : EPS);
		if(fabsf(ray.z) < EPS) ray.z = (ray.z < 0.0f ? -EPS : EPS);
		iax = tab_rcp(L.rcp, fabsf(ray.x)); iay_ = tab_rcp(L.rcp, fabsf(ray.y)); iaz = tab_rcp(L.rcp, fabsf(ray.z));
	}
}
//@R p_setup
iay = iay_;
wx *= iax; wy *= iay; wz *= iaz;
// the "-part of a two-level room shifts the floor by one: wy moves by -+iay
// (trace.h:345-349,381-385); iay_dn is the amount added when stepping DOWN into it
iay_dn = gyp ? iay : -iay;
iay_up_bits = gyp ? __float_as_uint(iay) : 0u;         // +iay when looking up, else +0
asm volatile("" : "+v"(iay_up_bits));        // keep it a register, not a select on gyp per step
ldir = FYN;
ev = EV_NONE; base = BASE_ROOM_Y;
