// trace_composite.inc -- a finished ray's colour composited with the surfaces it bounced off, fog included
// (trace.h:91-101), innermost first.  Textually included by both trace kernels where a pixel's ray has ended.
// Names it uses from the including scope:
//   L (Lds), COUNT, cnt;  depth (the number of surfaces the ray bounced off);  the composite stack, top entry first:
//   st_refl0, st_fog0, sc0x, sc0y, sc0z;  st_refl1, st_fog1, sc1x, sc1y, sc1z.
//   (The refill kernel keeps a two-entry shifted stack and includes this once.  The units kernel keeps its entries under names of their
//   own and includes it once per ENTRY, each time as a stack one entry deep -- `depth` 0 or 1, the second level's names aliased to the
//   first's and dead: trace_kernel.hip, ray_done.)
// Names it writes:
//   vx, vy, vz, vw (in: the last segment's colour; out: the pixel's, without w_acc).
//@R p_comp
// trace.h:91-101, innermost first
// the top of the stack is the last surface the ray bounced off, the entry below it the one before
if(depth >= 1)
{
	//@R p_comp1
	RG(RG_COMP1);
	const float r0 = st_refl0, q0 = 1.0f - st_refl0;
	vx = r0 * vx + q0 * sc0x; vy = r0 * vy + q0 * sc0y; vz = r0 * vz + q0 * sc0z; vw = r0 * vw;
	if(st_fog0 != 0.0f)
	{
		//@R p_comp1_fog
		RG(RG_COMP1_FOG);
		float f = glibc_expf(-0.6f * st_fog0, L.exp2), g = 1.0f - f;
		vx = f * vx + g; vy = f * vy + g; vz = f * vz + g; vw = f * vw + g;
	}
}
//@R p_comp
if(depth >= 2)
{
	//@R p_comp2
	RG(RG_COMP2);
	const float r1 = st_refl1, q1 = 1.0f - st_refl1;
	vx = r1 * vx + q1 * sc1x; vy = r1 * vy + q1 * sc1y; vz = r1 * vz + q1 * sc1z; vw = r1 * vw;
	if(st_fog1 != 0.0f)
	{
		//@R p_comp2_fog
		RG(RG_COMP2_FOG);
		float f = glibc_expf(-0.6f * st_fog1, L.exp2), g = 1.0f - f;
		vx = f * vx + g; vy = f * vy + g; vz = f * vz + g; vw = f * vw + g;
	}
}
