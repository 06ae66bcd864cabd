// trace_bounce.inc -- the two bounces that are not an axis-aligned mirror (trace.h:9-75): off the rippled floor and
// off a sphere.  Textually included by both trace kernels behind trace_shade.inc, for the lanes whose ray goes on.
// Names it uses from the including scope:
//   L (Lds), COUNT, HAS_W, V, cnt;  ldir (FYN: the floor, < 0: a sphere), sec_current, aux_norm.
// Names it writes:
//   ray (the reflected direction, normalised), pos (a sphere: stepped 0.001 back along the ray).
//@R p_post
// trace.h:9-75
if(ldir == FYN)
{
	//@R p_floor
	RG(RG_FLOOR);
	const float pi = (float)3.14159265358979323846;
	float ang = (pi * 2.0f) * (
		(glibc_sincosf((pi * 0.5f) * pos.x, 0) + glibc_sincosf((pi * 0.5f) * pos.z, 1))
		+ sec_current);
	const float2 sc = glibc_sincosf_both(ang);
	V n; n.x = sc.x; n.y = 38.0f; n.z = sc.y; n.w = 0.0f;
	n = vnormalise<HAS_W>(L.rsq, n);
	float rmul = -2.0f * ((ray.x * n.x + ray.y * n.y) + ray.z * n.z);
	ray = vnormalise<HAS_W>(L.rsq, vadd<HAS_W>(vscale<HAS_W>(rmul, n), ray));
}
else if(ldir < 0)
{
	//@R p_sphrefl
	RG(RG_SPHREFL);
	pos = vsub<HAS_W>(pos, vscale<HAS_W>(0.001f, ray));
	float rmul = -2.0f * ((ray.x * aux_norm.x + ray.y * aux_norm.y) + ray.z * aux_norm.z);
	ray = vnormalise<HAS_W>(L.rsq, vadd<HAS_W>(vscale<HAS_W>(rmul, aux_norm), ray));
}
