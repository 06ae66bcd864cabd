// trace_shade.inc -- the colour of what a ray segment ended on and what the surface does to the ray: a wall
// (trace.h:108-154 and the axis-aligned mirrors of trace.h:50-75) or the committed sphere (trace.h:283-291).
// Textually included by both trace kernels behind their walk, for the lanes whose segment ended on a surface.
// Names it uses from the including scope:
//   L (Lds), COUNT, HAS_W, LISTS (tables.h PWN_LF_*), V, cnt;  ev (EV_WALL, else the sphere), base, ray;  the colour the segment is lit with:
//   icx, icy, icz;  the sphere candidate: aux_idx, aux_pos, aux_diff.
// Names it writes:
//   colx, coly, colz (the segment's colour), refl (the surface's reflectivity), w_acc;  pos (moved off the surface);
//   ray (mirrored at a wall; the floor and a sphere get theirs in trace_bounce.inc);  ldir (-1: a sphere);
//   aux_norm (the sphere's normal); aux_idx (inline records: the sphere's byte offset).
//@R p_post
if(ev == EV_WALL)
{
	//@R p_wall
	RG(RG_WALL);
	// trace.h:108-154, and the axis-aligned mirrors of trace.h:50-75.  Colour by wall class and what
	// the face does to the ray are two constant tables in LDS (tables.h PWN_T_FACES): three 16-byte
	// reads instead of two switch trees (which the compiler builds out of lane masks and branches)
	const pwn_f4 wc = L.faces[base];
	const pwn_f4 fa = L.faces[4 + 2 * ldir], fb = L.faces[5 + 2 * ldir];
	float diffuse = (ldir & 1) ? ray.z : ray.x;
	diffuse = ldir >= FYP ? ray.y : diffuse;
	diffuse = __uint_as_float(__float_as_uint(diffuse) ^ __float_as_uint(fb.w));      // -ray.c on the N faces
	if(diffuse < 0.0f) diffuse = 0.0f;
	const float amb = 0.1f;
	diffuse = (1.0f - amb) * diffuse + amb;
	colx = diffuse * (icx * wc.x); coly = diffuse * (icy * wc.y); colz = diffuse * (icz * wc.z);
	w_acc = __builtin_fmaf(diffuse, 0.0f, w_acc);
	refl = fa.w;
	// the mirror: flip the ray component along the face normal, step 0.001 off the surface (the other
	// axes add -0.0f, which changes nothing); the floor (FYN) takes the step here and its ray from
	// the rippled normal below
	ray.x = __uint_as_float(__float_as_uint(ray.x) ^ __float_as_uint(fa.x));
	ray.y = __uint_as_float(__float_as_uint(ray.y) ^ __float_as_uint(fa.y));
	ray.z = __uint_as_float(__float_as_uint(ray.z) ^ __float_as_uint(fa.z));
	pos.x += fb.x; pos.y += fb.y; pos.z += fb.z;
}
else
{
	//@R p_sphere
	RG(RG_SPHERE);
	// trace.h:283-291 for the committed sphere
	// (inline records: aux_idx is the record's LDS address; which sphere it is of -- a byte offset -- is looked up here, once per hit)
	// (the global form: aux_idx is the record's index; which sphere -- an index -- and the sphere itself come from device memory)
	pwn_f4 s0, s1;
	if constexpr(LISTS == PWN_LF_GLOBAL)
	{
		const pwn_f4 *sp = L.g_sph + 2u * (size_t)L.g_which[aux_idx];
		s0 = sp[0]; s1 = sp[1];
	}
	else
	{
		if constexpr(LISTS == PWN_LF_INLINE) aux_idx = L.recsph[(aux_idx - PWN_T_BINIDX) >> 4];
		const PWN_LDS pwn_f4 *sp = (const PWN_LDS pwn_f4 *)((const PWN_LDS unsigned char *)L.sph + aux_idx);      // (a byte offset)
		s0 = sp[0]; s1 = sp[1];
	}
	V d;
	d.x = aux_pos.x - s0.x; d.y = aux_pos.y - s0.y; d.z = aux_pos.z - s0.z;
	if constexpr(HAS_W) d.w = aux_pos.w - 1.0f; else d.w = 0.0f;
	aux_norm = vnormalise<HAS_W>(L.rsq, d);
	colx = aux_diff * s1.y; coly = aux_diff * s1.z; colz = aux_diff * s1.w;
	w_acc = __builtin_fmaf(aux_diff, 0.0f, w_acc);
	refl = s1.x;
	ldir = -1;
	pos = aux_pos;
}
