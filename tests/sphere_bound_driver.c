/* sphere_bound_driver.c -- the walk's ball predicate (pwnfps_amd/csrc/sphere_bound.h) compiled for the CPU, for
   tests/test_sphere_bounds.py: the same text the kernels compile, evaluated for arrays of samples.  Built by the test with
   -ffp-contract=off, like the library. */
#include <stdint.h>
#include "sphere_bound.h"

/* sample i: pos[4i..], ray[4i..], the ball balls[5 * which[i]..] = cx, cy, cz, rr, neg_r;  out[i] = pwn_sb_pass */
void sb_pass_many(int has_w, long n, const float *pos, const float *ray, const float *balls, const int32_t *which, uint8_t *out)
{
	for(long i = 0; i < n; i++)
	{
		const float *p = pos + 4 * i, *r = ray + 4 * i, *b = balls + 5 * which[i];
		out[i] = (uint8_t)pwn_sb_pass(has_w, p[0], p[1], p[2], p[3], r[0], r[1], r[2], r[3], b[0], b[1], b[2], b[3], b[4]);
	}
}

/* v[4i..] normalised in place by the caller's normalise (the checker's table normalise, util.h:32-46) */
void sb_normalise_many(void (*norm)(const float in[4], float out[4]), long n, float *v)
{
	for(long i = 0; i < n; i++)
	{
		float o[4];
		norm(v + 4 * i, o);
		for(int k = 0; k < 4; k++) v[4 * i + k] = o[k];
	}
}

/* the constants the test restates the radius with */
double sb_const(int k)
{
	switch(k)
	{
		case 0: return PWN_SB_EPS_PROOF;
		case 1: return PWN_SB_ETA;
		case 2: return PWN_SB_D_MAX;
		case 3: return PWN_SB_R_LIMIT;
		case 4: return PWN_BOUND_MIN_RECORDS;
		case 5: return PWN_BOUNDS_MAX;
		case 6: return PWN_SB_COORD_LIMIT;
	}
	return 0.0;
}
