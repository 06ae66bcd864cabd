/* sphere_bound.h -- a bounding ball per long sphere list: may a ray skip the whole list?
 *
 * Plain C, one text for both sides: the walk (trace_walk.inc) asks pwn_sb_pass per lane in front of a cell's list, the host
 * (level_host.c, pwn_sphere_bounds_build) makes the balls with the constants below, and tests/test_sphere_bounds.py compiles the
 * predicate for the CPU and holds it against the exact test on millions of rays.
 *
 * THE EXACT TEST (trace.h:256-270, trace_sphere.inc), for a member s of the list, in fp32:
 *     rel = s - pos (w lane: 1 - pos.w),  d2 = rel.rel,  dt = rel.ray;   accept  <=>  dt > 0  and  d2 - dt*dt < r*r.
 * The ray is only table-normalised: lambda^2 = |ray|^2 = 1 +- 7e-4.  Rays and positions can be anything at all (far starts,
 * infinities, NaN: a ray with an infinite component "hits" with calc = -inf), so the skip is taken only under two GUARDS, and
 * outside them the list is run as it always was:
 *     G1   d2c = |c - pos|^2 <= 4                 (c = the ball's centre; the same lanes and the same w rule as rel)
 *     G2   | |ray|^2 - 1 | <= PWN_SB_RAY_EPS      (2^-10)
 * and inside them a lane PASSES (the list must be run) unless
 *     MISS   dtc <= -R_eff   or   d2c - dtc*dtc >= RR,        dtc = (c - pos).ray,  RR = R_eff^2 rounded up.
 * Every comparison is written so that it is FALSE with a NaN operand, and pass = !(G1 && G2 && MISS): a NaN anywhere passes.
 *
 * WHY A MISS OF THE BALL IS A MISS OF EVERY MEMBER.  First in real numbers.  Write rel_s = relc + d_s with relc = c - pos and
 * d_s = s - c (the w lanes of rel_s and relc are the same number, so d_s has none), rho_s = |d_s|, lambda = |ray|,
 * u = ray / lambda, and
 *     f(v) = |v|^2 - (v.ray)^2        (the exact test is f(rel_s) < r_s^2, the ball's f(relc) < RR).
 * f is the quadratic form of I - ray ray^T, whose eigenvalues are 1 and 1 - lambda^2.
 *   lambda <= 1: the form is positive semidefinite, sqrt f is a seminorm with sqrt f(v) <= |v|, and the triangle inequality
 *     gives, if s accepts,  sqrt f(relc) <= sqrt f(rel_s) + sqrt f(d_s) < r_s + rho_s.
 *   lambda > 1, e = lambda^2 - 1 <= eps: f(v) = g(v) - e (v.u)^2 with g(v) = |v|^2 - (v.u)^2, the squared distance of v from
 *     the line along u, for which the same holds.  If s accepts, g(rel_s) = f(rel_s) + e (rel_s.u)^2 < r_s^2 + eps a_s^2 with
 *     a_s = |rel_s| <= |relc| + rho_s <= 2 + rho_s (G1), and  sqrt f(relc) <= sqrt g(relc) <= sqrt g(rel_s) + rho_s.
 * Either way
 *     sqrt f(relc) < rho_s + sqrt(r_s^2 + eps a_s^2)  =: R0_s,
 * and for the other half, dt_s > 0 gives dtc = dt_s - d_s.ray > -rho_s lambda >= -rho_s (1 + eps) > -R0_s (sqrt(eps) a_s > eps rho_s).
 * So in real numbers an accept of s implies dtc > -R0_s and f(relc) < R0_s^2: not MISS with any R_eff >= max_s R0_s.
 *
 * fp32.  Both tests are evaluated in fp32, each product and sum rounded once (no FMA: the build's -ffp-contract=off), denormal
 * results flushed on the device (that moves a value by < 1.2e-38).  Inside the guards and with rho_s + r_s <= PWN_SB_R_LIMIT
 * every intermediate of both tests is below 16 in magnitude (|rel_s| <= 3.5, lambda^2 <= 1.001), so a rounding moves it by at
 * most 2^-20; the subtractions s - pos and c - pos round ONCE, relative to their result, whatever the coordinates are.  Carried
 * through (3 differences, 6 products and 5 sums per test, dt squared: d(dt*dt) <= 2 * 3.6 * 5e-6), the fp32 value of
 * d2 - dt*dt differs from its real value by less than 5e-5 in either test, that of dt and dtc by less than 5e-6, that of |ray|^2
 * by less than 4e-7.  The ball's own centre and radius are computed in double and rounded outwards.  So:
 *     eps   = PWN_SB_EPS_PROOF = 1.0e-3    >= 2^-10 + 4e-7: what G2 lets through, in real numbers;
 *     eta   = PWN_SB_ETA       = 2^-12     >= 2 * 5e-5 and the fp32 rounding of r*r (<= 2^-24 * 2.25): an fp32 accept of s
 *                                             means f(rel_s) < r_s^2 + eta/2 in real numbers, and an fp32 MISS of the ball
 *                                             means f(relc) >= RR - eta/2;
 *     a_s   = PWN_SB_D_MAX + rho_s,  PWN_SB_D_MAX = 2.001 >= sqrt(4 + 5e-5): what G1 lets through;
 *     R_eff = max_s( rho_s + sqrt(r_s^2 + eps a_s^2 + eta) ) * (1 + 2^-20), rounded up to fp32; RR = R_eff^2 rounded up.
 * eta under the root is at least 0.0156 of radius (sqrt eta) for the smallest spheres and 4e-4 for r = 0.3, far above the 1e-5
 * the dt half needs.  For the benchmark's list (cell (9, 5): one sphere of r = 0.3 at rho = 0.021 from the centre, five of r = 0.1
 * at rho = 0.279 and 0.301, eight of r = 0.03 at rho = 0.317) the maximum is taken by four of the r = 0.1 spheres at rho_s = 0.3008:
 *     sqrt(0.01 + 1e-3 * 2.3018^2 + 2.44e-4) = 0.1247,  R_eff = 0.3008 + 0.1247 = 0.4254   (the tight ball max(rho_s + r_s) is 0.4008);
 * the big sphere gives 0.021 + sqrt(0.09 + 1e-3 * 2.022^2 + 2.44e-4) = 0.329, the small ones 0.317 + 0.081 = 0.398.
 * A list is given no ball when a member is not finite, lies further than PWN_SB_COORD_LIMIT from the origin on an axis, or
 * rho_s + r_s exceeds PWN_SB_R_LIMIT for one of them (R_eff is then at most 1.5 + sqrt(eps) 3.51 + ... < 1.7).
 */
#ifndef PWN_SPHERE_BOUND_H
#define PWN_SPHERE_BOUND_H
#include <stdint.h>

#ifndef PWN_BOUNDS_MAX
#define PWN_BOUNDS_MAX 4              /* lists with a ball per launch: the longest ones (pwn_sphere_bounds_build) */
#endif
/* The shortest list that gets one.  By the issue model (profiles/r5_issue_model.txt) a sphere test is 19 VALU wave-instructions
   (w_sphtest) and the ball's block 29 (w_sphbound), beside 6 and 34 scalar / branch instructions, which issue in the shadow of
   other waves' VALU work.  In VALU instructions a visit of an n-list costs 19 n without the ball and 29 + p 19 n with it, p = the
   share of visits in which some lane passes: 0.30 measured on the benchmark's cluster (profiles/sphere_bounds/ab.txt).
   Break-even there is n = 29 / (0.70 * 19) = 2.2; with the scalar instructions priced like the others, 63 / (0.70 * 25) = 3.6.
   Four, the next whole number: at p = 0.30 a list of four saves 24 of its 76 VALU instructions per visit, and it is made
   slower only where more than three visits in five pass (29 + p 76 > 76 from p = 0.62). */
#define PWN_BOUND_MIN_RECORDS 4
#define PWN_SB_RAY_EPS    0.0009765625f       /* 2^-10: guard G2 */
#define PWN_SB_D2_MAX     4.0f                /* guard G1 */
#define PWN_SB_EPS_PROOF  1.0e-3
#define PWN_SB_ETA        0.000244140625      /* 2^-12 */
#define PWN_SB_D_MAX      2.001
#define PWN_SB_R_LIMIT    1.5
#define PWN_SB_COORD_LIMIT 1024.0

/* One ball.  32 bytes: the kernel reads a record with one scalar load (pwn_trace_params.bounds, tables.h). */
typedef struct pwn_sphere_bound
{
	uint32_t id;          /* the list, as bits 16..30 of its cell's word carry it in the form the tables have (tables.h) */
	uint32_t count;       /* records in the list: what a skip adds to the sphere-test counter per lane */
	float cx, cy, cz;     /* centre: the mean of the members' centres */
	float rr;             /* RR above */
	float neg_r;          /* -R_eff */
	uint32_t cell;        /* z * 64 + x of the list's cell */
} pwn_sphere_bound;

#ifdef __HIPCC__
#define PWN_SB_FN __device__ __host__ __forceinline__
#else
#define PWN_SB_FN static inline
#endif

/* 1: run the list; 0: no member can accept this ray.  pos / ray as the walk has them; has_w = 0: the 3-lane arithmetic (pw, rw not read). */
PWN_SB_FN int pwn_sb_pass(int has_w, float px, float py, float pz, float pw, float rx, float ry, float rz, float rw,
	float cx, float cy, float cz, float rr, float neg_r)
{
	const float ex = cx - px, ey = cy - py, ez = cz - pz;
	float d2c, dtc, l2;
	if(has_w)
	{
		const float ew = 1.0f - pw;
		d2c = (ex * ex + ez * ez) + (ey * ey + ew * ew);
		dtc = (ex * rx + ez * rz) + (ey * ry + ew * rw);
		l2 = (rx * rx + rz * rz) + (ry * ry + rw * rw);
	}
	else
	{
		d2c = (ex * ex + ez * ez) + ey * ey;
		dtc = (ex * rx + ez * rz) + ey * ry;
		l2 = (rx * rx + rz * rz) + ry * ry;
	}
	const float dl = l2 - 1.0f;
	const int g1 = d2c <= PWN_SB_D2_MAX;
	const int g2 = (dl <= PWN_SB_RAY_EPS) & (dl >= -PWN_SB_RAY_EPS);
	const int miss = (dtc <= neg_r) | (d2c - dtc * dtc >= rr);
	return !(g1 & g2 & miss);
}
#endif
