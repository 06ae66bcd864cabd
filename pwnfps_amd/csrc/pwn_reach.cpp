// pwn_reach.cpp -- rays that stop after a given distance (pwn_trace_reach, pwn_trace_reach_device, pwn_trace_reach_hide_device):
// pwn_trace_hits' batches with one float more per ray, traced by the REACH kernels (trace_reach.hip).  The device forms are one trace
// launch on the caller's stream; the host form stages its arrays through pwn_trace_hits' buffers like that call (pwn_calls.cpp) and ends
// with its stream drained.
#include <stdio.h>
#include <string.h>
#include "pwn_internal.h"

// d_reach of the device forms, reach of the host form's staging: n floats, 4-byte aligned, apart from the n records the call writes
// (the rule of a d_hide array, word for word: pwn_i_hide_array_ok)
static bool reach_array_ok(const void *d_reach, size_t n, void *d_hits)
{
	const void *const wr[1] = { d_hits };
	return pwn_i_hide_array_ok(d_reach, n, wr, 1, n * sizeof(pwn_hit));
}

// hide: pwn_trace_reach_hide_device -- the launch reads ray i's hidden sphere from d_hide as well and is one of the REACH | HIDE kernels
static int reach_device(pwn_ctx *c, int n, const void *d_rays, const void *d_reach, bool hide, const void *d_hide, int flags, void *d_hits, void *stream)
{
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && (d_rays == NULL || d_hits == NULL)) || (flags & ~PWN_RAYS_HAS_W) != 0) return PWN_EINVAL;
	if(((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_hits & 15u) != 0) return PWN_EINVAL;
	if(n > 0 && !reach_array_ok(d_reach, (size_t)n, d_hits)) return PWN_EINVAL;
	if(hide && n > 0 && !pwn_i_hide_array_ok(d_hide, (size_t)n, &d_hits, 1, (size_t)n * sizeof(pwn_hit))) return PWN_EINVAL;
	const int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	pwn_trace_launch T = { .rays = { (const float *)d_rays, NULL, (uint32_t)n, (flags & PWN_RAYS_HAS_W) != 0, d_hits, hide ? (const int32_t *)d_hide : NULL, (const float *)d_reach },
		.stream = (hipStream_t)stream };
	return pwn_i_launch_trace(c, &T);
}
extern "C" int pwn_trace_reach_device(pwn_ctx *c, int n, const void *d_rays, const void *d_reach, int flags, void *d_hits, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_reach_device");
	return reach_device(c, n, d_rays, d_reach, false, NULL, flags, d_hits, stream);
}
extern "C" int pwn_trace_reach_hide_device(pwn_ctx *c, int n, const void *d_rays, const void *d_reach, const void *d_hide, int flags, void *d_hits, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_reach_hide_device");
	return reach_device(c, n, d_rays, d_reach, true, d_hide, flags, d_hits, stream);
}

// The host form's staging for a call of n rays, in pwn_trace_hits' buffers (80 B a ray there: the larger need counts): the records at 0
// (32 B a ray), the reaches behind them at 32 n (4 B), the hit records at 36 n rounded up to a 16-byte word (48 B) -- 84 B a ray and at most
// 12 more; one copy up (records and reaches), one down (hits)
extern "C" int pwn_trace_reach(pwn_ctx *c, int n, const float *rays, const float *reach, pwn_hit *hits)
{
	GRP_REFUSE(c, "pwn_trace_reach");
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && (rays == NULL || reach == NULL || hits == NULL))) return PWN_EINVAL;
	if(((uintptr_t)reach & 3u) != 0) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	const size_t N = (size_t)n, per = 32 + sizeof(pwn_hit);
	const size_t hoff = (36 * N + 15) & ~(size_t)15, need = hoff + sizeof(pwn_hit) * N;
	rc = pwn_i_staging_reserve(c, (need + per - 1) / per, per, "pwn_trace_reach", &c->h_hits, &c->d_hits, &c->hits_cap);
	// (the reserve counts in pwn_trace_hits' 80-byte rays: the message names the caller's)
	if(rc == PWN_ENOMEM) snprintf(c->err, sizeof(c->err), "pwn_trace_reach: no room for %d rays", n);
	if(rc != PWN_OK) return rc;
	unsigned char *h = c->h_hits, *d = c->d_hits;
	memcpy(h + 32 * N, reach, 4 * N);
	pwn_trace_launch T = { .rays = { (const float *)d, NULL, (uint32_t)n, false, d + hoff, NULL, (const float *)(d + 32 * N) }, .stream = s };
	rc = pwn_i_rays_stage_and_launch(c, s, rays, N, h, d, 36 * N, &T, hoff, need);
	if(rc != PWN_OK) return rc;
	memcpy(hits, h + hoff, sizeof(pwn_hit) * N);
	return PWN_OK;
}
