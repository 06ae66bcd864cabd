// reach_driver.cpp -- the host side of pwn_trace_reach / pwn_trace_reach_device / pwn_trace_reach_hide_device on the CPU, under
// AddressSanitizer + UBSan: pwn_reach.cpp against the stand-in runtime and the stand-in launcher (fake_kernels.cpp pwn_launch_trace),
// which for a mode with the REACH bit writes every ray a record made of the ray's number, its eight floats, its reach and its hide word ("device" memory is
// malloc'ed to the byte: a staging that is too small, an array read past its n entries or a pointer that is off is a report).  What is
// looked at: the host form's arrays there and back as its staging grows -- pwn_trace_hits' buffers, the larger need counts --, where in
// the staging the launch finds records, reaches and hits, the exact mode of every call's launch, the 3-lane / 4-lane rule, the empty batch,
// every refusal -- a group's handle among them -- and the overlap rules with nothing launched and nothing written, no leak behind
// pwn_destroy.
//     reach_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern "C" thread_local int pwn_fake_trace_mode;

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)
static pwn_trace_params g_P;
static int g_launches, g_mode = -1, g_reach_launches;      // trace launches; the mode of the last one; those with the REACH bit
static void on_trace(const pwn_trace_params *P, int, size_t) { g_P = *P; g_launches++; g_mode = pwn_fake_trace_mode; if(g_mode & PWN_KM_REACH) g_reach_launches++; }

// (fake_kernels.cpp's record)
static uint32_t mix(uint32_t a, uint32_t b) { a ^= b + 0x9e3779b9u + (a << 6) + (a >> 2); return a * 2654435761u; }
static void expect(uint32_t i, const float *ray, float reach, bool has_hide, int32_t hide, bool ray_w, uint32_t *o)
{
	uint32_t k = mix(i, has_hide ? (uint32_t)hide : 0x5555u), u;
	for(int q = 0; q < 8; q++) { memcpy(&u, ray + q, 4); k = mix(k, (ray_w || (q & 3) != 3) ? u : 0u); }
	memcpy(&u, &reach, 4);
	k = mix(k, u);
	for(uint32_t q = 0; q < 12u; q++) o[q] = mix(k, q);
}

int main(int argc, char **argv)
{
	REQ(argc == 2);
	static_assert(sizeof(pwn_hit) == 48, "a record is twelve words");
	pwn_fake_trace_hook = on_trace;
	pwn_ctx *c = NULL, *bare = NULL;
	REQ(pwn_init(&c, 0, 32, 16) == PWN_OK);
	REQ(pwn_level_load(c, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 32, 16) == PWN_OK);                    // no level
	const int NMAX = 9000;
	std::vector<float> rays(8 * (size_t)NMAX), reach(NMAX);
	std::vector<pwn_hit> hits(NMAX);
	auto fill = [&](bool w) {
		for(int i = 0; i < NMAX; i++)
		{
			for(int k = 0; k < 8; k++) rays[8 * (size_t)i + k] = (float)(i * 8 + k) * 0.125f;
			rays[8 * (size_t)i + 3] = 1.0f; rays[8 * (size_t)i + 7] = 0.0f;
			reach[i] = i % 5 == 0 ? INFINITY : (i % 7 == 0 ? NAN : (float)(i % 11) - 2.5f);
		}
		if(w) rays[8 * 2 + 7] = 0.5f;
		memset(hits.data(), 0xab, sizeof(pwn_hit) * (size_t)NMAX);
	};

	// ---- the host form: there and back.  pwn_trace_hits first, so that its buffers stand at the 4096 rays of 80 B it makes them; the
	// same 4096 rays of pwn_trace_reach need 84 B each and have to make them grow
	fill(false);
	REQ(pwn_trace_hits(c, 4096, rays.data(), hits.data()) == PWN_OK);
	REQ(c->hits_cap == 4096 && g_reach_launches == 0 && g_mode == PWN_KM_HITS);
	const int ns[6] = { 3, 4096, 65, NMAX, 7, 1 };
	for(int k = 0; k < 6; k++)
		for(int w = 0; w < 2; w++)
		{
			fill(w != 0);
			const int n = ns[k], before = g_reach_launches, gl = g_launches;
			const size_t cap0 = c->hits_cap;
			REQ(pwn_trace_reach(c, n, rays.data(), reach.data(), hits.data()) == PWN_OK);
			REQ(g_reach_launches == before + 1 && g_launches == gl + 1 && g_mode == (PWN_KM_HITS | PWN_KM_REACH));
			const size_t N = (size_t)n, hoff = (36 * N + 15) & ~(size_t)15;
			REQ(c->hits_cap * 80 + 16 >= hoff + 48 * N && c->hits_cap >= cap0);
			if(n == 4096 && w == 0) REQ(c->hits_cap > 4096);
			REQ(g_P.nrays == (uint32_t)n && g_P.rays == (const float *)c->d_hits && g_P.ray_reach == (const float *)(c->d_hits + 32 * N));
			REQ(g_P.hits == (void *)(c->d_hits + hoff) && g_P.ray_hide == NULL && g_P.ray_seeds == NULL && g_P.sbuf == NULL && g_P.zbuf == NULL);
			REQ(g_P.views == NULL && g_P.vps == NULL && g_P.view_hide == 0);
			const bool ray_w = w != 0 && n > 2;
			REQ(g_P.ray_w == (ray_w ? 1 : 0) && g_P.has_w == (ray_w ? 1 : 0));
			for(int i = 0; i < NMAX; i++)
			{
				uint32_t want[12];
				if(i < n) expect((uint32_t)i, &rays[8 * (size_t)i], reach[i], false, 0, ray_w, want);
				else memset(want, 0xab, sizeof(want));
				REQ(memcmp(&hits[i], want, 48) == 0);
			}
		}
	// (pwn_trace_hits goes on in the grown buffers)
	REQ(pwn_trace_hits(c, NMAX, rays.data(), hits.data()) == PWN_OK && g_mode == PWN_KM_HITS);

	// ---- the device forms: arrays of exactly n entries
	for(int hide = 0; hide < 2; hide++)
		for(int flags = 0; flags < 2; flags++)
		{
			const int n = 257;
			fill(true);
			float *d_rays = NULL, *d_reach = NULL; int32_t *d_hide = NULL; pwn_hit *d_hits = NULL;
			REQ(hipMalloc((void **)&d_rays, 32 * (size_t)n) == hipSuccess && hipMalloc((void **)&d_reach, 4 * (size_t)n) == hipSuccess);
			REQ(hipMalloc((void **)&d_hide, 4 * (size_t)n) == hipSuccess && hipMalloc((void **)&d_hits, 48 * (size_t)n) == hipSuccess);
			memcpy(d_rays, rays.data(), 32 * (size_t)n); memcpy(d_reach, reach.data(), 4 * (size_t)n);
			for(int i = 0; i < n; i++) d_hide[i] = i % 3 == 0 ? PWN_HIDE_NONE : i;
			const int before = g_reach_launches, gl = g_launches;
			if(hide) REQ(pwn_trace_reach_hide_device(c, n, d_rays, d_reach, d_hide, flags ? PWN_RAYS_HAS_W : 0, d_hits, c->stream2) == PWN_OK);
			else REQ(pwn_trace_reach_device(c, n, d_rays, d_reach, flags ? PWN_RAYS_HAS_W : 0, d_hits, c->stream2) == PWN_OK);
			REQ(g_reach_launches == before + 1 && g_launches == gl + 1 && g_mode == (PWN_KM_HITS | PWN_KM_REACH | (hide ? PWN_KM_HIDE : 0)));
			REQ(g_P.rays == d_rays && g_P.ray_reach == d_reach && g_P.hits == (void *)d_hits && g_P.ray_hide == (hide ? d_hide : NULL));
			REQ(g_P.ray_w == flags && g_P.has_w == flags && g_P.nrays == (uint32_t)n);
			for(int i = 0; i < n; i++)
			{
				uint32_t want[12];
				expect((uint32_t)i, &rays[8 * (size_t)i], reach[i], hide != 0, d_hide[i], flags != 0, want);
				REQ(memcmp(&d_hits[i], want, 48) == 0);
			}
			REQ(hipFree(d_rays) == hipSuccess && hipFree(d_reach) == hipSuccess && hipFree(d_hide) == hipSuccess && hipFree(d_hits) == hipSuccess);
		}

	// ---- refusals: nothing launched, nothing written
	fill(false);
	const int n = 70;
	std::vector<int32_t> hide(NMAX, PWN_HIDE_NONE);
	const std::vector<pwn_hit> h0(hits);
	const int before = g_reach_launches, gl = g_launches;
	const float *pr = rays.data(), *pq = reach.data(); pwn_hit *ph = hits.data(); const int32_t *pi = hide.data();
	REQ(((uintptr_t)pr & 15u) == 0 && ((uintptr_t)ph & 15u) == 0);
#define ALL3(code, N, R, Q, H) do { REQ(pwn_trace_reach(ctx, N, R, Q, H) == code); REQ(pwn_trace_reach_device(ctx, N, R, Q, 0, H, NULL) == code); \
	REQ(pwn_trace_reach_hide_device(ctx, N, R, Q, pi, 0, H, NULL) == code); } while(0)
	pwn_ctx *ctxs[3] = { NULL, c, bare };
	for(int k = 0; k < 3; k++)
	{
		pwn_ctx *ctx = ctxs[k];
		ALL3(PWN_EINVAL, -1, pr, pq, ph);
		ALL3(PWN_EINVAL, PWN_RAYS_MAX + 1, pr, pq, ph);
		ALL3(PWN_EINVAL, n, NULL, pq, ph);
		ALL3(PWN_EINVAL, n, pr, NULL, ph);
		ALL3(PWN_EINVAL, n, pr, pq, NULL);
		ALL3(PWN_EINVAL, n, pr, (const float *)((const char *)pq + 2), ph);                        // reach misaligned
		if(ctx == NULL) continue;
		REQ(pwn_trace_reach_device(ctx, n, pr, pq, 2, ph, NULL) == PWN_EINVAL);                   // a flag that is none
		REQ(pwn_trace_reach_hide_device(ctx, n, pr, pq, pi, ~PWN_RAYS_HAS_W, ph, NULL) == PWN_EINVAL);
		REQ(pwn_trace_reach_device(ctx, n, pr + 1, pq, 0, ph, NULL) == PWN_EINVAL);               // records misaligned
		REQ(pwn_trace_reach_device(ctx, n, pr, pq, 0, (char *)ph + 4, NULL) == PWN_EINVAL);       // hits misaligned
		REQ(pwn_trace_reach_hide_device(ctx, n, pr + 2, pq, pi, 0, ph, NULL) == PWN_EINVAL);
		REQ(pwn_trace_reach_hide_device(ctx, n, pr, pq, pi, 0, (char *)ph + 8, NULL) == PWN_EINVAL);
		REQ(pwn_trace_reach_hide_device(ctx, n, pr, pq, NULL, 0, ph, NULL) == PWN_EINVAL);         // hide NULL, misaligned
		REQ(pwn_trace_reach_hide_device(ctx, n, pr, pq, (const int32_t *)((const char *)pi + 1), 0, ph, NULL) == PWN_EINVAL);
		// the overlap rules: reach and hide against the n x 48 bytes of hits, at both ends and inside
		const float *in_hits[3] = { (const float *)ph, (const float *)((const char *)ph + 48 * n - 4), (const float *)((const char *)ph - 4 * n + 4) };
		for(int q = 0; q < 3; q++)
		{
			REQ(pwn_trace_reach_device(ctx, n, pr, in_hits[q], 0, ph, NULL) == PWN_EINVAL);
			REQ(pwn_trace_reach_hide_device(ctx, n, pr, in_hits[q], pi, 0, ph, NULL) == PWN_EINVAL);
			REQ(pwn_trace_reach_hide_device(ctx, n, pr, pq, (const int32_t *)in_hits[q], 0, ph, NULL) == PWN_EINVAL);
		}
	}
	{
		pwn_ctx *ctx = bare;
		ALL3(PWN_ENOLEVEL, n, pr, pq, ph);
		ALL3(PWN_ENOLEVEL, 0, NULL, NULL, NULL);
		ctx = c;
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		ALL3(PWN_EBUSY, n, pr, pq, ph);
		c->tiled = NULL;
		// the empty batch: PWN_OK once the checks pass, every array may be NULL
		ALL3(PWN_OK, 0, NULL, NULL, NULL);
		REQ(pwn_trace_reach_hide_device(ctx, 0, NULL, NULL, NULL, 0, NULL, NULL) == PWN_OK);
		// arrays that touch without overlapping are taken: reach right behind the records written, hide right in front of them
		std::vector<unsigned char> blk(4 * n + 48 * n + 4 * n + 16);
		unsigned char *b = (unsigned char *)(((uintptr_t)blk.data() + 15) & ~(uintptr_t)15);
		const int l0 = g_reach_launches;
		int32_t *hd = (int32_t *)(b + 16 * ((4 * n + 15) / 16) - 4 * n);
		for(int i = 0; i < n; i++) hd[i] = PWN_HIDE_NONE;
		unsigned char *hh = b + 16 * ((4 * n + 15) / 16);
		memcpy(hh + 48 * n, pq, 4 * n);
		REQ(pwn_trace_reach_hide_device(ctx, n, pr, hh + 48 * n, hd, 0, hh, NULL) == PWN_OK);
		REQ(g_reach_launches == l0 + 1 && g_mode == (PWN_KM_HITS | PWN_KM_HIDE | PWN_KM_REACH));
		g_reach_launches = l0; g_launches--;
	}
	// ---- a group's handle (pwn_init_multi): PWN_ENOTSUP from all three, whatever else is right or wrong with the call
	{
		const int devs[2] = { 0, 0 };
		pwn_ctx *ctx = NULL;
		REQ(pwn_init_multi(&ctx, devs, 2, 32, 16) == PWN_OK);
		REQ(pwn_level_load(ctx, argv[1]) == PWN_OK);
		ALL3(PWN_ENOTSUP, n, pr, pq, ph);
		ALL3(PWN_ENOTSUP, 0, NULL, NULL, NULL);
		ALL3(PWN_ENOTSUP, -1, pr, pq, ph);
		pwn_destroy(ctx);
	}
	REQ(g_reach_launches == before && g_launches == gl);
	REQ(memcmp(hits.data(), h0.data(), sizeof(pwn_hit) * (size_t)NMAX) == 0);

	pwn_destroy(bare);
	pwn_destroy(c);
	printf("ok\n");
	return 0;
}
