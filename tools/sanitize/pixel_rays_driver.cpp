// pixel_rays_driver.cpp -- the host side of pwn_pixel_rays_device on the CPU, under AddressSanitizer + UBSan: pwn_pixel_rays.cpp against
// the stand-in runtime and stand-ins for its two launches (fake_kernels.cpp), which read every record and pixel pair of the ranges they are
// handed and write every byte of the output ranges and no other ("device" memory is malloc'ed to the byte: a range that is too long
// or a pointer that is off is a report).  What is looked at: what the two launches are handed in both layouts of the pixels and for
// the whole frame, with and without seeds; that the layouts agree with each other; every refusal with nothing launched and nothing
// written; PWN_OK before a level; pwn_stats and pwn_launch_order_waits as they were; no leak behind pwn_destroy.
//     pixel_rays_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)
struct seen { const void *src, *dst; size_t sizes[5]; };
static int g_setups, g_rays, g_other;
static seen g_setup, g_ray;
static void on_launch(const char *name, const void *src, const void *dst, int ns, const size_t *sizes)
{
	seen s = { src, dst, { 0, 0, 0, 0, 0 } };
	for(int i = 0; i < ns && i < 5; i++) s.sizes[i] = sizes[i];
	if(strcmp(name, "view_setup") == 0) { g_setups++; g_setup = s; }
	else if(strcmp(name, "pixel_rays") == 0) { g_rays++; g_ray = s; }
	else g_other++;
}

static const uint32_t POISON = 0xffffffffu;      // (the stand-in's ray words are below 2^30)
// a "device" array of exactly `words` 32-bit words, poisoned
struct dev
{
	std::vector<uint32_t> v;
	explicit dev(size_t words) : v(words, POISON) {}
	void *p() { return v.empty() ? NULL : (void *)v.data(); }
	bool poisoned() const { for(uint32_t u : v) if(u != POISON) return false; return true; }
	bool written() const { for(uint32_t u : v) if(u == POISON) return false; return true; }
};

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_launch_hook = on_launch;
	pwn_ctx *c = NULL, *bare = NULL;
	REQ(pwn_init(&c, 0, 32, 16) == PWN_OK);
	REQ(pwn_level_load(c, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 32, 16) == PWN_OK);                    // no level: the call needs none
	pwn_stats st0, st1; unsigned long long w0 = 0, w1 = 0;
	REQ(pwn_get_stats(c, &st0) == PWN_OK && pwn_launch_order_waits(c, &w0) == PWN_OK);
	const int other0 = g_other;

	const int W = 48, H = 20;
	const int ns[4] = { 1, 3, 65, 2 }, ms[4] = { 1, 7, 2, W * H };
	for(int k = 0; k < 4; k++)
		for(int pass = 0; pass < 2; pass++)
		{
			pwn_ctx *ctx = pass ? bare : c;
			const int n = ns[k], m = ms[k];
			const size_t T = (size_t)n * m;
			std::vector<float> cams(16 * (size_t)n);
			for(size_t i = 0; i < cams.size(); i++) cams[i] = (float)(i % 97) * 0.125f - 3.0f;
			// the pixels of every camera (for m == W * H: the frame, row-major), and the same list once per camera
			std::vector<int32_t> one(2 * (size_t)m), all(2 * T);
			for(int j = 0; j < m; j++) { one[2 * j] = m == W * H ? j % W : (j * 5) % W; one[2 * j + 1] = m == W * H ? j / W : (j * 3) % H; }
			for(int i = 0; i < n; i++) memcpy(&all[2 * (size_t)i * m], one.data(), 8 * (size_t)m);
			dev work(20 * (size_t)n), r_sh(8 * T), s_sh(T), r_all(8 * T), s_all(T), r_ns(8 * T);
			int su = g_setups, ra = g_rays;
			// shared pixels, with seeds
			REQ(pwn_pixel_rays_device(ctx, W, H, n, cams.data(), m, one.data(), PWN_PIXELS_SHARED, work.p(), r_sh.p(), s_sh.p(), ctx->stream) == PWN_OK);
			REQ(g_setups == su + 1 && g_rays == ra + 1);
			REQ(g_setup.src == cams.data() && g_setup.dst == work.p() && g_setup.sizes[0] == (size_t)n && g_setup.sizes[1] == (size_t)W && g_setup.sizes[2] == (size_t)H);
			REQ(g_ray.src == work.p() && g_ray.dst == r_sh.p() && g_ray.sizes[0] == T && g_ray.sizes[1] == (size_t)m && g_ray.sizes[2] == 1 && g_ray.sizes[3] == (size_t)W);
			REQ(work.written() && r_sh.written());
			// every camera its own pixels: the same rays
			REQ(pwn_pixel_rays_device(ctx, W, H, n, cams.data(), m, all.data(), 0, work.p(), r_all.p(), s_all.p(), NULL) == PWN_OK);
			REQ(g_setups == su + 2 && g_rays == ra + 2 && g_ray.sizes[2] == 0);
			REQ(r_all.v == r_sh.v && s_all.v == s_sh.v);
			// no seeds
			REQ(pwn_pixel_rays_device(ctx, W, H, n, cams.data(), m, all.data(), 0, work.p(), r_ns.p(), NULL, NULL) == PWN_OK);
			REQ(r_ns.v == r_sh.v);
			// the whole frame
			if(m == W * H)
			{
				dev r_wf(8 * T), s_wf(T);
				REQ(pwn_pixel_rays_device(ctx, W, H, n, cams.data(), m, NULL, PWN_PIXELS_SHARED, work.p(), r_wf.p(), s_wf.p(), NULL) == PWN_OK);
				REQ(r_wf.v == r_sh.v && s_wf.v == s_sh.v);
			}
			// (another camera gives other rays; another frame width too)
			if(n > 1) REQ(memcmp(&r_sh.v[0], &r_sh.v[8 * (size_t)m], 32) != 0);
			dev r_w(8 * T);
			REQ(pwn_pixel_rays_device(ctx, W + 1, H, n, cams.data(), m, one.data(), PWN_PIXELS_SHARED, work.p(), r_w.p(), NULL, NULL) == PWN_OK);
			REQ(r_w.v != r_sh.v);
		}

	// ---- refusals and empty calls: nothing launched, nothing written
	{
		const int n = 5, m = 3;
		const size_t T = (size_t)n * m;
		// one block that holds every range, so that ranges can be made to overlap: cams, xy, work, rays, seeds, each 16-byte aligned
		std::vector<uint32_t> block(16 * n + 2 * T + 4 + 20 * n + 8 * T + T + 8, POISON);
		uint32_t *base = block.data();
		REQ(((uintptr_t)base & 15u) == 0);
		float *pc = (float *)base; int32_t *px = (int32_t *)(base + 16 * n);
		uint32_t *pw = base + 16 * n + ((2 * T + 3) & ~(size_t)3), *pr = pw + 20 * n, *ps = pr + 8 * T;
		REQ(((uintptr_t)pw & 15u) == 0 && ((uintptr_t)pr & 15u) == 0);
		const std::vector<uint32_t> block0(block);
		const int su = g_setups, ra = g_rays;
		pwn_ctx *ctxs[3] = { NULL, c, bare };
		for(int k = 0; k < 3; k++)
		{
			pwn_ctx *ctx = ctxs[k];
#define CALL(Wd, Ht, N, C, M, X, F, Wk, R, S) pwn_pixel_rays_device(ctx, Wd, Ht, N, C, M, X, F, Wk, R, S, NULL)
			REQ(CALL(0, 16, n, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32769, 16, n, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 0, n, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 32769, n, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, -1, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, PWN_PLAYERS_MAX + 1, pc, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, -1, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, PWN_PLAYERS_MAX, pc, 257, px, PWN_PIXELS_SHARED, pw, pr, ps) == PWN_EINVAL);          // n x m = 2^28 + 2^20
			REQ(CALL(32, 16, 1 << 16, pc, 1 << 16, px, PWN_PIXELS_SHARED, pw, pr, ps) == PWN_EINVAL);              // n x m = 2^32: 64 bits
			REQ(CALL(32, 16, n, pc, m, px, 2, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, PWN_PIXELS_SHARED | 4, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, NULL, m, px, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, 0, NULL, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, NULL, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, NULL, 0, pw, pr, ps) == PWN_EINVAL);                                        // no pixels: not the whole frame
			REQ(CALL(32, 16, n, pc, m, NULL, PWN_PIXELS_SHARED, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(3, 1, n, pc, m, NULL, 0, pw, pr, ps) == PWN_EINVAL);                                          // ... the whole frame is shared
			if(ctx == NULL) continue;
			REQ(CALL(32, 16, n, pc + 1, m, px, 0, pw, pr, ps) == PWN_EINVAL);                                      // misaligned
			REQ(CALL(32, 16, n, pc, m, px + 1, 0, pw, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, 0, pw + 2, pr, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, pr + 1, ps) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, pr, (char *)ps + 2) == PWN_EINVAL);
			REQ(CALL(32, 16, n, pc, m, pc + 16 * n - 2, 0, pw, pr, ps) == PWN_EINVAL);                             // ranges overlap: xy in cams
			REQ(CALL(32, 16, n, pc, m, px, 0, pc + 16 * (n - 1), pr, ps) == PWN_EINVAL);                           // work in cams
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, pw + 20 * n - 4, ps) == PWN_EINVAL);                             // rays in work
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, pr, pr + 8 * T - 1) == PWN_EINVAL);                              // seeds in rays
			REQ(CALL(32, 16, n, pc, m, px, 0, pw, pr, px + 2 * T - 1) == PWN_EINVAL);                              // seeds in xy
			REQ(CALL(32, 16, n, pr + 8 * T - 4, m, px, 0, pw, pr, ps) == PWN_EINVAL);                              // cams in rays
			// (shared pixels are m pairs, not n x m: seeds right behind them is no overlap, but an empty call all the same here)
			REQ(CALL(32, 16, 0, NULL, m, NULL, 0, NULL, NULL, NULL) == PWN_OK);
			REQ(CALL(32, 16, n, NULL, 0, NULL, PWN_PIXELS_SHARED, NULL, NULL, NULL) == PWN_OK);
			REQ(CALL(32, 16, 0, pc, 0, px, 0, pw, pr, ps) == PWN_OK);
		}
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		{ pwn_ctx *ctx = c; REQ(CALL(32, 16, n, pc, m, px, 0, pw, pr, ps) == PWN_EBUSY); REQ(CALL(32, 16, 0, NULL, 0, NULL, 0, NULL, NULL, NULL) == PWN_EBUSY); }
		c->tiled = NULL;
		REQ(g_setups == su && g_rays == ra);
		REQ(block == block0);
		// the same ranges, in order: accepted (shared pixels: seeds may begin right behind the m pairs)
		{ pwn_ctx *ctx = c; REQ(CALL(32, 16, n, pc, m, px, PWN_PIXELS_SHARED, pw, pr, px + 2 * m) == PWN_OK); }
		REQ(g_setups == su + 1 && g_rays == ra + 1);
	}

	REQ(g_other == other0);          // nothing else was launched by any of it

	// a group's handle
	{
		const int devs[2] = { 0, 0 };
		pwn_ctx *g = NULL;
		REQ(pwn_init_multi(&g, devs, 2, 32, 16) == PWN_OK);
		std::vector<float> cams(16, 1.0f);
		std::vector<int32_t> xy(2, 0);
		dev work(20), rays(8), seeds(1);
		const int su = g_setups, ra = g_rays;
		REQ(pwn_pixel_rays_device(g, 32, 16, 1, cams.data(), 1, xy.data(), 0, work.p(), rays.p(), seeds.p(), NULL) == PWN_ENOTSUP);
		REQ(g_setups == su && g_rays == ra && work.poisoned() && rays.poisoned() && seeds.poisoned());
		pwn_destroy(g);
	}

	REQ(pwn_get_stats(c, &st1) == PWN_OK && memcmp(&st0, &st1, sizeof(st0)) == 0);          // no counters, no timings
	REQ(pwn_launch_order_waits(c, &w1) == PWN_OK && w0 == w1);
	pwn_destroy(bare);
	pwn_destroy(c);
	printf("ok\n");
	return 0;
}
