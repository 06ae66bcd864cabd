// viewport_hits_driver.cpp -- the host side of pwn_trace_viewport_hits / pwn_trace_viewport_hits_device on the CPU, under
// AddressSanitizer + UBSan: pwn_calls.cpp and pwn_viewports_device.cpp against the stand-in runtime and the stand-in launches
// (fake_kernels.cpp: the trace launch's writes a word per pixel of every rectangle in every plane it is handed, and nothing else).
// "Device" memory is malloc'ed to the byte, so a pitch, a range or a plane that is off is a report.  What is looked at: what each launch
// is handed (the records byte for byte the colour call's for the same rectangles and cameras, but for the time; the three plane
// pointers); 0 outside the rectangles from the host form, nothing written there by the device form; the staging as it grows; planes
// left out; the ticket sets over calls on one and on two streams, mixed with pwn_trace_viewports_device calls of the same layout; no
// allocation, synchronisation or host wait after the first device call; every refusal with nothing launched or written;
// pwn_viewports_layout_free waiting for a hits call's use; no leak behind pwn_destroy.
//     viewport_hits_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);
extern "C" void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern "C" void (*pwn_fake_blur_hook)(const pwn_blur_params *B);
extern "C" void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern "C" long fakehip_alloc_fail_in;

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)

static const uint32_t POISON = 0xa5a5a5a5u;
static std::vector<std::string> g_log;            // launches and runtime calls, in order
static int g_setups, g_traces, g_blurs, g_small_other, g_allocs, g_syncs, g_waits, g_event_syncs, g_memsets;
static std::vector<pwn_viewport_rec> g_recs;      // the records the last trace launch was handed
static pwn_trace_params g_P;

static void on_small(const char *name, const void *, const void *, int, const size_t *)
{
	if(strcmp(name, "viewport_setup") == 0) { g_setups++; g_log.push_back("setup"); }
	else if(strcmp(name, "upload") != 0) g_small_other++;
}
static void on_trace(const pwn_trace_params *P, int, size_t)
{
	g_traces++; g_log.push_back("trace"); g_P = *P;
	g_recs.clear();
	if(P->vps != NULL) g_recs.assign(P->vps, P->vps + P->nvp);
}
static void on_blur(const pwn_blur_params *) { g_blurs++; g_log.push_back("blur"); }
static const void *g_rec_ev, *g_rec_stream;      // the last event recorded and the stream it was recorded on
static std::vector<const void *> g_synced;        // the events waited for on the host, in order
static void on_call(const char *name, const void *a, const void *b, size_t)
{
	if(strcmp(name, "hipEventRecord") == 0) { g_rec_ev = a; g_rec_stream = b; }
	if(strcmp(name, "hipEventSynchronize") == 0) g_synced.push_back(a);
	if(strcmp(name, "hipMalloc") == 0 || strcmp(name, "hipHostMalloc") == 0) g_allocs++;
	else if(strcmp(name, "hipDeviceSynchronize") == 0 || strcmp(name, "hipStreamSynchronize") == 0) g_syncs++;
	else if(strcmp(name, "hipEventSynchronize") == 0) { g_event_syncs++; g_log.push_back("eventsync"); }
	else if(strcmp(name, "hipStreamWaitEvent") == 0) { g_waits++; g_log.push_back("wait"); }
	else if(strcmp(name, "hipMemsetAsync") == 0) g_memsets++;
	else if(strcmp(name, "hipFree") == 0) g_log.push_back("free");
}

// a "device" array of exactly `words` 32-bit words, 16-byte aligned, poisoned
struct dev
{
	uint32_t *q; size_t words;
	explicit dev(size_t w) : q(NULL), words(w) { REQ(posix_memalign((void **)&q, 16, w ? w * 4 : 16) == 0); fill(); }
	~dev() { free(q); }
	void fill() { for(size_t i = 0; i < words; i++) q[i] = POISON; }
	void *p() { return q; }
	bool poisoned() const { for(size_t i = 0; i < words; i++) if(q[i] != POISON) return false; return true; }
};

static void make_cams(std::vector<float> &cams, std::vector<float> &secs, int n, int salt)
{
	cams.resize(16 * (size_t)n); secs.resize((size_t)n);
	for(size_t i = 0; i < cams.size(); i++) cams[i] = (float)((i * 7 + (size_t)salt * 13) % 97) * 0.125f - 3.0f + 1.0f / (float)(3 + salt);
	for(int i = 0; i < n; i++) secs[i] = 0.5f * (float)(i + 1) + (float)salt;
}

static const pwn_viewport LA[5] = { { 0, 0, 96, 16 }, { 0, 16, 32, 24 }, { 32, 16, 16, 8 }, { 48, 16, 48, 4 }, { 32, 24, 64, 16 } };     // (covers 96 x 40 but 16 x 8 + 48 x 4: uncovered area)
static const pwn_viewport LB[5] = { { 0, 0, 37, 21 }, { 37, 0, 33, 5 }, { 37, 5, 1, 1 }, { 38, 5, 20, 12 }, { 3, 21, 17, 12 } };

static bool inside(int n, const pwn_viewport *vp, int x, int y)
{
	for(int i = 0; i < n; i++) if(x >= vp[i].x && x < vp[i].x + vp[i].w && y >= vp[i].y && y < vp[i].y + vp[i].h) return true;
	return false;
}

// the colour call's records for these rectangles and cameras on `ruler` (a context of W x H), their times set to 0
static std::vector<pwn_viewport_rec> colour_recs(pwn_ctx *ruler, int W, int H, int n, const pwn_viewport *vp, const std::vector<float> &cams, const std::vector<float> &secs)
{
	std::vector<uint32_t> hs((size_t)W * H);
	REQ(pwn_set_option(ruler, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
	REQ(pwn_trace_viewports(ruler, n, vp, cams.data(), secs.data(), hs.data(), NULL) == PWN_OK);
	std::vector<pwn_viewport_rec> want(g_recs);
	REQ((int)want.size() == n);
	for(int j = 0; j < n; j++) { REQ(want[j].sec_current != 0.0f); want[j].sec_current = 0.0f; }
	return want;
}

// one call of the device form of layout l on c: what the launches are handed, what is written
static void check_device(pwn_ctx *c, pwn_ctx *ruler, pwn_vp_layout *l, int W, int H, int n, const pwn_viewport *vp, int mask, int salt, hipStream_t s)
{
	std::vector<float> cams, secs;
	make_cams(cams, secs, n, salt);
	const std::vector<pwn_viewport_rec> want = colour_recs(ruler, W, H, n, vp, cams, secs);
	const pwn_trace_params RP = g_P;
	const size_t plane = (size_t)W * H;
	dev lb(plane), cl(plane), ds(plane);
	const size_t log0 = g_log.size();
	const int su = g_setups, tr = g_traces, bl = g_blurs, ms = g_memsets;
	const unsigned set = c->ticket_set % (2u * (unsigned)c->launch_rot);
	REQ(pwn_trace_viewport_hits_device(c, l, cams.data(), 0, lb.p(), (mask & 1) ? cl.p() : NULL, (mask & 2) ? ds.p() : NULL, s) == PWN_OK);
	// one set-up launch and one trace launch, nothing else (a wait between streams, where there is one, in front of the set-up)
	REQ(g_setups == su + 1 && g_traces == tr + 1 && g_blurs == bl && g_memsets == ms);
	{
		std::vector<std::string> got;
		for(size_t k = log0; k < g_log.size(); k++) if(g_log[k] != "wait") got.push_back(g_log[k]);
		REQ(got == (std::vector<std::string>{ "setup", "trace" }));
		if(got.size() != g_log.size() - log0) REQ(g_log[log0] == "wait");
	}
	// the records of the ticket set the launch counts in, byte for byte the colour call's but for the time
	REQ(g_P.vps == c->d_prec_dev + (size_t)set * PWN_VIEWS_MAX);
	REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
	REQ((int)g_recs.size() == n);
	for(int j = 0; j < n; j++) REQ(memcmp(&g_recs[j], &want[j], sizeof(pwn_viewport_rec)) == 0);
	// the launch: the LAYOUT's frame, the colour call's geometry, the three planes where they travel
	REQ(g_P.w == W && g_P.h == H && g_P.y0 == 0 && g_P.y1 == H && g_P.nvp == n && g_P.has_w == 0 && g_P.views == NULL && g_P.rays == NULL);
	REQ(g_P.tiles_total == RP.tiles_total && g_P.vp_step0 == RP.vp_step0 && g_P.tiles_x == RP.tiles_x && g_P.ux_magic == RP.ux_magic && g_P.ux_shift == RP.ux_shift);
	REQ(g_P.hits == lb.q && g_P.sbuf == ((mask & 1) ? cl.q : NULL) && g_P.zbuf == ((mask & 2) ? (float *)ds.q : NULL));
	// every word of every rectangle in every plane given, nothing outside them, nothing in a plane left out
	for(int y = 0; y < H; y++) for(int x = 0; x < W; x++)
	{
		const size_t o = (size_t)y * W + x;
		const bool in = inside(n, vp, x, y);
		REQ((lb.q[o] != POISON) == in);
		REQ((cl.q[o] != POISON) == (in && (mask & 1)));
		REQ((ds.q[o] != POISON) == (in && (mask & 2)));
		if(in && (mask & 1)) REQ(cl.q[o] == (lb.q[o] ^ 0x11111110u));
	}
}

// one call of the host form on a context of W x H: the records, the planes, 0 outside the rectangles
static void check_host(pwn_ctx *h, int W, int H, int n, const pwn_viewport *vp, int mask, int salt)
{
	std::vector<float> cams, secs;
	make_cams(cams, secs, n, salt);
	const std::vector<pwn_viewport_rec> want = colour_recs(h, W, H, n, vp, cams, secs);
	const pwn_trace_params RP = g_P;
	const size_t plane = (size_t)W * H;
	std::vector<uint32_t> lb(plane + 1, POISON), cl(plane + 1, POISON), ds(plane + 1, POISON);
	const int tr = g_traces, bl = g_blurs, su = g_setups;
	REQ(pwn_trace_viewport_hits(h, n, vp, cams.data(), lb.data(), (mask & 1) ? cl.data() : NULL, (mask & 2) ? (float *)ds.data() : NULL) == PWN_OK);
	REQ(g_traces == tr + 1 && g_blurs == bl && g_setups == su);
	REQ((int)g_recs.size() == n);
	for(int j = 0; j < n; j++) REQ(memcmp(&g_recs[j], &want[j], sizeof(pwn_viewport_rec)) == 0);
	REQ(g_P.w == W && g_P.h == H && g_P.nvp == n && g_P.vps == h->d_prec && g_P.tiles_total == RP.tiles_total && g_P.vp_step0 == RP.vp_step0);
	// the staging: pwn_trace_hits' buffers, 12 B a pixel of W x H
	REQ(h->hits_cap * 80 >= 12 * plane);
	REQ(g_P.hits == h->d_hits && g_P.sbuf == ((mask & 1) ? (uint32_t *)(h->d_hits + 4 * plane) : NULL) && g_P.zbuf == ((mask & 2) ? (float *)(h->d_hits + 8 * plane) : NULL));
	for(int y = 0; y < H; y++) for(int x = 0; x < W; x++)
	{
		const size_t o = (size_t)y * W + x;
		const bool in = inside(n, vp, x, y);
		REQ((lb[o] != 0u) == in);
		if(mask & 1) REQ(in ? cl[o] == (lb[o] ^ 0x11111110u) : cl[o] == 0u); else REQ(cl[o] == POISON);
		if(mask & 2) REQ((ds[o] != 0u) == in); else REQ(ds[o] == POISON);
	}
	REQ(lb[plane] == POISON && cl[plane] == POISON && ds[plane] == POISON);
	pwn_stats st;
	REQ(pwn_get_stats(h, &st) == PWN_OK && st.blur_ms == 0.0f && st.total_ms >= st.trace_ms);
}

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_launch_hook = on_small; pwn_fake_trace_hook = on_trace; pwn_fake_blur_hook = on_blur;
	fakehip_call_hook = on_call;
	pwn_ctx *c = NULL, *rulerA = NULL, *rulerB = NULL, *bare = NULL, *other = NULL, *hostA = NULL, *hostB = NULL;
	REQ(pwn_init(&c, 0, 64, 48) == PWN_OK && pwn_level_load(c, argv[1]) == PWN_OK);              // (deliberately of another size than any layout)
	REQ(pwn_init(&rulerA, 0, 96, 40) == PWN_OK && pwn_level_load(rulerA, argv[1]) == PWN_OK);
	REQ(pwn_init(&rulerB, 0, 70, 33) == PWN_OK && pwn_level_load(rulerB, argv[1]) == PWN_OK);
	REQ(pwn_init(&hostA, 0, 96, 40) == PWN_OK && pwn_level_load(hostA, argv[1]) == PWN_OK);
	REQ(pwn_init(&hostB, 0, 70, 33) == PWN_OK && pwn_level_load(hostB, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 96, 40) == PWN_OK);
	REQ(pwn_init(&other, 0, 64, 48) == PWN_OK && pwn_level_load(other, argv[1]) == PWN_OK);
	pwn_stats st0, st1;
	REQ(pwn_get_stats(c, &st0) == PWN_OK);

	// ---- the host form: every combination of planes, two layouts, one view that is the whole frame; blur passes are ignored
	{
		// (the staging grows from nothing: a small call first on a context of its own, then larger ones)
		const pwn_viewport tiny = { 5, 3, 1, 1 };
		REQ(hostB->hits_cap == 0 && hostB->h_prec == NULL);
		check_host(hostB, 70, 33, 1, &tiny, 3, 1);
		const size_t cap0 = hostB->hits_cap;
		REQ(cap0 * 80 >= 12 * 70 * 33);
		for(int mask = 0; mask < 4; mask++) check_host(hostB, 70, 33, 5, LB, mask, 2 + mask);
		REQ(hostB->hits_cap == cap0);                       // (12 B a pixel of W x H, whatever the rectangles: nothing grew)
		for(int mask = 0; mask < 4; mask++) check_host(hostA, 96, 40, 5, LA, mask, 7 + mask);
		const pwn_viewport whole = { 0, 0, 96, 40 };
		check_host(hostA, 96, 40, 1, &whole, 3, 11);
		REQ(pwn_set_option(hostB, PWN_OPT_BLUR_PASSES, 2) == PWN_OK);          // (a width and rectangles no blur could take)
		{
			std::vector<float> cams, secs;
			make_cams(cams, secs, 5, 3);
			std::vector<uint32_t> lb(70 * 33);
			const int bl = g_blurs;
			REQ(pwn_trace_viewport_hits(hostB, 5, LB, cams.data(), lb.data(), NULL, NULL) == PWN_OK && g_blurs == bl);
		}
		// a larger need of pwn_trace_hits' own grows the same buffers, and the planes still come out right afterwards
		{
			const int nr = 40000;
			std::vector<float> rays(8 * (size_t)nr, 0.0f);
			for(int i = 0; i < nr; i++) { rays[8 * (size_t)i + 0] = 6.5f; rays[8 * (size_t)i + 1] = 0.5f; rays[8 * (size_t)i + 2] = 6.5f; rays[8 * (size_t)i + 3] = 1.0f; rays[8 * (size_t)i + 4] = 1.0f; }
			std::vector<pwn_hit> hits((size_t)nr);
			REQ(pwn_trace_hits(hostB, nr, rays.data(), hits.data()) == PWN_OK);
			REQ(hostB->hits_cap >= (size_t)nr);
			check_host(hostB, 70, 33, 5, LB, 3, 5);
		}
		// the colour call's planes and depth plane were made by the ruler calls of check_host on these contexts; the view slots never
		REQ(hostA->views_cap == 0 && hostA->d_vrec_dev == NULL && hostA->d_prec_dev == NULL);
	}
	// a context that has only ever been asked for first-hit planes owns no colour planes
	{
		pwn_ctx *only = NULL;
		REQ(pwn_init(&only, 0, 96, 40) == PWN_OK && pwn_level_load(only, argv[1]) == PWN_OK);
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 4);
		std::vector<uint32_t> lb(96 * 40);
		REQ(pwn_trace_viewport_hits(only, 5, LA, cams.data(), lb.data(), NULL, NULL) == PWN_OK);
		REQ(only->d_ppre == NULL && only->d_pout == NULL && only->d_pz == NULL && only->h_prec != NULL && only->views_cap == 0 && only->h_rays == NULL);
		// out of memory when the staging has to grow: refused, nothing launched, and the next call is fine
		pwn_ctx *big = NULL;
		REQ(pwn_init(&big, 0, 96, 40) == PWN_OK && pwn_level_load(big, argv[1]) == PWN_OK);
		REQ(pwn_trace_viewport_hits(big, 1, LA, cams.data(), lb.data(), NULL, NULL) == PWN_OK);         // (tables, records)
		pwn_destroy(big);
		REQ(pwn_init(&big, 0, 96, 40) == PWN_OK && pwn_level_load(big, argv[1]) == PWN_OK);
		const int tr = g_traces;
		fakehip_alloc_fail_in = 3;                          // (the records' two allocations pass, the staging's first does not)
		const int rc = pwn_trace_viewport_hits(big, 5, LA, cams.data(), lb.data(), NULL, NULL);
		fakehip_alloc_fail_in = 0;
		REQ(rc == PWN_ENOMEM && g_traces == tr && big->hits_cap == 0);
		REQ(pwn_trace_viewport_hits(big, 5, LA, cams.data(), lb.data(), NULL, NULL) == PWN_OK);
		pwn_destroy(big); pwn_destroy(only);
	}

	// ---- refusals of the host form: nothing launched, nothing written
	{
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 6);
		std::vector<uint32_t> a(96 * 40, POISON), b(96 * 40, POISON);
		const int tr = g_traces, so = g_small_other;
		const pwn_viewport over[2] = { { 0, 0, 20, 20 }, { 19, 19, 4, 4 } }, outside = { 90, 0, 8, 8 }, empty = { 0, 0, 0, 4 };
		REQ(pwn_trace_viewport_hits(NULL, 5, LA, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 5, NULL, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 5, LA, NULL, a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 5, LA, cams.data(), NULL, b.data(), (float *)a.data()) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 0, LA, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, PWN_VIEWS_MAX + 1, LA, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 2, over, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 1, &outside, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(hostA, 1, &empty, cams.data(), a.data(), b.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_viewport_hits(bare, 5, LA, cams.data(), a.data(), b.data(), NULL) == PWN_ENOLEVEL);
		hostA->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(pwn_trace_viewport_hits(hostA, 5, LA, cams.data(), a.data(), b.data(), NULL) == PWN_EBUSY);
		hostA->tiled = NULL;
		REQ(g_traces == tr && g_small_other == so);
		for(size_t o = 0; o < a.size(); o++) REQ(a[o] == POISON && b[o] == POISON);
	}

	// ---- the device form.  The first call allocates the records; after it nothing allocates, synchronises or waits on the host
	pwn_vp_layout *A = NULL, *B = NULL, *bl = NULL;
	REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &A) == PWN_OK && pwn_viewports_layout(c, 70, 33, 5, LB, &B) == PWN_OK);
	REQ(pwn_viewports_layout(bare, 96, 40, 5, LA, &bl) == PWN_OK);
	hipStream_t s2 = NULL;
	REQ(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess);
	REQ(c->d_prec_dev == NULL);
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 2) == PWN_OK);          // (ignored: B is no layout a blur could take)
	check_device(c, rulerA, A, 96, 40, 5, LA, 3, 0, c->stream);
	REQ(c->d_prec_dev != NULL);
	for(int k = 0; k < 10; k++)
	{
		const int w0 = g_waits;
		check_device(c, k & 1 ? rulerB : rulerA, k & 1 ? B : A, k & 1 ? 70 : 96, k & 1 ? 33 : 40, 5, k & 1 ? LB : LA, k % 4, 1 + k, c->stream);
		REQ(g_waits == w0);                                 // (one stream: no wait between streams)
	}
	{
		const pwn_viewport whole = { 0, 0, 96, 40 };
		pwn_vp_layout *Cw = NULL;
		REQ(pwn_viewports_layout(c, 96, 40, 1, &whole, &Cw) == PWN_OK);
		check_device(c, rulerA, Cw, 96, 40, 1, &whole, 3, 5, s2);
		REQ(pwn_viewports_layout_free(c, Cw) == PWN_OK);
	}
	{
		// by itself, two streams alternating, mixed with colour calls of the same layout: the sets in turn, whichever family the call is of
		std::vector<float> cams, secs;
		const size_t plane = 96 * 40;
		dev lb(plane), cl(plane), ds(plane), sb(plane), zb(plane);
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
		make_cams(cams, secs, 5, 30);
		// (two on c->stream first: the launches n - 2 of the loop's first two calls are then on c->stream)
		for(int k = 0; k < 2; k++) REQ(pwn_trace_viewport_hits_device(c, A, cams.data(), 0, lb.p(), cl.p(), ds.p(), c->stream) == PWN_OK);
		const int a0 = g_allocs, s0 = g_syncs, e0 = g_event_syncs;
		unsigned sets_seen = 0;
		for(int k = 0; k < 12; k++)
		{
			make_cams(cams, secs, 5, 40 + k);
			const int w0 = g_waits;
			const unsigned set = c->ticket_set % 4u;
			hipStream_t s = (k & 1) ? s2 : c->stream;
			if(k % 3 == 2) REQ(pwn_trace_viewports_device(c, A, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), s) == PWN_OK);
			else REQ(pwn_trace_viewport_hits_device(c, A, cams.data(), (k & 2) ? PWN_VIEWS_HAS_W : 0, lb.p(), cl.p(), ds.p(), s) == PWN_OK);
			REQ(g_P.vps == c->d_prec_dev + (size_t)set * PWN_VIEWS_MAX);
			REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
			REQ((g_P.hits != NULL) == (k % 3 != 2));
			if(k % 3 != 2) REQ(g_P.has_w == ((k & 2) ? 1 : 0));
			// (the time a record carries: the colour call's own, 0 for the planes -- also where the set held a colour call's records before)
			for(int j = 0; j < 5; j++) REQ((g_recs[j].sec_current == 0.0f) == (k % 3 != 2));
			sets_seen |= 1u << set;
			// (alternating: launch n - 2 is on this call's stream -- but for k == 1, the first on s2, which is put behind launch n - 2
			// before its set-up writes and, by the launcher, before its trace)
			REQ(g_waits - w0 == (k == 1 ? 2 : 0));
		}
		REQ(sets_seen == 0xfu);
		REQ(g_allocs == a0 && g_syncs == s0 && g_event_syncs == e0);
		// a call that leaves the rotation: two in a row on one stream after an alternation -- behind launch n - 2 before the set-up writes
		REQ(pwn_trace_viewport_hits_device(c, A, cams.data(), 0, lb.p(), NULL, NULL, c->stream) == PWN_OK);      // (launch n - 2 was on c->stream)
		const size_t log1 = g_log.size();
		REQ(pwn_trace_viewport_hits_device(c, A, cams.data(), 0, lb.p(), NULL, NULL, c->stream) == PWN_OK);      // (launch n - 2 was on s2)
		REQ(g_log.size() > log1 + 1 && g_log[log1] == "wait" && g_log[log1 + 1] == "setup");
	}

	// ---- refusals of the device form: nothing launched, nothing written, nothing changed
	{
		const size_t plane = 96 * 40;
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 9);
		dev blk(3 * plane + 8);
		uint32_t *lb = blk.q, *cl = blk.q + plane, *ds = blk.q + 2 * plane;
		const int su = g_setups, tr = g_traces, bu = g_blurs, so = g_small_other, wa = g_waits;
		const unsigned set0 = c->ticket_set;
#define CALL(ctx, L, C, F, Lb, Cl, Ds) pwn_trace_viewport_hits_device(ctx, L, C, F, Lb, Cl, Ds, NULL)
		REQ(CALL(NULL, A, cams.data(), 0, lb, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, NULL, cams.data(), 0, lb, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, NULL, 0, lb, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, NULL, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, bl, cams.data(), 0, lb, cl, ds) == PWN_EINVAL);                          // another context's layout
		REQ(CALL(other, A, cams.data(), 0, lb, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 2, lb, cl, ds) == PWN_EINVAL);                           // other flags
		REQ(CALL(c, A, cams.data(), PWN_VIEWS_HAS_W | 4, lb, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data() + 1, 0, lb, cl, ds) == PWN_EINVAL);                       // misaligned
		REQ(CALL(c, A, cams.data(), 0, lb + 1, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb, cl + 2, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb, cl, ds + 3) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb, lb, ds) == PWN_EINVAL);                           // planes overlap
		REQ(CALL(c, A, cams.data(), 0, lb, cl, cl) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb, cl, lb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb + 4, cl, ds) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, lb, NULL, lb + plane - 4) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), 0, cl + plane - 4, cl, NULL) == PWN_EINVAL);
		REQ(CALL(bare, bl, cams.data(), 0, lb, cl, ds) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(CALL(c, A, cams.data(), 0, lb, cl, ds) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(g_setups == su && g_traces == tr && g_blurs == bu && g_small_other == so && g_waits == wa && c->ticket_set == set0 && blk.poisoned());
		// the same ranges back to back: accepted
		REQ(CALL(c, A, cams.data(), 0, lb, cl, ds) == PWN_OK);
		REQ(g_setups == su + 1 && g_traces == tr + 1);
#undef CALL
	}

	// ---- free waits for a hits call's use, per stream; a freed layout is refused
	{
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 2);
		const size_t plane = 96 * 40;
		dev lb(plane), sb(plane), zb(plane);
		pwn_vp_layout *F = NULL;
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		g_rec_ev = NULL;
		REQ(pwn_trace_viewport_hits_device(c, F, cams.data(), 0, lb.p(), NULL, NULL, c->stream) == PWN_OK);
		// (the last thing the call does: an event of the layout's own behind the trace launch, on the call's stream ...)
		const void *used = g_rec_ev;
		REQ(used != NULL && g_rec_stream == (const void *)c->stream && g_log.back() == "trace");
		for(int k = 0; k < 3; k++) REQ(used != (const void *)c->launch_event[k]);
		const size_t log0 = g_log.size();
		const int e0 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK);
		REQ(g_event_syncs == e0 + 1 && g_synced.back() == used);          // (... which free waits for)
		REQ(g_log.size() >= log0 + 2 && g_log[log0] == "eventsync" && g_log[log0 + 1] == "free");
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		REQ(pwn_trace_viewport_hits_device(c, F, cams.data(), 0, lb.p(), NULL, NULL, c->stream) == PWN_OK);
		REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), s2) == PWN_OK);
		REQ(pwn_trace_viewport_hits_device(c, F, cams.data(), 0, lb.p(), NULL, NULL, s2) == PWN_OK);
		const int e1 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK && g_event_syncs == e1 + 2);          // one per stream it was used on
		const int su = g_setups;
		lb.fill();
		REQ(pwn_trace_viewport_hits_device(c, F, cams.data(), 0, lb.p(), NULL, NULL, c->stream) == PWN_EINVAL);
		REQ(g_setups == su && lb.poisoned());
		// more streams than a layout has entries for: the fifth takes over the oldest, behind its record on the device
		hipStream_t more[5];
		for(int k = 0; k < 5; k++) REQ(hipStreamCreateWithFlags(&more[k], hipStreamNonBlocking) == hipSuccess);
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		for(int k = 0; k < 5; k++) REQ(pwn_trace_viewport_hits_device(c, F, cams.data(), 0, lb.p(), NULL, NULL, more[k]) == PWN_OK);
		const int e2 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK && g_event_syncs == e2 + 4);
		for(int k = 0; k < 5; k++) REQ(hipStreamDestroy(more[k]) == hipSuccess);
	}

	// ---- a group's handle
	{
		const int devs[2] = { 0, 0 };
		pwn_ctx *g = NULL;
		REQ(pwn_init_multi(&g, devs, 2, 96, 40) == PWN_OK);
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 1);
		dev lb(96 * 40);
		const int su = g_setups, tr = g_traces;
		REQ(pwn_trace_viewport_hits_device(g, A, cams.data(), 0, lb.p(), NULL, NULL, NULL) == PWN_ENOTSUP);
		REQ(pwn_trace_viewport_hits(g, 5, LA, cams.data(), lb.q, NULL, NULL) == PWN_ENOTSUP);
		REQ(g_setups == su && g_traces == tr && lb.poisoned());
		pwn_destroy(g);
	}

	REQ(g_small_other == 0);                               // nothing else was launched by any of it
	REQ(pwn_get_stats(c, &st1) == PWN_OK && memcmp(&st0, &st1, sizeof(st0)) == 0);          // the device form: no counters, no timings
	// the host form's planes and staging, the colour call's planes, the view slots: never made by the device form
	REQ(c->d_ppre == NULL && c->d_pz == NULL && c->h_prec == NULL && c->d_vrec_dev == NULL && c->views_cap == 0 && c->hits_cap == 0 && c->h_hits == NULL);
	REQ(hipStreamDestroy(s2) == hipSuccess);
	// A, B and bl are still alive: pwn_destroy frees what is left (the leak check at exit says so)
	pwn_destroy(other); pwn_destroy(bare); pwn_destroy(hostB); pwn_destroy(hostA); pwn_destroy(rulerB); pwn_destroy(rulerA); pwn_destroy(c);
	printf("ok\n");
	return 0;
}
