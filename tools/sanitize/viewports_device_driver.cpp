// viewports_device_driver.cpp -- the host side of pwn_viewports_layout / pwn_trace_viewports_device on the CPU, under AddressSanitizer +
// UBSan: pwn_viewports_device.cpp against the stand-in runtime and stand-ins for its three kinds of launch (fake_kernels.cpp; the
// set-up launch's stand-in is the algorithm itself, one record after the other).  "Device" memory is malloc'ed to the byte, so a
// pitch, a range or a table that is off is a report.  What is looked at: what the set-up, trace and blur launches are handed (records in
// rising-units order, perm a permutation, pitch = the layout's W, a skip-ahead table long enough for the widest view and with the
// right values, the records of the ticket set the trace launch counts in, over 10 calls on one and on two streams); the records word
// for word against what the host form makes for the same rectangles, cameras and times; no allocation, synchronisation or host wait
// after the first call; every refusal with nothing launched and nothing written; free, and a freed layout refused; 100 layouts
// created and freed; no leak behind pwn_destroy.
//     viewports_device_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);
extern "C" void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern "C" void (*pwn_fake_blur_hook)(const pwn_blur_params *B);
extern "C" void (*pwn_fake_viewport_setup_hook)(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm, const pwn_viewport_rec *out, int n);
extern "C" void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern "C" long fakehip_alloc_fail_in;

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)

static const uint32_t POISON = 0xa5a5a5a5u;
static std::vector<std::string> g_log;            // launches and runtime calls, in order
static int g_setups, g_traces, g_blurs, g_small_other, g_allocs, g_syncs, g_waits, g_event_syncs;
static std::vector<pwn_viewport_rec> g_recs;      // the records the last trace launch was handed
static pwn_trace_params g_P;
static pwn_blur_params g_B;
static std::vector<uint2> g_skip;                 // the last blur launch's table, as far as its widest view reads it
static const pwn_viewport_rec *g_setup_out, *g_setup_master;
static std::vector<uint32_t> g_perm;
static std::vector<pwn_viewport_rec> g_master;
static std::vector<float> g_scal;

static void on_small(const char *name, const void *, const void *, int, const size_t *)
{
	if(strcmp(name, "viewport_setup") == 0) { g_setups++; g_log.push_back("setup"); }
	else if(strcmp(name, "upload") != 0) g_small_other++;
}
static void on_setup(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm, const pwn_viewport_rec *out, int n)
{
	g_setup_out = out; g_setup_master = master;
	g_perm.assign(perm, perm + n); g_master.assign(master, master + n); g_scal.assign(scal, scal + 4 * (size_t)n);
}
static void on_trace(const pwn_trace_params *P, int, size_t)
{
	g_traces++; g_log.push_back("trace"); g_P = *P;
	g_recs.clear();
	if(P->vps != NULL) g_recs.assign(P->vps, P->vps + P->nvp);
}
static void on_blur(const pwn_blur_params *B)
{
	g_blurs++; g_log.push_back("blur"); g_B = *B;
	g_skip.clear();
	int wide = 0;
	for(int i = 0; i < B->nvp; i++) if(B->vps[i].w > wide) wide = B->vps[i].w;
	if(B->vps != NULL) g_skip.assign(B->skip, B->skip + wide / 4 + 1);        // (a table that is too short is a report here)
}
static void on_call(const char *name, const void *, const void *, size_t)
{
	if(strcmp(name, "hipMalloc") == 0 || strcmp(name, "hipHostMalloc") == 0) g_allocs++;
	else if(strcmp(name, "hipDeviceSynchronize") == 0 || strcmp(name, "hipStreamSynchronize") == 0) g_syncs++;
	else if(strcmp(name, "hipEventSynchronize") == 0) { g_event_syncs++; g_log.push_back("eventsync"); }
	else if(strcmp(name, "hipStreamWaitEvent") == 0) { g_waits++; g_log.push_back("wait"); }
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

static const pwn_viewport LA[5] = { { 0, 0, 96, 16 }, { 0, 16, 32, 24 }, { 32, 16, 16, 8 }, { 48, 16, 48, 4 }, { 32, 24, 64, 16 } };
static const pwn_viewport LB[5] = { { 0, 0, 37, 21 }, { 37, 0, 33, 5 }, { 37, 5, 1, 1 }, { 38, 5, 20, 12 }, { 3, 21, 17, 12 } };

// one call of layout l (n rectangles vp of a W x H frame) on context c against the host form on `ruler` (a context of W x H)
static void check_call(pwn_ctx *c, pwn_ctx *ruler, pwn_vp_layout *l, int W, int H, int n, const pwn_viewport *vp, int blur, int salt, hipStream_t s)
{
	std::vector<float> cams, secs;
	make_cams(cams, secs, n, salt);
	const size_t plane = (size_t)W * H;
	dev sb(plane), zb(plane), wk(plane);
	memset(zb.q, 0, plane * 4);
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, blur) == PWN_OK && pwn_set_option(ruler, PWN_OPT_BLUR_PASSES, blur) == PWN_OK);
	// the ruler: the host form's records for the same rectangles, cameras and times
	std::vector<uint32_t> hs(plane), hz(plane);
	REQ(pwn_trace_viewports(ruler, n, vp, cams.data(), secs.data(), hs.data(), (float *)hz.data()) == PWN_OK);
	const std::vector<pwn_viewport_rec> want(g_recs);
	const pwn_trace_params RP = g_P;
	const pwn_blur_params RB = g_B;
	REQ((int)want.size() == n);
	const size_t log0 = g_log.size();
	const int su = g_setups, tr = g_traces, bl = g_blurs;
	const unsigned set = c->ticket_set % (2u * (unsigned)c->launch_rot);
	REQ(pwn_trace_viewports_device(c, l, cams.data(), secs.data(), 0, blur ? wk.p() : NULL, sb.p(), zb.p(), s) == PWN_OK);
	REQ(g_setups == su + 1 && g_traces == tr + 1 && g_blurs == bl + blur);
	// the launches in order: set-up, trace, a blur per pass; a wait between streams, where there is one, in front of the set-up
	{
		std::vector<std::string> got;
		for(size_t k = log0; k < g_log.size(); k++) if(g_log[k] != "wait") got.push_back(g_log[k]);
		std::vector<std::string> exp = { "setup", "trace" };
		for(int p = 0; p < blur; p++) exp.push_back("blur");
		REQ(got == exp);
		if(got.size() != g_log.size() - log0) REQ(g_log[log0] == "wait");
	}
	// the set-up: n master records in rising-units order, perm a permutation, the records of the ticket set the launch counts in
	REQ((int)g_perm.size() == n);
	std::vector<int> seen((size_t)n, 0);
	for(int j = 0; j < n; j++) { REQ(g_perm[j] < (uint32_t)n); seen[g_perm[j]]++; }
	for(int j = 0; j < n; j++) REQ(seen[j] == 1);
	for(int j = 1; j < n; j++) REQ(g_master[j - 1].units <= g_master[j].units && (g_master[j - 1].units < g_master[j].units || g_perm[j - 1] < g_perm[j]));
	for(int j = 0; j < n; j++)
	{
		const pwn_viewport &v = vp[g_perm[j]];
		REQ(g_master[j].x == v.x && g_master[j].y == v.y && g_master[j].w == v.w && g_master[j].h == v.h);
		const pwn_setup_scalars S = pwn_frame_setup_scalars(v.w, v.h);
		const float sc[3] = { -S.yrat, S.xsrat, S.ysrat };
		REQ(memcmp(&g_scal[4 * (size_t)j], sc, 12) == 0);
	}
	REQ(g_setup_out == c->d_prec_dev + (size_t)set * PWN_VIEWS_MAX && g_P.vps == g_setup_out);
	REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
	// the trace launch: pitch and height of the LAYOUT's frame, the units of all views, the caller's planes
	REQ(g_P.w == W && g_P.h == H && g_P.y0 == 0 && g_P.y1 == H && g_P.nvp == n);
	REQ(g_P.tiles_total == RP.tiles_total && g_P.vp_step0 == RP.vp_step0 && g_P.tiles_x == RP.tiles_x && g_P.ux_magic == RP.ux_magic && g_P.ux_shift == RP.ux_shift);
	REQ(g_P.has_w == 0 && g_P.views == NULL && g_P.rays == NULL);
	REQ(g_P.sbuf == ((blur & 1) ? wk.q : sb.q) && g_P.zbuf == (float *)zb.q);
	// the records word for word against the host form's
	REQ((int)g_recs.size() == n);
	for(int j = 0; j < n; j++) REQ(memcmp(&g_recs[j], &want[j], sizeof(pwn_viewport_rec)) == 0);
	// the blur launches: the frame's size, the layout's table with pwn_init's values, the last pass into d_sbuf
	if(blur)
	{
		REQ(g_B.w == W && g_B.h == H && g_B.groups == W / 4 && g_B.nvp == n && g_B.vp_tiles == RB.vp_tiles);
		REQ(g_B.vps == g_setup_master && g_B.vps != g_P.vps);          // (the rectangles from the layout's own copy, which no later call's set-up writes)
		REQ(g_B.tile_w == RB.tile_w && g_B.tile_h == RB.tile_h);
		REQ(g_B.out == sb.q && g_B.zbuf == (float *)zb.q);
		REQ(g_B.skip != c->d_skip);
		uint32_t A = 1, C = 0;
		for(size_t g = 0; g < g_skip.size(); g++)
		{
			REQ(g_skip[g].x == A && g_skip[g].y == C);
			for(int k = 0; k < 32; k++) { A = (A * 25739u) & 0x7FFFFFFFu; C = (C * 25739u + 4u) & 0x7FFFFFFFu; }
		}
	}
	// (the stand-ins write whole planes of the size they are told: the same words as the host form's frame)
	REQ(memcmp(sb.q, hs.data(), plane * 4) == 0 && memcmp(zb.q, hz.data(), plane * 4) == 0);
}

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_launch_hook = on_small; pwn_fake_trace_hook = on_trace; pwn_fake_blur_hook = on_blur; pwn_fake_viewport_setup_hook = on_setup;
	fakehip_call_hook = on_call;
	pwn_ctx *c = NULL, *rulerA = NULL, *rulerB = NULL, *bare = NULL, *other = NULL;
	REQ(pwn_init(&c, 0, 64, 48) == PWN_OK && pwn_level_load(c, argv[1]) == PWN_OK);              // (deliberately of another size than any layout)
	REQ(pwn_init(&rulerA, 0, 96, 40) == PWN_OK && pwn_level_load(rulerA, argv[1]) == PWN_OK);
	REQ(pwn_init(&rulerB, 0, 70, 33) == PWN_OK && pwn_level_load(rulerB, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 64, 48) == PWN_OK);
	REQ(pwn_init(&other, 0, 64, 48) == PWN_OK && pwn_level_load(other, argv[1]) == PWN_OK);
	pwn_stats st0, st1;
	REQ(pwn_get_stats(c, &st0) == PWN_OK);

	// ---- layouts: what they report; creation needs no level
	pwn_vp_layout *A = NULL, *B = NULL, *bl = NULL;
	unsigned long long info[6];
	REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &A) == PWN_OK && A != NULL);
	REQ(pwn_viewports_layout_info(A, info) == PWN_OK);
	REQ(info[0] == 96 && info[1] == 40 && info[2] == 5 && info[3] == 57 && info[4] == 3648 && info[5] == 1);
	REQ(pwn_viewports_layout(c, 70, 33, 5, LB, &B) == PWN_OK && B != NULL);
	REQ(pwn_viewports_layout_info(B, info) == PWN_OK);
	REQ(info[0] == 70 && info[1] == 33 && info[2] == 5 && info[3] == 18 + 6 + 1 + 6 + 6 && info[4] == 37 * 21 + 33 * 5 + 1 + 20 * 12 + 17 * 12 && info[5] == 0);
	REQ(pwn_viewports_layout(bare, 96, 40, 5, LA, &bl) == PWN_OK && bl != NULL);
	REQ(pwn_viewports_layout_info(NULL, info) == PWN_EINVAL && pwn_viewports_layout_info(A, NULL) == PWN_EINVAL);
	REQ(g_setups == 0 && g_traces == 0 && g_blurs == 0);

	// ---- the first call allocates the records; after it nothing allocates, synchronises or waits on the host
	hipStream_t s2 = NULL;
	REQ(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess);
	REQ(c->d_prec_dev == NULL);
	check_call(c, rulerA, A, 96, 40, 5, LA, 1, 0, c->stream);
	REQ(c->d_prec_dev != NULL);
	// ten calls on one stream: the sets in turn (check_call), no wait between streams
	for(int k = 0; k < 10; k++)
	{
		const int w0 = g_waits;
		check_call(c, rulerA, A, 96, 40, 5, LA, k % 3, 1 + k, c->stream);
		REQ(g_waits == w0);
	}
	{
		// the device form by itself: no allocation, no synchronisation, no event wait on the host, no wait between the streams
		std::vector<float> cams, secs;
		const size_t plane = 96 * 40;
		dev sb(plane), zb(plane), wk(plane);
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 2) == PWN_OK);
		const int a0 = g_allocs, s0 = g_syncs, e0 = g_event_syncs;
		unsigned sets_seen = 0;
		for(int k = 0; k < 10; k++)
		{
			make_cams(cams, secs, 5, 40 + k);
			const int w0 = g_waits;
			const unsigned set = c->ticket_set % 4u;
			REQ(pwn_trace_viewports_device(c, A, cams.data(), secs.data(), 0, wk.p(), sb.p(), zb.p(), (k & 1) ? s2 : c->stream) == PWN_OK);
			REQ(g_P.vps == c->d_prec_dev + (size_t)set * PWN_VIEWS_MAX && g_setup_out == g_P.vps);
			REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
			sets_seen |= 1u << set;
			// (ten alternating between two streams: launch n - 2 is on this call's stream -- but for k == 1, the first on s2, which is put
			// behind launch n - 2 before its set-up writes and, by the launcher, before its trace)
			REQ(g_waits - w0 == (k == 1 ? 2 : 0));
		}
		REQ(sets_seen == 0xfu);
		REQ(g_allocs == a0 && g_syncs == s0 && g_event_syncs == e0);
		// a call that leaves the rotation: two in a row on s2 -- behind launch n - 2 ON the stream, before the set-up kernel writes
		REQ(pwn_trace_viewports_device(c, A, cams.data(), secs.data(), 0, wk.p(), sb.p(), zb.p(), c->stream) == PWN_OK);     // (launch n - 2 was on c->stream)
		const size_t log1 = g_log.size();
		REQ(pwn_trace_viewports_device(c, A, cams.data(), secs.data(), 0, wk.p(), sb.p(), zb.p(), c->stream) == PWN_OK);     // (launch n - 2 was on s2)
		REQ(g_log.size() > log1 + 1 && g_log[log1] == "wait" && g_log[log1 + 1] == "setup");
	}

	// ---- layout B (odd widths, a 1 x 1 view, a tie), blur off; one view that is the whole frame
	check_call(c, rulerB, B, 70, 33, 5, LB, 0, 3, c->stream);
	{
		const pwn_viewport whole = { 0, 0, 96, 40 };
		pwn_vp_layout *Cw = NULL;
		REQ(pwn_viewports_layout(c, 96, 40, 1, &whole, &Cw) == PWN_OK);
		check_call(c, rulerA, Cw, 96, 40, 1, &whole, 1, 5, s2);
		REQ(pwn_viewports_layout_free(c, Cw) == PWN_OK);
	}

	// ---- refusals: nothing launched, nothing written
	{
		const size_t plane = 96 * 40;
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 9);
		dev blk(3 * plane + 8);
		uint32_t *sb = blk.q, *zb = blk.q + plane, *wk = blk.q + 2 * plane;
		const int su = g_setups, tr = g_traces, bu = g_blurs, so = g_small_other;
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 1) == PWN_OK);
#define CALL(ctx, L, C, S, F, Wk, Sb, Zb) pwn_trace_viewports_device(ctx, L, C, S, F, Wk, Sb, Zb, NULL)
		REQ(CALL(NULL, A, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, NULL, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, NULL, secs.data(), 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), NULL, 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, NULL, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb, NULL) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, NULL, sb, zb) == PWN_EINVAL);                        // blur on, no work plane
		REQ(CALL(c, bl, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EINVAL);                         // another context's layout
		REQ(CALL(other, A, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 2, wk, sb, zb) == PWN_EINVAL);                          // other flags
		REQ(CALL(c, A, cams.data(), secs.data(), PWN_VIEWS_HAS_W | 4, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data() + 1, secs.data(), 0, wk, sb, zb) == PWN_EINVAL);                      // misaligned
		REQ(CALL(c, A, cams.data(), secs.data() + 1, 0, wk, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk + 1, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb + 2, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb, zb + 3) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb, sb) == PWN_EINVAL);                          // planes overlap
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb + 4, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, zb + plane - 4, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, sb + plane - 4, sb, zb) == PWN_EINVAL);
		REQ(CALL(c, B, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EINVAL);                          // blur on, a layout that is not usable with it
		REQ(CALL(bare, bl, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(g_setups == su && g_traces == tr && g_blurs == bu && g_small_other == so && blk.poisoned());
		// the same ranges back to back: accepted; with blur off the work plane may be missing and the planes' rule still holds
		REQ(CALL(c, A, cams.data(), secs.data(), 0, wk, sb, zb) == PWN_OK);
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, NULL, sb, zb) == PWN_OK);
		REQ(CALL(c, A, cams.data(), secs.data(), 0, NULL, sb, sb + 16) == PWN_EINVAL);
		REQ(g_setups == su + 2);
#undef CALL
	}

	// ---- layout creation: what pwn_viewports_plan refuses, a NULL out, no memory
	{
		pwn_vp_layout *x = (pwn_vp_layout *)(uintptr_t)8;
		const pwn_viewport over[2] = { { 0, 0, 20, 20 }, { 19, 19, 4, 4 } }, outside = { 90, 0, 8, 8 }, empty = { 0, 0, 0, 4 };
		std::vector<pwn_viewport> many(PWN_VIEWS_MAX + 1);
		for(size_t i = 0; i < many.size(); i++) many[i] = pwn_viewport{ (int32_t)(i % 64), (int32_t)(i / 64), 1, 1 };
		REQ(pwn_viewports_layout(c, 96, 40, 2, over, &x) == PWN_EINVAL && x == NULL);
		REQ(pwn_viewports_layout(c, 96, 40, 1, &outside, &x) == PWN_EINVAL && x == NULL);
		REQ(pwn_viewports_layout(c, 96, 40, 1, &empty, &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 96, 40, 0, LA, &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 96, 40, PWN_VIEWS_MAX + 1, many.data(), &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 0, 40, 5, LA, &x) == PWN_EINVAL && pwn_viewports_layout(c, 96, 32769, 5, LA, &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 96, 40, 5, NULL, &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, NULL) == PWN_EINVAL);
		REQ(pwn_viewports_layout(NULL, 96, 40, 5, LA, &x) == PWN_EINVAL);
		REQ(pwn_viewports_layout(c, 64, 17, PWN_VIEWS_MAX, many.data(), &x) == PWN_OK && x != NULL);      // (the limit itself is fine)
		REQ(pwn_viewports_layout_free(c, x) == PWN_OK);
		fakehip_alloc_fail_in = 1;
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &x) == PWN_ENOMEM && x == NULL);
		fakehip_alloc_fail_in = 0;
	}

	// ---- free: behind the event of the last use, then the layout is refused; another context's is refused and stays
	{
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 2);
		const size_t plane = 96 * 40;
		dev sb(plane), zb(plane);
		pwn_vp_layout *F = NULL;
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), c->stream) == PWN_OK);
		REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), s2) == PWN_OK);
		REQ(pwn_viewports_layout_free(other, F) == PWN_EINVAL && pwn_viewports_layout_free(NULL, F) == PWN_EINVAL && pwn_viewports_layout_free(c, NULL) == PWN_EINVAL);
		const size_t log0 = g_log.size();
		const int e0 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK);
		REQ(g_event_syncs == e0 + 2);                    // one per stream it was used on
		REQ(g_log.size() >= log0 + 3 && g_log[log0] == "eventsync" && g_log[log0 + 1] == "eventsync" && g_log[log0 + 2] == "free");
		const int su = g_setups;
		sb.fill(); zb.fill();
		REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), c->stream) == PWN_EINVAL);
		REQ(pwn_viewports_layout_free(c, F) == PWN_EINVAL);
		REQ(g_setups == su && sb.poisoned() && zb.poisoned());
		// a layout that was never used is freed without a wait
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		const int e1 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK && g_event_syncs == e1);
		for(int k = 0; k < 100; k++)
		{
			REQ(pwn_viewports_layout(c, 96, 40, 1 + k % 5, LA, &F) == PWN_OK);
			if(k % 3 == 0) REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), (k & 1) ? s2 : c->stream) == PWN_OK);
			REQ(pwn_viewports_layout_free(c, F) == PWN_OK);
		}
		// more streams than a layout has entries for: the fifth takes over the oldest, behind its record on the device
		hipStream_t more[5];
		for(int k = 0; k < 5; k++) REQ(hipStreamCreateWithFlags(&more[k], hipStreamNonBlocking) == hipSuccess);
		REQ(pwn_viewports_layout(c, 96, 40, 5, LA, &F) == PWN_OK);
		for(int k = 0; k < 5; k++) REQ(pwn_trace_viewports_device(c, F, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), more[k]) == PWN_OK);
		const int e2 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK && g_event_syncs == e2 + 4);
		for(int k = 0; k < 5; k++) REQ(hipStreamDestroy(more[k]) == hipSuccess);
	}

	// ---- a group's handle
	{
		const int devs[2] = { 0, 0 };
		pwn_ctx *g = NULL;
		pwn_vp_layout *x = NULL;
		REQ(pwn_init_multi(&g, devs, 2, 32, 16) == PWN_OK);
		std::vector<float> cams, secs;
		make_cams(cams, secs, 5, 1);
		dev sb(96 * 40), zb(96 * 40);
		const int su = g_setups;
		REQ(pwn_viewports_layout(g, 96, 40, 5, LA, &x) == PWN_ENOTSUP && x == NULL);
		REQ(pwn_trace_viewports_device(g, A, cams.data(), secs.data(), 0, NULL, sb.p(), zb.p(), NULL) == PWN_ENOTSUP);
		REQ(g_setups == su && sb.poisoned() && zb.poisoned());
		pwn_destroy(g);
	}

	REQ(g_small_other == 0);                               // nothing else was launched by any of it
	REQ(pwn_get_stats(c, &st1) == PWN_OK && memcmp(&st0, &st1, sizeof(st0)) == 0);          // no counters, no timings
	REQ(c->d_ppre == NULL && c->d_pz == NULL && c->d_vrec_dev == NULL && c->views_cap == 0);     // the host form's planes, the view slots: never made
	REQ(hipStreamDestroy(s2) == hipSuccess);
	// A, B and bl are still alive: pwn_destroy frees what is left (the leak check at exit says so)
	pwn_destroy(other); pwn_destroy(bare); pwn_destroy(rulerB); pwn_destroy(rulerA); pwn_destroy(c);
	printf("ok\n");
	return 0;
}
