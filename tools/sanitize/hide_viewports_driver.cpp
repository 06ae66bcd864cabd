// hide_viewports_driver.cpp -- the host side of pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device and
// pwn_trace_rays_hide_device on the CPU, under AddressSanitizer + UBSan: pwn_viewports_device.cpp, pwn_calls.cpp and pwn_launch.cpp
// against the stand-in runtime and the stand-in launches (fake_kernels.cpp), as viewport_hits_driver.cpp runs the calls they shadow.
// "Device" memory is malloc'ed to the byte.  What is looked at: d_hide reaches the set-up launcher and the records carry
// hide[perm[j]] + 1 (0 for a value that is no index); a plain call hands the set-up launcher no array and its records' words are 0,
// also in a record set that held a hide call's before; the trace launch of every call has exactly the call's mode, the HIDE bit for a
// hide call and none for a plain one; every refusal -- NULL, misaligned, overlapping each written range -- with nothing launched and nothing written;
// the ticket sets over mixed plain and hide calls on one and on two streams; no allocation, synchronisation or host wait after the
// first device call; the layout-use event of a hide call, which pwn_viewports_layout_free waits for; the rays' call: the array in the
// launch's parameters, the empty batch, refusals; a group's handle; no leak behind pwn_destroy.
//     hide_viewports_asan LEVEL.txt        prints "ok"
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);
extern "C" void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern "C" void (*pwn_fake_blur_hook)(const pwn_blur_params *B);
extern "C" void (*pwn_fake_viewport_hide_hook)(const int32_t *hide, int n);
extern "C" void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern "C" thread_local int pwn_fake_trace_mode;

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)

static const uint32_t POISON = 0xa5a5a5a5u;
static std::vector<std::string> g_log;
static int g_setups, g_traces, g_blurs, g_small_other, g_allocs, g_syncs, g_waits, g_event_syncs;
static std::vector<pwn_viewport_rec> g_recs;      // the records the last trace launch was handed
static pwn_trace_params g_P;
static int g_mode = -1;                           // the mode of the last trace launch
static const int32_t *g_hide_seen;                // the array the last set-up launch was handed (NULL: none)
static int g_hide_n, g_hide_calls;

static void on_small(const char *name, const void *, const void *, int, const size_t *)
{
	if(strcmp(name, "viewport_setup") == 0) { g_setups++; g_hide_seen = NULL; g_hide_n = 0; g_log.push_back("setup"); }
	else if(strcmp(name, "upload") != 0) g_small_other++;
}
static void on_hide(const int32_t *hide, int n) { g_hide_seen = hide; g_hide_n = n; g_hide_calls++; }
static void on_trace(const pwn_trace_params *P, int, size_t)
{
	g_traces++; g_log.push_back("trace"); g_P = *P; g_mode = pwn_fake_trace_mode;
	g_recs.clear();
	if(P->vps != NULL) g_recs.assign(P->vps, P->vps + P->nvp);
}
static void on_blur(const pwn_blur_params *) { g_blurs++; g_log.push_back("blur"); }
static const void *g_rec_ev, *g_rec_stream;
static std::vector<const void *> g_synced;
static void on_call(const char *name, const void *a, const void *b, size_t)
{
	if(strcmp(name, "hipEventRecord") == 0) { g_rec_ev = a; g_rec_stream = b; }
	if(strcmp(name, "hipEventSynchronize") == 0) g_synced.push_back(a);
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

// 96 x 40, usable with blur; the units are 21, 16, 18 and 1: the records' order is not the caller's
static const int NV = 4, W = 96, H = 40;
static const pwn_viewport HV[NV] = { { 0, 0, 40, 26 }, { 40, 0, 56, 16 }, { 0, 26, 96, 12 }, { 40, 16, 4, 4 } };

static uint32_t word_of(int32_t k) { return k >= 0 && k < PWN_OBJ_MAX ? (uint32_t)k + 1u : 0u; }
// the records the last trace launch was handed carry, each, the word of the RECTANGLE it stands for (hide NULL: 0 everywhere)
static void check_words(const int32_t *hide)
{
	REQ((int)g_recs.size() == NV);
	bool in_order = true;
	for(int j = 0; j < NV; j++)
	{
		int i = -1;
		for(int k = 0; k < NV; k++) if(g_recs[j].x == HV[k].x && g_recs[j].y == HV[k].y && g_recs[j].w == HV[k].w && g_recs[j].h == HV[k].h) i = k;
		REQ(i >= 0);
		if(i != j) in_order = false;
		REQ(g_recs[j].hide == (hide != NULL ? word_of(hide[i]) : 0u));
		REQ(g_recs[j].pad_ == 0u);
	}
	REQ(!in_order);                                   // (the layout exercises perm)
}

enum { PLAIN_COL, HIDE_COL, PLAIN_HITS, HIDE_HITS };
struct planes { dev a, b, d; planes() : a((size_t)W * H), b((size_t)W * H), d((size_t)W * H) {} };
// one call of a kind on layout l; what the launches were handed
static void one_call(pwn_ctx *c, pwn_vp_layout *l, int kind, const int32_t *hide, int salt, hipStream_t s, planes &pl, int blur)
{
	std::vector<float> cams, secs;
	make_cams(cams, secs, NV, salt);
	const int su = g_setups, tr = g_traces, bl = g_blurs, hc = g_hide_calls;
	const unsigned set = c->ticket_set % (2u * (unsigned)c->launch_rot);
	const size_t log0 = g_log.size();
	int rc = PWN_EINVAL;
	if(kind == PLAIN_COL) rc = pwn_trace_viewports_device(c, l, cams.data(), secs.data(), 0, pl.a.p(), pl.b.p(), pl.d.p(), s);
	if(kind == HIDE_COL) rc = pwn_trace_viewports_hide_device(c, l, cams.data(), secs.data(), hide, 0, pl.a.p(), pl.b.p(), pl.d.p(), s);
	if(kind == PLAIN_HITS) rc = pwn_trace_viewport_hits_device(c, l, cams.data(), 0, pl.a.p(), pl.b.p(), pl.d.p(), s);
	if(kind == HIDE_HITS) rc = pwn_trace_viewport_hits_hide_device(c, l, cams.data(), hide, 0, pl.a.p(), pl.b.p(), pl.d.p(), s);
	REQ(rc == PWN_OK);
	const bool hid = kind == HIDE_COL || kind == HIDE_HITS, col = kind == PLAIN_COL || kind == HIDE_COL;
	// the launches: one set-up, one trace, the blur passes of a colour call; a wait between streams only in front of the set-up
	REQ(g_setups == su + 1 && g_traces == tr + 1 && g_blurs == bl + (col ? blur : 0));
	{
		std::vector<std::string> got;
		for(size_t k = log0; k < g_log.size(); k++) if(g_log[k] != "wait") got.push_back(g_log[k]);
		REQ(got.size() >= 2 && got[0] == "setup" && got[1] == "trace");
		for(size_t k = 2; k < got.size(); k++) REQ(got[k] == "blur");
	}
	// d_hide reaches the set-up launcher -- and a plain call passes none
	REQ(g_hide_calls == hc + (hid ? 1 : 0));
	REQ(g_hide_seen == (hid ? hide : NULL) && g_hide_n == (hid ? NV : 0));
	check_words(hid ? hide : NULL);
	// the trace launch: the call's mode, with the HIDE bit for a hide call and without it otherwise; the set's records and tickets
	REQ(g_mode == ((col ? PWN_KM_VIEWPORTS : PWN_KM_VIEWPORT_HITS) | (hid ? PWN_KM_HIDE : 0)));
	REQ(g_P.view_hide == (hid ? 1 : 0) && g_P.ray_hide == NULL && g_P.vps != NULL && g_P.views == NULL && g_P.rays == NULL);
	REQ((g_P.hits != NULL) == !col);
	REQ(g_P.vps == c->d_prec_dev + (size_t)set * PWN_VIEWS_MAX);
	REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
	REQ(g_P.w == W && g_P.h == H && g_P.nvp == NV);
}

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_launch_hook = on_small; pwn_fake_trace_hook = on_trace; pwn_fake_blur_hook = on_blur; pwn_fake_viewport_hide_hook = on_hide;
	fakehip_call_hook = on_call;
	pwn_ctx *c = NULL, *bare = NULL, *other = NULL;
	REQ(pwn_init(&c, 0, 64, 48) == PWN_OK && pwn_level_load(c, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 64, 48) == PWN_OK);
	REQ(pwn_init(&other, 0, 64, 48) == PWN_OK && pwn_level_load(other, argv[1]) == PWN_OK);
	pwn_vp_layout *A = NULL, *odd = NULL, *bl = NULL;
	REQ(pwn_viewports_layout(c, W, H, NV, HV, &A) == PWN_OK);
	REQ(pwn_viewports_layout(bare, W, H, NV, HV, &bl) == PWN_OK);
	{
		unsigned long long info[6];
		REQ(pwn_viewports_layout_info(A, info) == PWN_OK && info[5] == 1ull && info[3] == 21ull + 16ull + 18ull + 1ull);
		const pwn_viewport o = { 1, 0, 37, 21 };          // (no layout a blur could take)
		REQ(pwn_viewports_layout(c, W, H, 1, &o, &odd) == PWN_OK);
		REQ(pwn_viewports_layout_info(odd, info) == PWN_OK && info[5] == 0ull);
	}
	hipStream_t s2 = NULL;
	REQ(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess);
	dev hd(8);
	int32_t *hide = (int32_t *)hd.q;
	const int32_t h0[NV] = { 0, 1, 5, PWN_HIDE_NONE }, h1[NV] = { 13, PWN_HIDE_NONE, 0, 0 }, hx[NV] = { -7, PWN_OBJ_MAX, INT_MAX, PWN_OBJ_MAX - 1 };
	planes pl;

	// ---- the first device call allocates the records; after it nothing allocates, synchronises or waits on the host
	memcpy(hide, h0, sizeof(h0));
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 1) == PWN_OK);
	one_call(c, A, HIDE_COL, hide, 1, c->stream, pl, 1);
	const int a0 = g_allocs, s0 = g_syncs, e0 = g_event_syncs;
	memcpy(hide, hx, sizeof(hx));
	one_call(c, A, HIDE_COL, hide, 2, c->stream, pl, 1);          // (values that are no index: word 0; the largest index: its word)
	one_call(c, A, HIDE_HITS, hide, 3, c->stream, pl, 1);
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);

	// ---- mixed plain and hide calls, colour and hits, on one stream: the sets in turn; every set holds a hide call's records and then
	// a plain call's, whose words are 0 (check_words in one_call)
	memcpy(hide, h1, sizeof(h1));
	{
		unsigned hid_sets = 0, plain_after = 0;
		for(int k = 0; k < 16; k++)
		{
			const int w0 = g_waits;
			const unsigned set = c->ticket_set % (2u * (unsigned)c->launch_rot);
			// (five of a kind in turn over four sets: every set meets every kind)
			const int kind = (k / 5) % 2 == 0 ? ((k & 1) ? HIDE_HITS : HIDE_COL) : ((k & 1) ? PLAIN_HITS : PLAIN_COL);
			one_call(c, A, kind, hide, 10 + k, c->stream, pl, 0);
			REQ(g_waits == w0);
			if(kind == HIDE_COL || kind == HIDE_HITS) hid_sets |= 1u << set;
			else if(hid_sets & (1u << set)) plain_after |= 1u << set;
		}
		REQ(hid_sets == 0xfu && plain_after == 0xfu);
	}
	// ---- two streams alternating, hide and plain alternating against the streams
	{
		for(int k = 0; k < 2; k++) one_call(c, A, PLAIN_COL, hide, 30 + k, c->stream, pl, 0);
		unsigned sets_seen = 0;
		for(int k = 0; k < 12; k++)
		{
			const int w0 = g_waits;
			sets_seen |= 1u << (c->ticket_set % 4u);
			static const int kinds[3] = { HIDE_COL, PLAIN_HITS, HIDE_HITS };
			one_call(c, A, k % 4 == 3 ? PLAIN_COL : kinds[k % 3], hide, 40 + k, (k & 1) ? s2 : c->stream, pl, 0);
			// (alternating: launch n - 2 is on this call's stream -- but for the first on s2, put behind launch n - 2 twice)
			REQ(g_waits - w0 == (k == 1 ? 2 : 0));
		}
		REQ(sets_seen == 0xfu);
	}
	REQ(g_allocs == a0 && g_syncs == s0 && g_event_syncs == e0);

	// ---- refusals: nothing launched, nothing written, nothing changed
	{
		const size_t plane = (size_t)W * H;
		std::vector<float> cams, secs;
		make_cams(cams, secs, NV, 9);
		dev blk(3 * plane + 8);
		uint32_t *p0 = blk.q, *p1 = blk.q + plane, *p2 = blk.q + 2 * plane;
		const int su = g_setups, tr = g_traces, bu = g_blurs, so = g_small_other, wa = g_waits, hc = g_hide_calls;
		const unsigned set0 = c->ticket_set;
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 1) == PWN_OK);
#define COL(ctx, L, Hd, Wk, Sb, Zb) pwn_trace_viewports_hide_device(ctx, L, cams.data(), secs.data(), Hd, 0, Wk, Sb, Zb, NULL)
#define HIT(ctx, L, Hd, Lb, Cl, Ds) pwn_trace_viewport_hits_hide_device(ctx, L, cams.data(), Hd, 0, Lb, Cl, Ds, NULL)
		REQ(COL(c, A, NULL, p0, p1, p2) == PWN_EINVAL);                                      // NULL
		REQ(COL(c, A, (char *)hide + 2, p0, p1, p2) == PWN_EINVAL);                          // misaligned
		REQ(COL(c, A, p0, p0, p1, p2) == PWN_EINVAL);                                        // inside d_work, d_sbuf, d_zbuf
		REQ(COL(c, A, p1 + plane - 1, p0, p1, p2) == PWN_EINVAL);
		REQ(COL(c, A, p2 + 17, p0, p1, p2) == PWN_EINVAL);
		REQ(COL(c, A, p2 + plane - 3, p0, p1, p2) == PWN_EINVAL);                            // (its first three entries are d_zbuf's last words)
		REQ(COL(NULL, A, hide, p0, p1, p2) == PWN_EINVAL);
		REQ(COL(c, NULL, hide, p0, p1, p2) == PWN_EINVAL);
		REQ(COL(c, bl, hide, p0, p1, p2) == PWN_EINVAL);                                     // another context's layout
		REQ(COL(other, A, hide, p0, p1, p2) == PWN_EINVAL);
		REQ(COL(c, odd, hide, p0, p1, p2) == PWN_EINVAL);                                    // blur on a layout not usable with blur
		REQ(pwn_trace_viewports_device(c, odd, cams.data(), secs.data(), 0, p0, p1, p2, NULL) == PWN_EINVAL);     // (as its sibling)
		REQ(COL(bare, bl, hide, p0, p1, p2) == PWN_ENOLEVEL);
		REQ(HIT(c, A, NULL, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(c, A, (char *)hide + 1, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(c, A, p0 + 5, p0, p1, p2) == PWN_EINVAL);                                    // inside d_label, d_cell, d_dist
		REQ(HIT(c, A, p1, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(c, A, p2 + plane - 1, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(c, A, p2 + plane - 1, p0, NULL, p2) == PWN_EINVAL);
		REQ(HIT(NULL, A, hide, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(c, bl, hide, p0, p1, p2) == PWN_EINVAL);
		REQ(HIT(bare, bl, hide, p0, p1, p2) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(COL(c, A, hide, p0, p1, p2) == PWN_EBUSY && HIT(c, A, hide, p0, p1, p2) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(g_setups == su && g_traces == tr && g_blurs == bu && g_small_other == so && g_waits == wa && g_hide_calls == hc && c->ticket_set == set0 && blk.poisoned());
		// an array next to the planes, and inside a plane the call was not given: accepted
		REQ(HIT(c, A, p1 + 8, p0, NULL, p2) == PWN_OK);
		REQ(COL(c, A, blk.q + 3 * plane, p0, p1, p2) == PWN_OK);
		REQ(g_setups == su + 2 && g_traces == tr + 2 && g_hide_calls == hc + 2);
		REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
#undef COL
#undef HIT
	}

	// ---- a hide call records the layout-use event that free waits for, per stream
	{
		std::vector<float> cams, secs;
		make_cams(cams, secs, NV, 2);
		pwn_vp_layout *F = NULL;
		REQ(pwn_viewports_layout(c, W, H, NV, HV, &F) == PWN_OK);
		g_rec_ev = NULL;
		REQ(pwn_trace_viewport_hits_hide_device(c, F, cams.data(), hide, 0, pl.a.p(), NULL, NULL, c->stream) == PWN_OK);
		const void *used = g_rec_ev;
		REQ(used != NULL && g_rec_stream == (const void *)c->stream && g_log.back() == "trace");
		for(int k = 0; k < 3; k++) REQ(used != (const void *)c->launch_event[k]);
		const size_t log0 = g_log.size();
		const int e1 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK);
		REQ(g_event_syncs == e1 + 1 && g_synced.back() == used);
		REQ(g_log.size() >= log0 + 2 && g_log[log0] == "eventsync" && g_log[log0 + 1] == "free");
		REQ(pwn_viewports_layout(c, W, H, NV, HV, &F) == PWN_OK);
		g_rec_ev = NULL;
		REQ(pwn_trace_viewports_hide_device(c, F, cams.data(), secs.data(), hide, 0, NULL, pl.b.p(), pl.d.p(), c->stream) == PWN_OK);
		const void *used1 = g_rec_ev;
		REQ(used1 != NULL && g_rec_stream == (const void *)c->stream);
		REQ(pwn_trace_viewports_hide_device(c, F, cams.data(), secs.data(), hide, 0, NULL, pl.b.p(), pl.d.p(), s2) == PWN_OK);
		REQ(g_rec_ev != used1 && g_rec_stream == (const void *)s2);
		const int e2 = g_event_syncs;
		REQ(pwn_viewports_layout_free(c, F) == PWN_OK && g_event_syncs == e2 + 2);          // one per stream it was used on
		const int su = g_setups;
		pl.a.fill();
		REQ(pwn_trace_viewport_hits_hide_device(c, F, cams.data(), hide, 0, pl.a.p(), NULL, NULL, c->stream) == PWN_EINVAL);      // a freed layout
		REQ(g_setups == su && pl.a.poisoned());
	}

	// ---- the rays' call: the array travels in the launch's parameters, and the launch has the HIDE bit
	{
		const int n = 65;
		dev rays(8 * (size_t)n + 4), seeds(n), col((size_t)n + 4), depth(n), rh((size_t)n + 2);
		const int tr = g_traces, su = g_setups;
		unsigned set = c->ticket_set % (2u * (unsigned)c->launch_rot);
		REQ(pwn_trace_rays_hide_device(c, n, rays.p(), seeds.p(), rh.p(), 1.25f, 0, col.p(), depth.p(), c->stream) == PWN_OK);
		REQ(g_traces == tr + 1 && g_setups == su && g_mode == (PWN_KM_RAYS | PWN_KM_HIDE));
		REQ(g_P.ray_hide == (const int32_t *)rh.q && g_P.view_hide == 0 && g_P.hits == NULL && g_P.rays == (const float *)rays.q && g_P.nrays == (uint32_t)n);
		REQ(g_P.ray_seeds == seeds.q && g_P.sbuf == col.q && g_P.zbuf == (float *)depth.q && g_P.sec_current == 1.25f && g_P.ray_w == 0);
		REQ(g_P.tickets == c->d_tickets + set * PWN_QUEUES * PWN_QUEUE_STRIDE);
		REQ(pwn_trace_rays_hide_device(c, n, rays.p(), NULL, rh.q + 1, 0.0f, PWN_RAYS_HAS_W, col.p(), depth.p(), s2) == PWN_OK);
		REQ(g_P.ray_hide == (const int32_t *)rh.q + 1 && g_P.ray_w == 1 && g_P.ray_seeds == NULL && g_traces == tr + 2 && g_mode == (PWN_KM_RAYS | PWN_KM_HIDE));
		// a plain call passes none, and its mode has no HIDE bit; the first hits' hide call has its own mode
		REQ(pwn_trace_rays_device(c, n, rays.p(), seeds.p(), 1.25f, 0, col.p(), depth.p(), c->stream) == PWN_OK);
		REQ(g_P.ray_hide == NULL && g_traces == tr + 3 && g_mode == PWN_KM_RAYS);
		{
			dev hits(12 * (size_t)n);
			REQ(pwn_trace_hits_hide_device(c, n, rays.p(), rh.p(), 0, hits.p(), c->stream) == PWN_OK);
			REQ(g_P.ray_hide == (const int32_t *)rh.q && g_P.hits == hits.q && g_traces == tr + 4 && g_mode == (PWN_KM_HITS | PWN_KM_HIDE));
		}
		// the empty batch: nothing launched, d_hide may be NULL
		const int tr1 = g_traces;
		REQ(pwn_trace_rays_hide_device(c, 0, NULL, NULL, NULL, 0.0f, 0, NULL, NULL, c->stream) == PWN_OK && g_traces == tr1);
		// refusals
		const unsigned set0 = c->ticket_set;
		col.fill(); depth.fill();
#define RAY(ctx, N, Hd, Col, Dep) pwn_trace_rays_hide_device(ctx, N, rays.p(), seeds.p(), Hd, 0.0f, 0, Col, Dep, NULL)
		REQ(RAY(c, n, NULL, col.p(), depth.p()) == PWN_EINVAL);
		REQ(RAY(c, n, (char *)rh.q + 2, col.p(), depth.p()) == PWN_EINVAL);
		REQ(RAY(c, n, col.q, col.p(), depth.p()) == PWN_EINVAL);                             // inside d_col
		REQ(RAY(c, n, col.q + n - 1, col.p(), depth.p()) == PWN_EINVAL);
		REQ(RAY(c, 1, depth.q, col.p(), depth.p()) == PWN_EINVAL);                           // d_depth itself
		REQ(RAY(c, 2, depth.q - 1 + 2, col.p(), depth.q + 2) == PWN_EINVAL);                 // (its last entry is d_depth's first word)
		REQ(RAY(NULL, n, rh.p(), col.p(), depth.p()) == PWN_EINVAL);
		REQ(RAY(c, -1, rh.p(), col.p(), depth.p()) == PWN_EINVAL);
		REQ(RAY(c, n, rh.p(), NULL, depth.p()) == PWN_EINVAL);
		REQ(pwn_trace_rays_hide_device(c, n, rays.p(), seeds.p(), rh.p(), 0.0f, 2, col.p(), depth.p(), NULL) == PWN_EINVAL);
		REQ(RAY(bare, n, rh.p(), col.p(), depth.p()) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;
		REQ(RAY(c, n, rh.p(), col.p(), depth.p()) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(g_traces == tr1 && c->ticket_set == set0 && col.poisoned() && depth.poisoned());
		// n entries behind the colours' n words: accepted
		REQ(RAY(c, 4, col.q + 4, col.p(), depth.p()) == PWN_OK && g_traces == tr1 + 1);
#undef RAY
	}

	// ---- a group's handle
	{
		const int devs[2] = { 0, 0 };
		pwn_ctx *g = NULL;
		REQ(pwn_init_multi(&g, devs, 2, W, H) == PWN_OK);
		std::vector<float> cams, secs;
		make_cams(cams, secs, NV, 1);
		const int su = g_setups, tr = g_traces;
		pl.a.fill(); pl.b.fill(); pl.d.fill();
		REQ(pwn_trace_viewports_hide_device(g, A, cams.data(), secs.data(), hide, 0, pl.a.p(), pl.b.p(), pl.d.p(), NULL) == PWN_ENOTSUP);
		REQ(pwn_trace_viewport_hits_hide_device(g, A, cams.data(), hide, 0, pl.a.p(), NULL, NULL, NULL) == PWN_ENOTSUP);
		REQ(pwn_trace_rays_hide_device(g, 1, pl.a.p(), NULL, hide, 0.0f, 0, pl.b.p(), pl.d.p(), NULL) == PWN_ENOTSUP);
		REQ(g_setups == su && g_traces == tr && pl.a.poisoned() && pl.b.poisoned() && pl.d.poisoned());
		pwn_destroy(g);
	}

	REQ(g_small_other == 0);
	REQ(hipStreamDestroy(s2) == hipSuccess);
	// A, odd and bl are still alive: pwn_destroy frees what is left (the leak check at exit says so)
	pwn_destroy(other); pwn_destroy(bare); pwn_destroy(c);
	printf("ok\n");
	return 0;
}
