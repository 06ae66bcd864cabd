// What every entry point of the host API sends to the device, written down: the blocking call (one piece and in strips), the view
// batches (host and device form, viewports), the ray and hit batches and the frames in flight, with 0 to 3 blur passes, their
// refusals and their out-of-memory paths -- on the CPU, under AddressSanitizer + UBSan, against the fake HIP runtime (README.txt).
// For every API call the transcript on stdout has the return code, pwn_last_error where it is not PWN_OK, in order every runtime
// call of the choreography (copies, memsets, events, waits, allocations) and every launch with its parameters, and an FNV hash of
// every buffer the call filled.  Pointers are printed as the context's or the caller's buffer they point into plus an offset, event
// times not at all: two runs print the same bytes, and tests/golden/host_calls.txt is what the tree printed before the batch calls'
// common code was folded (tests/test_sanitize_host.py compares).  To keep the file small a launch's fields that are 0 / NULL are
// not printed, an offset of 0 neither, runtime calls in a row share a line, and a call that sent nothing is one line.
//   calls_asan <level file>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "pwn_internal.h"

extern "C" {
extern void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern void (*pwn_fake_blur_hook)(const pwn_blur_params *B);
extern void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);
extern void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern long fakehip_alloc_fail_in;
extern int fakehip_query_busy;
}

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
	const unsigned char *b = (const unsigned char *)p;
	for(size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
	return h;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ---- names for pointers ----
struct named { std::string name; const void *base; size_t bytes; };
static pwn_ctx *g_c;
static std::vector<named> g_caller, g_new;       // the caller's buffers; what the current call has allocated so far
static void reg(const char *name, const void *p, size_t bytes) { g_caller.push_back({ name, p, bytes }); }
static std::string idx(const char *n, int i, int k = -1) { char b[64]; if(k < 0) snprintf(b, sizeof(b), "%s[%d]", n, i); else snprintf(b, sizeof(b), "slot[%d].%s", i, n); return b; }
static std::string nm(const void *p)
{
	if(p == NULL) return "NULL";
	std::vector<named> t;
	pwn_ctx *c = g_c;
	if(c != NULL)
	{
		const size_t pl = (size_t)c->w * c->h * 4;
#define N(f, bytes) t.push_back({ #f, c->f, (size_t)(bytes) })
		N(d_pre, pl); N(d_out, pl); N(d_z, pl); N(d_pre2, pl); N(d_skip, c->w * 2); N(d_counters, PWN_NCOUNTERS * 8);
		N(d_vpre, pl * c->views_cap); N(d_vout, pl * c->views_cap); N(d_vz, pl * c->views_cap);
		N(h_vrec, PWN_VIEWS_MAX * sizeof(pwn_view_rec)); N(d_vrec, PWN_VIEWS_MAX * sizeof(pwn_view_rec));
		N(d_vrec_dev, (size_t)PWN_TICKET_SETS * PWN_VIEWS_MAX * sizeof(pwn_view_rec));
		N(d_ppre, pl); N(d_pout, pl); N(d_pz, pl);
		N(h_prec, PWN_VIEWS_MAX * sizeof(pwn_viewport_rec)); N(d_prec, PWN_VIEWS_MAX * sizeof(pwn_viewport_rec));
		N(h_rays, c->rays_cap * 44 + 16); N(d_rays, c->rays_cap * 44 + 16);
		N(h_hits, c->hits_cap * 80 + 16); N(d_hits, c->hits_cap * 80 + 16);
		N(d_tickets, (size_t)PWN_TICKET_SETS * PWN_QUEUES * PWN_QUEUE_STRIDE * 4);
		N(d_strip_miss, 64); N(h_strip_miss, 64);
		N(stream, 1); N(stream2, 1); N(copy_stream, 1); N(copy_stream2, 1); N(up_stream, 1);
		N(d_wave_log, c->wave_log_cap * 16);
#undef N
		for(int i = 0; i < PWN_NBLOB; i++)
		{
			t.push_back({ idx("d_blob", i), c->d_blob[i], PWN_BLOB_MAX }); t.push_back({ idx("d_big", i), c->d_big[i], c->d_big_cap[i] });
			t.push_back({ idx("ev_tables", i), c->ev_tables[i], 1 }); t.push_back({ idx("ev_upload", i), c->ev_upload[i], 1 });
		}
		for(int i = 0; i < PWN_NSTAGE; i++)
		{
			t.push_back({ idx("h_stage", i), c->h_stage[i], PWN_BLOB_MAX }); t.push_back({ idx("h_big", i), c->h_big[i], c->h_big_cap[i] });
			t.push_back({ idx("ev_stage", i), c->ev_stage[i], 1 });
		}
		for(int i = 0; i < 4; i++) t.push_back({ idx("ev", i), c->ev[i], 1 });
		for(int i = 0; i < c->strip_ev_n; i++) t.push_back({ idx("strip_ev", i), c->strip_ev[i], 1 });
		for(int i = 0; i < 4; i++) { t.push_back({ idx("order_cost", i), c->order[i].d_cost, c->order[i].cost_cap * 2 }); t.push_back({ idx("order_perm", i), c->order[i].d_perm, c->order[i].perm_cap * 4 }); }
		const size_t surf = (size_t)c->frame_pitch * c->h * c->frame_scale;
		for(int i = 0; i < PWN_MAX_SLOTS; i++)
		{
			const pwn_slot &s = c->slot[i];
			t.push_back({ idx("d_out", i, 0), s.d_out, pl }); t.push_back({ idx("d_z", i, 0), s.d_z, pl }); t.push_back({ idx("d_surface", i, 0), s.d_surface, surf });
			t.push_back({ idx("h_sbuf", i, 0), s.h_sbuf, pl }); t.push_back({ idx("h_zbuf", i, 0), s.h_zbuf, pl }); t.push_back({ idx("h_surface", i, 0), s.h_surface, surf });
			for(int k = 0; k < 4; k++) { char b[32]; snprintf(b, sizeof(b), "ev_k[%d]", k); t.push_back({ idx(b, i, 0), s.ev_k[k], 1 }); }
			t.push_back({ idx("ev_done", i, 0), s.ev_done, 1 });
		}
	}
	t.insert(t.end(), g_caller.begin(), g_caller.end());
	t.insert(t.end(), g_new.begin(), g_new.end());
	for(const named &e : t)
		if(e.base != NULL && e.bytes > 0 && (const char *)p >= (const char *)e.base && (const char *)p < (const char *)e.base + e.bytes)
		{
			char b[32];
			if(p == e.base) return e.name;
			snprintf(b, sizeof(b), "+%zu", (size_t)((const char *)p - (const char *)e.base));
			return e.name + b;
		}
	return "?";
}
#define S(p) nm(p).c_str()

// ---- the hooks ----
#include <stdarg.h>
static bool g_in_row;                            // the last thing sent was a runtime call, not a launch
static std::string g_body;                       // what the current call has sent so far
static void emit(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void emit(const char *fmt, ...)
{
	char b[2048];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(b, sizeof(b), fmt, ap);
	va_end(ap);
	g_body += b;
}
// (fields of a launch that are 0 / NULL are left out)
static void fu(const char *n, unsigned long long v) { if(v) emit(" %s %llu", n, v); }
static void fp(const char *n, const void *p);
static void on_call(const char *name, const void *a, const void *b, size_t bytes)
{
	const bool alloc = strcmp(name, "hipMalloc") == 0 || strcmp(name, "hipHostMalloc") == 0;
	// (runtime calls in a row share a line: launches and the result begin a new one)
	const char *sep = "  ";
	if(g_body.size() > 1 && g_body.back() == '\n' && g_in_row) { g_body.pop_back(); sep = "; "; }
	g_in_row = true;
	if(alloc)
	{
		char nb[32];
		snprintf(nb, sizeof(nb), "new%zu", g_new.size());
		if(a != NULL) g_new.push_back({ nb, a, bytes ? bytes : 1 });
		emit("%s%s %zu -> %s\n", sep, name + 3, bytes, a != NULL ? nb : "fails");
		return;
	}
	emit("%s%s %s", sep, name + 3, S(a));
	if(b != NULL) emit(" %s", S(b));
	if(bytes) emit(" %zu", bytes);
	emit("\n");
}
static void fp(const char *n, const void *p) { if(p != NULL) emit(" %s %s", n, S(p)); }
static void f4(const char *n, const float *v) { if(bits(v[0]) | bits(v[1]) | bits(v[2]) | bits(v[3])) emit(" %s %08x %08x %08x %08x", n, bits(v[0]), bits(v[1]), bits(v[2]), bits(v[3])); }
static void on_trace(const pwn_trace_params *P, int grid, size_t lds_bytes)
{
	g_in_row = false;
	emit("  TRACE grid %d lds %zu", grid, lds_bytes);
	f4("rayb", P->rayb); f4("rdx", P->rdx); f4("rdy", P->rdy); f4("from", P->from);
	if(bits(P->sec_current)) emit(" sec %08x", bits(P->sec_current));
	emit(" w %d h %d y %d %d tiles %d %d ux %u %d blob %u %u %u", P->w, P->h, P->y0, P->y1, P->tiles_x, P->tiles_total, P->ux_magic, P->ux_shift, P->blob_bytes, P->off_sph, P->off_recsph);
	if(P->tile_pairs) emit(" pairs %d single %d tx %u %d", P->tile_pairs, P->pair_single_rows, P->tx_magic, P->tx_shift);
	fp("sbuf", P->sbuf); fp("zbuf", P->zbuf); fp("blob", P->blob); fp("counters", P->counters); fp("wave_log", P->wave_log);
	fu("has_w", (unsigned)P->has_w); fu("scheduler", (unsigned)P->scheduler); fu("refill_limit", (unsigned)P->refill_limit);
	fp("tickets", P->tickets); fp("next", P->tickets_next); fp("cost_word", P->cost_word); fp("unit_cost", P->unit_cost); fp("perm", P->perm); fu("perm_cap", P->perm_cap);
	fp("clear_word", P->clear_word);
	if(P->views != NULL) emit(" views %s %d %u %d plane %llu records %016llx", S(P->views), P->nviews, P->views_magic, P->views_shift, P->plane, (unsigned long long)fnv(P->views, sizeof(pwn_view_rec) * (size_t)P->nviews));
	if(P->vps != NULL) emit(" vps %s %d step0 %u records %016llx", S(P->vps), P->nvp, P->vp_step0, (unsigned long long)fnv(P->vps, sizeof(pwn_viewport_rec) * (size_t)P->nvp));
	fp("g_rec", P->g_rec); fp("g_which", P->g_which); fp("g_sph", P->g_sph);
	if(P->nbounds) emit(" nbounds %d bounds %016llx", P->nbounds, (unsigned long long)fnv(P->bounds, sizeof(pwn_sphere_bound) * (size_t)P->nbounds));
	for(int i = 0; i < PWN_BOUNDS_MAX; i++) if(P->bound_ids[i] != 0xffffffffu) emit(" id%d %08x", i, P->bound_ids[i]);
	if(P->rays != NULL)
		emit(" rays %s seeds %s n %u ray_w %d hits %s records %016llx seeds %016llx", S(P->rays), S(P->ray_seeds), P->nrays, P->ray_w, S(P->hits),
			(unsigned long long)fnv(P->rays, 32 * (size_t)P->nrays), (unsigned long long)(P->ray_seeds ? fnv(P->ray_seeds, 4 * (size_t)P->nrays) : 0ull));
	emit("\n");
	// (the stand-in kernel traces frames; for a batch of rays this writes what the copy down brings back)
	if(P->rays != NULL)
	{
		for(uint32_t i = 0; i < P->nrays; i++)
		{
			const uint32_t k = (uint32_t)fnv(P->rays + 8 * (size_t)i, 32) ^ (P->ray_seeds ? P->ray_seeds[i] : 0u) ^ bits(P->sec_current);
			if(P->hits != NULL)
			{
				pwn_hit hit;
				memset(&hit, 0, sizeof(hit));
				hit.kind = (int32_t)(k % 3u); hit.object = (int32_t)i; hit.dist = (float)(k & 1023u);
				memcpy((unsigned char *)P->hits + sizeof(pwn_hit) * (size_t)i, &hit, sizeof(hit));
			}
			else { P->sbuf[i] = k; P->zbuf[i] = P->zbuf[i] + 1.0f + (float)(k & 7u); }
		}
	}
}
static void on_blur(const pwn_blur_params *B)
{
	g_in_row = false;
	emit("  BLUR w %d h %d y %d %d groups %d pre %s zbuf %s out %s skip %s tile %d %d batch %d cost %u %u", B->w, B->h, B->y0, B->y1, B->groups, S(B->pre), S(B->zbuf), S(B->out), S(B->skip),
		B->tile_h, B->tile_w, B->batch, B->cost_mul, B->cost_div);
	if(B->avail_y0 | B->avail_y1) emit(" avail %d %d", B->avail_y0, B->avail_y1);
	fp("miss", B->miss); fp("cost_acc", B->cost_acc); fp("cost_out", B->cost_out);
	if(B->views) emit(" views %d", B->views);
	emit(" plane %llu", B->plane);
	if(B->vps != NULL) emit(" vps %s %d %d", S(B->vps), B->nvp, B->vp_tiles);
	emit("\n");
}
static void on_launch(const char *name, const void *src, const void *dst, int ns, const size_t *sizes)
{
	g_in_row = false;
	emit("  LAUNCH %s %s -> %s", name, S(src), S(dst));
	for(int i = 0; i < ns; i++) emit(" %zu", sizes[i]);
	if(strcmp(name, "upload") == 0) emit(" bytes %016llx", (unsigned long long)fnv(src, sizes[0]));
	emit("\n");
}

// ---- one API call of the transcript ----
#define SENTINEL (-7777.0f)
static std::string g_what;
static bool g_open;               // the result line is still open: the outputs' hashes go on it
static void close_line() { if(g_open) printf("\n"); g_open = false; }
static void begin(const char *what)
{
	g_what = what; g_body.clear(); g_in_row = false;
	g_new.clear();
	if(g_c != NULL) g_c->stats.trace_ms = g_c->stats.blur_ms = g_c->stats.total_ms = SENTINEL;
}
static int end(int rc)
{
	close_line();
	printf("== %s", g_what.c_str());
	if(!g_body.empty())
	{
		if(g_body.find('\n') == g_body.size() - 1 && g_body.size() < 120) printf(":%.*s", (int)g_body.size() - 2, g_body.c_str() + 1);      // (one short line: beside the name)
		else printf("\n%s ", g_body.c_str());
	}
	printf(" -> %d", rc);
	if(rc < 0 && g_c != NULL) printf(" (%s)", pwn_last_error(g_c));
	if(g_c != NULL)
	{
		const pwn_stats &s = g_c->stats;
		if(s.trace_ms != SENTINEL || s.blur_ms != SENTINEL || s.total_ms != SENTINEL)
			printf(" stats written:%s%s%s%s", s.trace_ms != SENTINEL ? " trace_ms" : "", s.blur_ms != SENTINEL ? " blur_ms" : "", s.total_ms != SENTINEL ? " total_ms" : "",
				s.blur_ms == 0.0f ? " (blur_ms == 0)" : "");
	}
	g_body.clear(); g_new.clear();
	g_open = true;
	return rc;
}
#define CALL(what, expr) (begin(what), end(expr))
static void out(const char *name, const void *p, size_t bytes) { printf(" | %s %016llx", name, (unsigned long long)fnv(p, bytes)); }
#define OUT2(a, na, b, nb) (out(#a, a, na), out(#b, b, nb))
#define REQ(x) do { if(!(x)) { fflush(stdout); fprintf(stderr, "CHECK FAILED %s line %d\n", #x, __LINE__); exit(1); } } while(0)
static void opt(pwn_ctx *c, int o, int v) { REQ(pwn_set_option(c, o, v) == PWN_OK); }

static unsigned rs = 2024; static float rnd() { rs = rs * 1664525u + 1013904223u; return (float)(rs >> 8) / 16777216.0f; }

// ---- the trace launcher's branches (pwn_i_launch_trace): contexts of their own, whose pwn_init reads the settings given (name,
// value, ...), with the level and these spheres; every launch is a pwn_trace_rows_device into planes of the caller's
static std::vector<uint32_t> big_s(32768 * 16);
static std::vector<float> big_z(32768 * 16);
static pwn_ctx *ctx_env(int w, int h, const char *level, const std::vector<pwn_sphere> &sph, std::initializer_list<const char *> kv = {})
{
	for(const char *const *p = kv.begin(); p != kv.end(); p += 2) setenv(p[0], p[1], 1);
	pwn_ctx *x = NULL;
	REQ(pwn_init(&x, 0, w, h) == PWN_OK);
	for(const char *const *p = kv.begin(); p != kv.end(); p += 2) unsetenv(p[0]);
	REQ(pwn_level_load(x, level) == PWN_OK);
	REQ(pwn_upload_spheres(x, sph.data(), (int)sph.size()) == PWN_OK);
	return x;
}
static void section(const char *title) { close_line(); printf("---- launcher: %s\n", title); }
static void rows(pwn_ctx *x, const float *cam, int y0, int y1, hipStream_t s = NULL)
{
	char b[96];
	g_c = x;
	snprintf(b, sizeof(b), "pwn_trace_rows_device %d x %d rows %d %d%s", x->w, x->h, y0, y1, s != NULL ? " on stream2" : "");
	REQ(CALL(b, pwn_trace_rows_device(x, cam, 0.5f, y0, y1, big_s.data(), big_z.data(), s != NULL ? s : x->stream)) == PWN_OK);
}
static void blur_rows(pwn_ctx *x)
{
	g_c = x;
	REQ(CALL("pwn_blur_rows_device", pwn_blur_rows_device(x, 0, x->h, big_s.data(), big_z.data(), big_z.data() + (size_t)x->w * x->h, x->stream)) == PWN_OK);
}

#define W 96
#define H 64
#define PLANE (W * H)
#define VMAX 3
#define RMAX 5000

int main(int argc, char **argv)
{
	clearenv();            // (no PWN_* setting of the caller's changes what is sent)
	if(argc < 2) { fprintf(stderr, "usage: %s level.txt\n", argv[0]); return 2; }
	setvbuf(stdout, NULL, _IOFBF, 1 << 16);
	pwn_ctx *c = NULL, *bare = NULL, *odd = NULL, *wide = NULL, *m = NULL;
	REQ(pwn_init(&c, 0, W, H) == PWN_OK);
	REQ(pwn_level_load(c, argv[1]) == PWN_OK);
	std::vector<pwn_sphere> sph;
	for(int i = 0; i < 12; i++) sph.push_back({ 0.1f + 0.3f * rnd(), rnd(), 2.0f + 20.0f * rnd(), rnd(), 2.0f + 20.0f * rnd(), rnd(), rnd(), rnd() });
	REQ(pwn_upload_spheres(c, sph.data(), 12) == PWN_OK);
	REQ(pwn_init(&bare, 0, W, H) == PWN_OK);                      // no level
	REQ(pwn_init(&odd, 0, W - 2, H) == PWN_OK);                   // w & 3
	REQ(pwn_level_load(odd, argv[1]) == PWN_OK);
	REQ(pwn_init(&wide, 0, 32768, 16) == PWN_OK);                 // 1024 views of it are more than 2^28 pixels
	REQ(pwn_level_load(wide, argv[1]) == PWN_OK);
	REQ(pwn_init(&m, 0, W, H) == PWN_OK);                         // the out-of-memory paths: every buffer still to be allocated
	REQ(pwn_level_load(m, argv[1]) == PWN_OK);

	// cameras: ordinary ones, and [3] with w components
	static float cams[4 * 16], secs[4] = { 0.25f, 1.5f, 101.0f, 7.0f };
	for(int v = 0; v < 4; v++)
	{
		const float m[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 3.5f + v, 0.5f, 2.5f + 0.25f * v, 1 };
		memcpy(cams + 16 * v, m, sizeof(m));
		cams[16 * v + 1] = 0.125f * v; cams[16 * v + 8] = -0.0625f * v;
	}
	cams[16 * 3 + 3] = 0.5f; cams[16 * 3 + 15] = 0.75f;
	// the caller's buffers ("device" memory of the device forms is host memory here); 16-byte aligned, as the device forms ask
	static uint32_t sbuf[VMAX * PLANE] __attribute__((aligned(16))), work[VMAX * PLANE] __attribute__((aligned(16))), col[RMAX] __attribute__((aligned(16)));
	static float zbuf[VMAX * PLANE] __attribute__((aligned(16))), depth[RMAX] __attribute__((aligned(16))), rays[8 * RMAX] __attribute__((aligned(16))), dsecs[4] __attribute__((aligned(16)));
	static uint32_t seeds[RMAX] __attribute__((aligned(16)));
	static pwn_hit hits[RMAX] __attribute__((aligned(16)));
	static float dcams[4 * 16] __attribute__((aligned(16)));
	memcpy(dcams, cams, sizeof(cams)); memcpy(dsecs, secs, sizeof(secs));
	reg("sbuf", sbuf, sizeof(sbuf)); reg("zbuf", zbuf, sizeof(zbuf)); reg("work", work, sizeof(work)); reg("col", col, sizeof(col)); reg("depth", depth, sizeof(depth));
	reg("rays", rays, sizeof(rays)); reg("seeds", seeds, sizeof(seeds)); reg("hits", hits, sizeof(hits)); reg("cams", cams, sizeof(cams)); reg("secs", secs, sizeof(secs));
	reg("dcams", dcams, sizeof(dcams)); reg("dsecs", dsecs, sizeof(dsecs));
	for(int i = 0; i < RMAX; i++)
	{
		const float r[8] = { 3.5f + rnd(), 0.5f, 2.5f + rnd(), 1.0f, rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f, 0.0f };
		memcpy(rays + 8 * i, r, sizeof(r));
		seeds[i] = 77u * (uint32_t)i + 1u;
	}
	char what[160];
	g_c = c;
	pwn_fake_trace_hook = on_trace; pwn_fake_blur_hook = on_blur; pwn_fake_launch_hook = on_launch; fakehip_call_hook = on_call;

	// ---- the blocking call
	for(int passes = 0; passes <= 3; passes++)
	{
		opt(c, PWN_OPT_BLUR_PASSES, passes);
		snprintf(what, sizeof(what), "pwn_trace_screen_centred passes %d zbuf", passes);
		REQ(CALL(what, pwn_trace_screen_centred(c, cams, secs[0], sbuf, zbuf)) == PWN_OK);
		OUT2(sbuf, PLANE * 4, zbuf, PLANE * 4);
		snprintf(what, sizeof(what), "pwn_trace_screen_centred passes %d no zbuf", passes);
		REQ(CALL(what, pwn_trace_screen_centred(c, cams + 16, secs[1], sbuf, NULL)) == PWN_OK);
		out("sbuf", sbuf, PLANE * 4);
	}
	opt(c, PWN_OPT_CALL_STRIPS, 2);
	for(int passes = 0; passes <= 2; passes++)           // (two passes: not in strips)
	{
		opt(c, PWN_OPT_BLUR_PASSES, passes);
		snprintf(what, sizeof(what), "pwn_trace_screen_centred strips 2 passes %d", passes);
		REQ(CALL(what, pwn_trace_screen_centred(c, cams, secs[2], sbuf, passes == 1 ? NULL : zbuf)) == PWN_OK);
		printf(" | strips_last %d", c->strips_last);
		OUT2(sbuf, PLANE * 4, zbuf, PLANE * 4);
	}
	opt(c, PWN_OPT_CALL_STRIPS, -1);
	// with the units' order on, the sort goes between the last record and the wait
	opt(c, PWN_OPT_UNIT_ORDER, 1); opt(c, PWN_OPT_BLUR_PASSES, 1);
	for(int k = 0; k < 2; k++)
	{
		REQ(CALL("pwn_trace_screen_centred unit order passes 1", pwn_trace_screen_centred(c, cams, secs[0], sbuf, zbuf)) == PWN_OK);
		out("sbuf", sbuf, PLANE * 4);
	}
	opt(c, PWN_OPT_UNIT_ORDER, 0);

	// ---- batches of views
	const int vn[3] = { 1, 3, 2 };
	for(int passes = 0; passes <= 3; passes++)
	{
		opt(c, PWN_OPT_BLUR_PASSES, passes);
		for(int k = passes == 0 ? 0 : 2; k < 3; k++)          // (the planes grow once, under the first setting)
		{
			snprintf(what, sizeof(what), "pwn_trace_views n %d passes %d", vn[k], passes);
			REQ(CALL(what, pwn_trace_views(c, vn[k], cams, secs, sbuf, (k == 2 && passes == 0) ? NULL : zbuf)) == PWN_OK);
			OUT2(sbuf, (size_t)vn[k] * PLANE * 4, zbuf, (size_t)vn[k] * PLANE * 4);
		}
		snprintf(what, sizeof(what), "pwn_trace_views n 2 passes %d, a camera with w", passes);
		REQ(CALL(what, pwn_trace_views(c, 2, cams + 32, secs + 2, sbuf, zbuf)) == PWN_OK);
		OUT2(sbuf, 2 * PLANE * 4, zbuf, 2 * PLANE * 4);
	}
	for(int passes = 0; passes <= 3; passes++)
	{
		opt(c, PWN_OPT_BLUR_PASSES, passes);
		for(int flags = 0; flags <= PWN_VIEWS_HAS_W; flags++)
		{
			memset(zbuf, 0, sizeof(zbuf));
			snprintf(what, sizeof(what), "pwn_trace_views_device n 3 passes %d flags %d", passes, flags);
			REQ(CALL(what, pwn_trace_views_device(c, 3, dcams + 16, dsecs, flags, passes == 0 && flags == 0 ? NULL : work, sbuf, zbuf, c->stream)) == PWN_OK);
			OUT2(sbuf, 3 * PLANE * 4, zbuf, 3 * PLANE * 4);
		}
	}
	// (a call on another stream than the launches before it: the wait that puts it behind them)
	REQ(CALL("pwn_trace_views_device on stream2", pwn_trace_views_device(c, 2, dcams, dsecs, 0, work, sbuf, zbuf, c->stream2)) == PWN_OK);
	out("sbuf", sbuf, 2 * PLANE * 4);

	// ---- viewports
	const pwn_viewport some[3] = { { 0, 0, 48, 32 }, { 48, 0, 32, 64 }, { 4, 36, 20, 12 } }, all[1] = { { 0, 0, W, H } };
	for(int passes = 0; passes <= 3; passes++)
	{
		opt(c, PWN_OPT_BLUR_PASSES, passes);
		snprintf(what, sizeof(what), "pwn_trace_viewports 3 rectangles passes %d", passes);
		REQ(CALL(what, pwn_trace_viewports(c, 3, some, cams + 16, secs + 1, sbuf, zbuf)) == PWN_OK);
		OUT2(sbuf, PLANE * 4, zbuf, PLANE * 4);
		snprintf(what, sizeof(what), "pwn_trace_viewports the whole frame passes %d", passes);
		REQ(CALL(what, pwn_trace_viewports(c, 1, all, cams, secs, sbuf, NULL)) == PWN_OK);
		out("sbuf", sbuf, PLANE * 4);
	}

	// ---- rays and hits
	opt(c, PWN_OPT_BLUR_PASSES, 1);
	const int rn[4] = { 0, 1, 65, 5000 };
	for(int k = 0; k < 4; k++)
	{
		for(int i = 0; i < RMAX; i++) depth[i] = (float)(i % 13);
		snprintf(what, sizeof(what), "pwn_trace_rays n %d", rn[k]);
		REQ(CALL(what, pwn_trace_rays(c, rn[k], rays, seeds, secs[0], col, depth)) == PWN_OK);
		OUT2(col, 4 * (size_t)rn[k], depth, 4 * (size_t)rn[k]);
	}
	REQ(CALL("pwn_trace_rays n 65 seeds NULL", pwn_trace_rays(c, 65, rays, NULL, secs[1], col, depth)) == PWN_OK);
	OUT2(col, 4 * 65, depth, 4 * 65);
	REQ(CALL("pwn_trace_rays n 65 depth NULL", pwn_trace_rays(c, 65, rays, seeds, secs[1], col, NULL)) == PWN_OK);
	OUT2(col, 4 * 65, depth, 4 * 65);
	REQ(CALL("pwn_trace_rays n 65 col NULL", pwn_trace_rays(c, 65, rays, seeds, secs[1], NULL, depth)) == PWN_OK);
	OUT2(col, 4 * 65, depth, 4 * 65);
	rays[8 * 40 + 7] = 0.5f;
	REQ(CALL("pwn_trace_rays n 65, a ray with w", pwn_trace_rays(c, 65, rays, seeds, secs[1], col, depth)) == PWN_OK);
	OUT2(col, 4 * 65, depth, 4 * 65);
	for(int flags = 0; flags <= PWN_RAYS_HAS_W; flags++)
	{
		snprintf(what, sizeof(what), "pwn_trace_rays_device n 65 flags %d", flags);
		REQ(CALL(what, pwn_trace_rays_device(c, 65, rays, flags ? NULL : seeds, secs[2], flags, col, depth, c->stream)) == PWN_OK);
		OUT2(col, 4 * 65, depth, 4 * 65);
	}
	REQ(CALL("pwn_trace_rays_device n 0", pwn_trace_rays_device(c, 0, NULL, NULL, 0.0f, 0, NULL, NULL, c->stream)) == PWN_OK);
	for(int k = 0; k < 4; k++)
	{
		snprintf(what, sizeof(what), "pwn_trace_hits n %d", rn[k]);
		REQ(CALL(what, pwn_trace_hits(c, rn[k], rays, hits)) == PWN_OK);
		out("hits", hits, sizeof(pwn_hit) * (size_t)rn[k]);
	}
	rays[8 * 40 + 7] = 0.0f;
	REQ(CALL("pwn_trace_hits n 65, no ray with w", pwn_trace_hits(c, 65, rays, hits)) == PWN_OK);
	out("hits", hits, sizeof(pwn_hit) * 65);
	for(int flags = 0; flags <= PWN_RAYS_HAS_W; flags++)
	{
		snprintf(what, sizeof(what), "pwn_trace_hits_device n 65 flags %d", flags);
		REQ(CALL(what, pwn_trace_hits_device(c, 65, rays, flags, hits, c->stream)) == PWN_OK);
		out("hits", hits, sizeof(pwn_hit) * 65);
	}
	REQ(CALL("pwn_trace_hits_device n 0", pwn_trace_hits_device(c, 0, NULL, 0, NULL, c->stream)) == PWN_OK);

	// ---- frames in flight: three slots, six frames
	// (four frames: the fourth into the first slot again; the surface with one pass only, and a blocking call behind those)
	const int fflags[2] = { PWN_FRAME_SBUF | PWN_FRAME_ZBUF, PWN_FRAME_SURFACE };
	for(int ff = 0; ff < 2; ff++)
		for(int overlap = 0; overlap <= 1; overlap++)
			for(int passes = ff ? 1 : 0; passes <= (ff ? 1 : 3); passes++)
			{
				opt(c, PWN_OPT_BLUR_PASSES, passes); opt(c, PWN_OPT_FRAME_OVERLAP, overlap); opt(c, PWN_OPT_FRAME_TIMING, 2);
				close_line();
				printf("---- frames: 3 slots, flags %d, overlap %d, passes %d\n", fflags[ff], overlap, passes);
				fakehip_call_hook = NULL;            // (the slots' allocations are not what is looked at)
				REQ(pwn_frames_config(c, 3, fflags[ff], 2, 0) == PWN_OK);
				fakehip_call_hook = on_call;
				for(int f = 0; f < 4 + 3; f++)
				{
					const int slot = f % 3;
					if(f >= 3)
					{
						pwn_frame fr;
						snprintf(what, sizeof(what), "pwn_wait_frame slot %d", slot);
						REQ(CALL(what, pwn_wait_frame(c, slot, &fr)) == PWN_OK);
						printf(" | frame seq %llu sec %08x timed %d sbuf %s zbuf %s surface %s pitch %d d_sbuf %s d_zbuf %s d_surface %s", (unsigned long long)fr.seq, bits(fr.sec_current), fr.timed,
							S(fr.sbuf), S(fr.zbuf), S(fr.surface), fr.surface_pitch_bytes, S(fr.d_sbuf), S(fr.d_zbuf), S(fr.d_surface));
						if(fr.sbuf) printf(" out sbuf %016llx", (unsigned long long)fnv(fr.sbuf, PLANE * 4));
						if(fr.zbuf) printf(" zbuf %016llx", (unsigned long long)fnv(fr.zbuf, PLANE * 4));
						if(fr.surface) printf(" out surface %016llx", (unsigned long long)fnv(fr.surface, (size_t)fr.surface_pitch_bytes * H * 2));
					}
					if(f < 4)
					{
						snprintf(what, sizeof(what), "pwn_submit_frame %d slot %d", f, slot);
						REQ(CALL(what, pwn_submit_frame(c, cams + 16 * (f % 3), 0.5f * (float)f, slot)) == PWN_OK);
					}
				}
				if(ff == 0 && passes != 1) continue;
				// (a blocking call behind frames that were in flight on the two streams)
				REQ(CALL("pwn_trace_screen_centred behind the frames", pwn_trace_screen_centred(c, cams, secs[0], sbuf, zbuf)) == PWN_OK);
				out("sbuf", sbuf, PLANE * 4);
			}
	REQ(CALL("pwn_submit_frame into a slot in flight", (pwn_submit_frame(c, cams, 0.0f, 0), pwn_submit_frame(c, cams, 0.0f, 0))) == PWN_EBUSY);
	REQ(CALL("pwn_wait_frame slot 0", pwn_wait_frame(c, 0, NULL)) == PWN_OK);
	fakehip_call_hook = NULL;
	REQ(pwn_frames_config(c, 0, 0, 0, 0) == PWN_OK);
	fakehip_call_hook = on_call;

	// ---- refusals: which code a caller gets, also one with two faults
	opt(c, PWN_OPT_BLUR_PASSES, 1); opt(bare, PWN_OPT_BLUR_PASSES, 1); opt(odd, PWN_OPT_BLUR_PASSES, 1); opt(wide, PWN_OPT_BLUR_PASSES, 1);
	pwn_tiled *const busy = (pwn_tiled *)(uintptr_t)16;       // (never looked at by a call that is refused)
	const pwn_viewport badvp[2] = { { 0, 0, 48, 32 }, { 40, 0, 32, 32 } }, oddvp[1] = { { 0, 0, 46, 32 } };
#define REFUSE(ctx, expr) do { g_c = (ctx); CALL(#ctx ": " #expr, expr); g_c = c; } while(0)
	REFUSE(c, pwn_trace_screen_centred(NULL, cams, 0, sbuf, zbuf));
	REFUSE(c, pwn_trace_screen_centred(c, NULL, 0, sbuf, zbuf));
	REFUSE(c, pwn_trace_screen_centred(c, cams, 0, NULL, zbuf));
	REFUSE(odd, pwn_trace_screen_centred(odd, cams, 0, sbuf, zbuf));
	REFUSE(bare, pwn_trace_screen_centred(bare, cams, 0, sbuf, zbuf));
	REFUSE(c, pwn_submit_frame(c, cams, 0, 0));
	REFUSE(c, pwn_submit_frame(c, NULL, 0, 0));

	REFUSE(c, pwn_trace_views(NULL, 1, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_views(c, 1, NULL, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_views(c, 1, cams, NULL, sbuf, zbuf));
	REFUSE(c, pwn_trace_views(c, 1, cams, secs, NULL, zbuf));
	REFUSE(c, pwn_trace_views(c, 0, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_views(c, PWN_VIEWS_MAX + 1, cams, secs, sbuf, zbuf));
	REFUSE(wide, pwn_trace_views(wide, PWN_VIEWS_MAX, cams, secs, sbuf, zbuf));
	REFUSE(odd, pwn_trace_views(odd, 1, cams, secs, sbuf, zbuf));
	REFUSE(bare, pwn_trace_views(bare, 1, cams, secs, sbuf, zbuf));
	bare->tiled = busy; odd->tiled = busy; c->tiled = busy; wide->tiled = busy;
	REFUSE(c, pwn_trace_views(c, 1, cams, secs, sbuf, zbuf));
	REFUSE(bare, pwn_trace_views(bare, 1, cams, secs, sbuf, zbuf));
	REFUSE(odd, pwn_trace_views(odd, 1, cams, secs, sbuf, zbuf));
	REFUSE(wide, pwn_trace_views(wide, PWN_VIEWS_MAX, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(bare, pwn_trace_views_device(bare, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(odd, pwn_trace_views_device(odd, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(wide, pwn_trace_views_device(wide, PWN_VIEWS_MAX, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_viewports(c, 1, all, cams, secs, sbuf, zbuf));
	REFUSE(bare, pwn_trace_viewports(bare, 1, all, cams, secs, sbuf, zbuf));
	REFUSE(bare, pwn_trace_viewports(bare, 2, badvp, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_rays(c, 1, rays, seeds, 0, col, depth));
	REFUSE(bare, pwn_trace_rays(bare, 1, rays, seeds, 0, col, depth));
	REFUSE(bare, pwn_trace_rays(bare, 0, NULL, NULL, 0, col, depth));
	REFUSE(bare, pwn_trace_rays(bare, 1, NULL, seeds, 0, col, depth));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(bare, pwn_trace_rays_device(bare, 1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(bare, pwn_trace_rays_device(bare, 1, rays + 1, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_hits(c, 1, rays, hits));
	REFUSE(bare, pwn_trace_hits(bare, 1, rays, hits));
	REFUSE(bare, pwn_trace_hits(bare, 1, rays, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, rays, 0, hits, NULL));
	REFUSE(bare, pwn_trace_hits_device(bare, 0, NULL, 0, NULL, NULL));
	REFUSE(bare, pwn_trace_hits_device(bare, 1, rays, 2, hits, NULL));
	bare->tiled = NULL; odd->tiled = NULL; c->tiled = NULL; wide->tiled = NULL;

	REFUSE(c, pwn_trace_views_device(NULL, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, NULL, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, NULL, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work, NULL, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work, sbuf, NULL, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, NULL, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 0, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, PWN_VIEWS_MAX + 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 2, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams + 1, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs + 1, 0, work, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work + 1, sbuf, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work, sbuf + 2, zbuf, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, work, sbuf, zbuf + 3, NULL));
	REFUSE(c, pwn_trace_views_device(c, 2, dcams, dsecs, 0, work, sbuf, (float *)(sbuf + PLANE), NULL));
	REFUSE(c, pwn_trace_views_device(c, 2, dcams, dsecs, 0, work + PLANE, sbuf, (float *)work, NULL));
	REFUSE(c, pwn_trace_views_device(c, 1, dcams, dsecs, 0, sbuf, sbuf, zbuf, NULL));
	REFUSE(wide, pwn_trace_views_device(wide, PWN_VIEWS_MAX, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(odd, pwn_trace_views_device(odd, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));
	REFUSE(bare, pwn_trace_views_device(bare, 1, dcams, dsecs, 0, work, sbuf, zbuf, NULL));

	REFUSE(c, pwn_trace_viewports(NULL, 1, all, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 1, NULL, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 1, all, NULL, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 1, all, cams, NULL, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 1, all, cams, secs, NULL, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 0, all, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, PWN_VIEWS_MAX + 1, all, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 2, badvp, cams, secs, sbuf, zbuf));
	REFUSE(c, pwn_trace_viewports(c, 1, oddvp, cams, secs, sbuf, zbuf));
	REFUSE(odd, pwn_trace_viewports(odd, 1, badvp, cams, secs, sbuf, zbuf));
	REFUSE(bare, pwn_trace_viewports(bare, 1, all, cams, secs, sbuf, zbuf));

	REFUSE(c, pwn_trace_rays(NULL, 1, rays, seeds, 0, col, depth));
	REFUSE(c, pwn_trace_rays(c, -1, rays, seeds, 0, col, depth));
	REFUSE(c, pwn_trace_rays(c, PWN_RAYS_MAX + 1, rays, seeds, 0, col, depth));
	REFUSE(c, pwn_trace_rays(c, 1, NULL, seeds, 0, col, depth));
	REFUSE(c, pwn_trace_rays(c, 1, rays, seeds, 0, NULL, NULL));
	REFUSE(c, pwn_trace_rays(c, 0, NULL, NULL, 0, NULL, NULL));
	REFUSE(bare, pwn_trace_rays(bare, 1, rays, seeds, 0, col, depth));
	REFUSE(bare, pwn_trace_rays(bare, 0, NULL, NULL, 0, col, NULL));
	REFUSE(c, pwn_trace_rays_device(NULL, 1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, -1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, PWN_RAYS_MAX + 1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, NULL, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 0, NULL, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 0, col, NULL, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 2, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays + 1, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, (uint32_t *)((char *)seeds + 2), 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 0, (uint32_t *)((char *)col + 1), depth, NULL));
	REFUSE(c, pwn_trace_rays_device(c, 1, rays, seeds, 0, 0, col, (float *)((char *)depth + 2), NULL));
	REFUSE(bare, pwn_trace_rays_device(bare, 1, rays, seeds, 0, 0, col, depth, NULL));
	REFUSE(c, pwn_trace_hits(NULL, 1, rays, hits));
	REFUSE(c, pwn_trace_hits(c, -1, rays, hits));
	REFUSE(c, pwn_trace_hits(c, PWN_RAYS_MAX + 1, rays, hits));
	REFUSE(c, pwn_trace_hits(c, 1, NULL, hits));
	REFUSE(c, pwn_trace_hits(c, 1, rays, NULL));
	REFUSE(bare, pwn_trace_hits(bare, 1, rays, hits));
	REFUSE(bare, pwn_trace_hits(bare, 0, NULL, NULL));
	REFUSE(c, pwn_trace_hits_device(NULL, 1, rays, 0, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, -1, rays, 0, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, PWN_RAYS_MAX + 1, rays, 0, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, NULL, 0, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, rays, 0, NULL, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, rays, 2, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, rays + 2, 0, hits, NULL));
	REFUSE(c, pwn_trace_hits_device(c, 1, rays, 0, (char *)hits + 8, NULL));
	REFUSE(bare, pwn_trace_hits_device(bare, 1, rays, 0, hits, NULL));

	// ---- no memory: the k-th allocation of the call fails; a smaller call afterwards is served
	g_c = m;
	REQ(CALL("pwn_trace_views n 1 (a context of its own)", pwn_trace_views(m, 1, cams, secs, sbuf, zbuf)) == PWN_OK);
	for(int k = 1; k <= 3; k++)
	{
		fakehip_alloc_fail_in = k;
		snprintf(what, sizeof(what), "pwn_trace_views n 3, allocation %d fails", k);
		REQ(CALL(what, pwn_trace_views(m, 3, cams, secs, sbuf, zbuf)) == PWN_ENOMEM);
		fakehip_alloc_fail_in = 0;
		REQ(CALL("pwn_trace_views n 1 afterwards", pwn_trace_views(m, 1, cams, secs, sbuf, zbuf)) == PWN_OK);
		out("sbuf", sbuf, PLANE * 4);
	}
	// (the viewport records are two allocations in front of the three planes)
	REQ(CALL("pwn_trace_viewports", (fakehip_alloc_fail_in = 3, pwn_trace_viewports(m, 1, all, cams, secs, sbuf, zbuf))) == PWN_ENOMEM);
	for(int k = 2; k <= 3; k++)
	{
		fakehip_alloc_fail_in = k;
		snprintf(what, sizeof(what), "pwn_trace_viewports, allocation %d fails", k);
		REQ(CALL(what, pwn_trace_viewports(m, 1, all, cams, secs, sbuf, zbuf)) == PWN_ENOMEM);
	}
	fakehip_alloc_fail_in = 0;
	REQ(CALL("pwn_trace_viewports afterwards", pwn_trace_viewports(m, 1, all, cams, secs, sbuf, zbuf)) == PWN_OK);
	out("sbuf", sbuf, PLANE * 4);
	REQ(CALL("pwn_trace_rays n 65 (a context of its own)", pwn_trace_rays(m, 65, rays, seeds, 0.0f, col, depth)) == PWN_OK);
	REQ(CALL("pwn_trace_hits n 65 (a context of its own)", pwn_trace_hits(m, 65, rays, hits)) == PWN_OK);
	for(int k = 1; k <= 2; k++)
	{
		fakehip_alloc_fail_in = k;
		snprintf(what, sizeof(what), "pwn_trace_rays n 5000, allocation %d fails", k);
		REQ(CALL(what, pwn_trace_rays(m, 5000, rays, seeds, 0.0f, col, depth)) == PWN_ENOMEM);
		fakehip_alloc_fail_in = k;
		snprintf(what, sizeof(what), "pwn_trace_hits n 5000, allocation %d fails", k);
		REQ(CALL(what, pwn_trace_hits(m, 5000, rays, hits)) == PWN_ENOMEM);
		fakehip_alloc_fail_in = 0;
		REQ(CALL("pwn_trace_rays n 65 afterwards", pwn_trace_rays(m, 65, rays, seeds, 0.0f, col, depth)) == PWN_OK);
		out("col", col, 4 * 65);
		REQ(CALL("pwn_trace_hits n 65 afterwards", pwn_trace_hits(m, 65, rays, hits)) == PWN_OK);
		out("hits", hits, sizeof(pwn_hit) * 65);
	}
	REQ(CALL("pwn_trace_rays n 5000 afterwards", pwn_trace_rays(m, 5000, rays, seeds, 0.0f, col, depth)) == PWN_OK);
	REQ(CALL("pwn_trace_hits n 5000 afterwards", pwn_trace_hits(m, 5000, rays, hits)) == PWN_OK);


	// ---- the branches of the trace launcher that 96 x 64 frames on four CUs do not reach
	{
		reg("big_s", big_s.data(), big_s.size() * 4); reg("big_z", big_z.data(), big_z.size() * 4);
		const char *lv = argv[1];
		pwn_ctx *x;
		section("512 x 160, 1280 units = 16 * 4 * grid: tile pairs; a strip with y0 > 0");
		x = ctx_env(512, 160, lv, sph);
		rows(x, cams, 0, 160); rows(x, cams, 40, 120); rows(x, cams, 80, 80);
		section("the same context: a number of PWN_OPT_TRACE_ROOM, one too large to take, the row tiling's reserve above it");
		opt(x, PWN_OPT_TRACE_ROOM, 4); rows(x, cams, 0, 160);
		opt(x, PWN_OPT_TRACE_ROOM, 10); rows(x, cams, 0, 160);
		opt(x, PWN_OPT_TRACE_ROOM, 4); x->grid_reserve = 6; rows(x, cams, 0, 160);
		x->grid_reserve = 0; opt(x, PWN_OPT_TRACE_ROOM, -1);
		section("the same context: counters on");
		opt(x, PWN_OPT_COUNTERS, 1); rows(x, cams, 0, 160); rows(x, cams + 48, 0, 160); opt(x, PWN_OPT_COUNTERS, 0);
		section("the same context: the wave log follows the grid; with PWN_DBG_UNIT_COST the launch writes the units' costs");
		opt(x, PWN_OPT_WAVE_LOG, 1); rows(x, cams, 0, 8); rows(x, cams, 0, 160);
		REQ(CALL("pwn_trace_rays_device n 65 (a batch writes no wave log)", pwn_trace_rays_device(x, 65, rays, seeds, secs[2], 0, col, depth, x->stream)) == PWN_OK);
		setenv("PWN_DBG_UNIT_COST", "/dev/null", 1); rows(x, cams, 0, 160); unsetenv("PWN_DBG_UNIT_COST");
		opt(x, PWN_OPT_WAVE_LOG, 0);
		section("the same context: a launch on the second stream waits for the launch two before it; tables whose upload is not through");
		rows(x, cams, 0, 160); rows(x, cams, 0, 160, x->stream2);
		printf(" | launch_waits %llu", x->launch_waits);
		REQ(pwn_upload_spheres(x, sph.data(), 11) == PWN_OK);
		fakehip_query_busy = 1; rows(x, cams, 0, 160); fakehip_query_busy = 0; rows(x, cams, 0, 160);
		section("the same context: the refill scheduler (the tables are packed again)");
		opt(x, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL); rows(x, cams, 0, 160); rows(x, cams + 48, 0, 160);
		REQ(CALL("pwn_trace_rays_device n 65 (a batch runs the units scheduler)", pwn_trace_rays_device(x, 65, rays, seeds, secs[2], 0, col, depth, x->stream)) == PWN_OK);
		opt(x, PWN_OPT_SCHEDULER, PWN_SCHED_DEFAULT);
		section("the same context: PWN_OPT_UNIT_ORDER keeps single units; the buffers grow, the sorted order is used for the same rows");
		opt(x, PWN_OPT_UNIT_ORDER, 1);
		rows(x, cams, 0, 40); rows(x, cams, 0, 160); blur_rows(x); rows(x, cams, 0, 160); rows(x, cams, 40, 120);
		printf(" | order_used %llu order_sorts %llu", x->order_used, x->order_sorts);
		// (the order of rows 0 .. 80: not for as many units of other rows)
		rows(x, cams, 0, 80); blur_rows(x); rows(x, cams, 40, 120); rows(x, cams, 0, 78); rows(x, cams, 0, 80);
		printf(" | order_used %llu order_sorts %llu", x->order_used, x->order_sorts);
		opt(x, PWN_OPT_UNIT_ORDER, 0);
		section("the same context: a frame slot's event guards a copy of the tables until the slot's next frame");
		fakehip_call_hook = NULL;
		REQ(pwn_frames_config(x, 1, 0, 0, 0) == PWN_OK);
		fakehip_call_hook = on_call;
		REQ(CALL("pwn_submit_frame slot 0", pwn_submit_frame(x, cams, 0.5f, 0)) == PWN_OK);
		REQ(pwn_upload_spheres(x, sph.data(), 12) == PWN_OK);
		REQ(CALL("pwn_wait_frame slot 0", pwn_wait_frame(x, 0, NULL)) == PWN_OK);
		REQ(CALL("pwn_submit_frame slot 0, new tables", pwn_submit_frame(x, cams, 1.0f, 0)) == PWN_OK);
		for(int i = 0; i < PWN_NBLOB; i++) printf(" | in_use[%d] %d", i, (int)x->tables_in_use[i]);
		REQ(CALL("pwn_wait_frame slot 0", pwn_wait_frame(x, 0, NULL)) == PWN_OK);
		g_c = NULL; pwn_destroy(x);
		section("496 x 160, 1240 units: no pairs");
		x = ctx_env(496, 160, lv, sph); rows(x, cams, 0, 160); g_c = NULL; pwn_destroy(x);
		section("528 x 160, 33 units a row: pairs, the last tile of a row half empty");
		x = ctx_env(528, 160, lv, sph); rows(x, cams, 0, 160); g_c = NULL; pwn_destroy(x);
		section("32768 x 16: the first round's rows are the fifth of the rows");
		x = ctx_env(32768, 16, lv, sph); rows(x, cams, 0, 16); g_c = NULL; pwn_destroy(x);
		section("PWN_TILE_PAIRS=2 at 96 x 64 and at 16 x 64 (one unit a row)");
		x = ctx_env(96, 64, lv, sph, { "PWN_TILE_PAIRS", "2" }); rows(x, cams, 0, 64); g_c = NULL; pwn_destroy(x);
		x = ctx_env(16, 64, lv, sph, { "PWN_TILE_PAIRS", "2" }); rows(x, cams, 0, 64); g_c = NULL; pwn_destroy(x);
		section("PWN_TILE_PAIRS=0 at 512 x 160");
		x = ctx_env(512, 160, lv, sph, { "PWN_TILE_PAIRS", "0" }); rows(x, cams, 0, 160); g_c = NULL; pwn_destroy(x);
		section("PWN_DBG_BLOCKS_PER_CU=2 at 512 x 160");
		x = ctx_env(512, 160, lv, sph, { "PWN_DBG_BLOCKS_PER_CU", "2" }); rows(x, cams, 0, 160); g_c = NULL; pwn_destroy(x);
		section("PWN_SCHEDULER=refill and PWN_DBG_FORCE_HASW at 96 x 64; more workgroups than units");
		x = ctx_env(96, 64, lv, sph, { "PWN_SCHEDULER", "refill", "PWN_DBG_FORCE_HASW", "1" }); rows(x, cams, 0, 64); rows(x, cams, 0, 8); g_c = NULL; pwn_destroy(x);
		section("PWN_SPHERE_LISTS=global at 512 x 160, also under the refill scheduler");
		x = ctx_env(512, 160, lv, sph, { "PWN_SPHERE_LISTS", "global" }); rows(x, cams, 0, 160);
		opt(x, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL); opt(x, PWN_OPT_UNIT_ORDER, 1); rows(x, cams, 0, 160); g_c = NULL; pwn_destroy(x);
		// 240 spheres, 40 of them in one cell: a blob of which four fit a CU's LDS where the occupancy query says five, and a list with a ball
		std::vector<pwn_sphere> many;
		for(int i = 0; i < 200; i++) many.push_back({ 0.1f + 0.3f * rnd(), rnd(), 2.0f + 20.0f * rnd(), rnd(), 2.0f + 20.0f * rnd(), rnd(), rnd(), rnd() });
		for(int i = 0; i < 40; i++) many.push_back({ 0.05f, rnd(), 5.25f + 0.5f * rnd(), 0.5f, 5.25f + 0.5f * rnd(), rnd(), rnd(), rnd() });
		section("240 spheres at 96 x 64: the LDS rule caps the workgroups per CU; the longest lists' balls, and PWN_SPHERE_BOUNDS=0");
		x = ctx_env(96, 64, lv, many); rows(x, cams, 0, 64); g_c = NULL; pwn_destroy(x);
		x = ctx_env(96, 64, lv, many, { "PWN_SPHERE_BOUNDS", "0" }); rows(x, cams, 0, 64); g_c = NULL; pwn_destroy(x);
		g_c = c;
	}

	pwn_fake_trace_hook = NULL; pwn_fake_blur_hook = NULL; pwn_fake_launch_hook = NULL; fakehip_call_hook = NULL;
	g_c = NULL;
	pwn_destroy(m); pwn_destroy(wide); pwn_destroy(odd); pwn_destroy(bare); pwn_destroy(c);
	close_line();
	printf("ok\n");
	return 0;
}
