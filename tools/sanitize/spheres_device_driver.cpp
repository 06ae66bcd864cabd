// spheres_device_driver.cpp -- the host side of pwn_upload_spheres_device on the CPU, under AddressSanitizer + UBSan:
// pwn_spheres_device.cpp against the stand-in runtime and a stand-in for the build's launches (fake_kernels.cpp) that reads and writes
// exactly the ranges the kernels do ("device" memory is malloc'ed to the byte: a section that is off or too short is a report).
// What is looked at: every pointer and size a build and the trace launches behind it are handed lies inside what was reserved, for
// growing and shrinking n / max_pairs; the tables a launch reads, walked as trace_walk.inc walks them, are pwn_bin_spheres' lists of
// the spheres given; eight builds in a row go twice round the copies; the overflow tables hold no sphere; every refusal launches
// nothing; pwn_upload_spheres, pwn_prepare_render and a level call bring the host's table back and a scheduler change does not;
// the base copy travels once per level; pwn_stats and pwn_launch_order_waits as they were; no leak behind pwn_destroy.
//     spheres_device_asan        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "pwn_internal.h"
#include "level_host.h"

extern "C" {
extern void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);
extern void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes);
extern void (*pwn_fake_sphere_bins_hook)(const void *d_scratch, const void *d_base, const void *d_blob);
extern void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern long fakehip_alloc_fail_in;
}
#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)

static std::map<const void *, size_t> g_alloc;          // what the runtime handed out, to the byte
static int g_waits, g_syncs;
static std::vector<std::pair<const void *, const void *>> g_waited;          // (stream, event) of every hipStreamWaitEvent
static bool waited(const void *s, const void *e) { for(auto &w : g_waited) if(w.first == s && w.second == e) return true; return false; }
static void on_hip(const char *name, const void *a, const void *b, size_t bytes)
{
	if(strcmp(name, "hipStreamWaitEvent") == 0) g_waited.push_back({ a, b });
	if((strcmp(name, "hipMalloc") == 0 || strcmp(name, "hipHostMalloc") == 0) && a != NULL) g_alloc[a] = bytes;
	if(strcmp(name, "hipFree") == 0 || strcmp(name, "hipHostFree") == 0) g_alloc.erase(a);
	if(strcmp(name, "hipStreamWaitEvent") == 0) g_waits++;
	if(strcmp(name, "hipDeviceSynchronize") == 0 || strcmp(name, "hipStreamSynchronize") == 0 || strcmp(name, "hipEventSynchronize") == 0) g_syncs++;
}
static size_t room(const void *p) { auto it = g_alloc.find(p); return it == g_alloc.end() ? 0 : it->second; }

static int g_builds, g_uploads, g_other;
static size_t g_b_n, g_b_mp;
static const void *g_b_src, *g_b_big, *g_b_blob;
static void on_launch(const char *name, const void *src, const void *dst, int ns, const size_t *sizes)
{
	if(strcmp(name, "sphere_bins") == 0)
	{
		REQ(ns == 4);
		g_builds++; g_b_src = src; g_b_big = dst; g_b_n = sizes[0]; g_b_mp = sizes[1];
		REQ(sizes[2] == pwn_g_which_offset(g_b_mp) && sizes[3] == pwn_g_sph_offset(g_b_mp));
		REQ(room(dst) >= pwn_g_total(g_b_mp, g_b_n));          // the device-memory part as laid out fits what was reserved
	}
	else if(strcmp(name, "upload") == 0) g_uploads++;
	else g_other++;
}
static void on_bins(const void *d_scratch, const void *d_base, const void *d_blob)
{
	REQ(room(d_scratch) == PWN_SD_SCRATCH_BYTES && room(d_base) == PWN_T_BINIDX);
	REQ(room(d_blob) >= pwn_t_total_glb(g_b_mp < 4096 ? (uint32_t)g_b_mp : 4096u));
	g_b_blob = d_blob;
}

// what the next trace launch is to find: device-built tables of these spheres under this capacity, or (dev = false) the host's
static bool g_dev;
static std::vector<pwn_sphere> g_exp;
static int g_exp_mp, g_checked;
static const void *g_last_blob;
static pwn_ctx *g_ctx;
static void check_tables(const pwn_trace_params *P, int, size_t lds_bytes)
{
	g_checked++;
	g_last_blob = P->blob;
	REQ(lds_bytes == P->blob_bytes + 16 && P->blob_bytes % 16 == 0);
	if(!g_dev) { REQ(g_ctx->sd.in_force == false); return; }
	const int n = (int)g_exp.size();
	std::vector<int32_t> off(4097, 0);
	const int nb = pwn_bin_spheres(g_exp.data(), n, off.data(), NULL, 0);
	std::vector<int32_t> idx((size_t)(nb > 0 ? nb : 1));
	REQ(pwn_bin_spheres(g_exp.data(), n, off.data(), idx.data(), nb) == nb);
	uint32_t longest = 0;
	for(int c = 0; c < 4096; c++) if((uint32_t)(off[c + 1] - off[c]) > longest) longest = (uint32_t)(off[c + 1] - off[c]);
	const bool over = nb > g_exp_mp || longest > PWN_LIST_MAX;
	const uint32_t cap_cells = g_exp_mp < 4096 ? (uint32_t)g_exp_mp : 4096u;
	REQ(P->g_rec != NULL && P->nbounds == 0 && P->off_sph == 0 && P->off_recsph == 0);
	REQ(P->blob_bytes == pwn_t_total_glb(cap_cells) && room(P->blob) >= P->blob_bytes);
	REQ((const uint8_t *)P->g_which - (const uint8_t *)P->g_rec == (ptrdiff_t)pwn_g_which_offset((uint64_t)g_exp_mp));
	REQ((const uint8_t *)P->g_sph - (const uint8_t *)P->g_rec == (ptrdiff_t)pwn_g_sph_offset((uint64_t)g_exp_mp));
	REQ(room(P->g_rec) >= pwn_g_total((uint64_t)g_exp_mp, (uint64_t)n));
	const uint8_t *blob = (const uint8_t *)P->blob;
	const uint32_t *ci = (const uint32_t *)(blob + PWN_T_CELLINFO), *liststart = (const uint32_t *)(blob + PWN_T_BINIDX);
	// the level's part is the host's, byte for byte
	REQ(memcmp(blob + PWN_T_RCP, g_ctx->tabs, 8192) == 0 && memcmp(blob + PWN_T_EPREC, g_ctx->ep_recs, sizeof(g_ctx->ep_recs)) == 0);
	uint32_t ord_seen = 0; int k = 0;
	for(int z = 0; z <= 64; z++) for(int x = 0; x <= 64; x++)
	{
		const uint32_t cw = ci[z * 65 + x], base = g_ctx->cell_base[z * 65 + x];
		const int c = z * 64 + x;
		const int cnt = (z < 64 && x < 64 && !over) ? off[c + 1] - off[c] : 0;
		if(cnt == 0) { REQ(cw == base); continue; }
		const uint32_t ord = (cw >> 16) & 0x7fffu;
		REQ(cw == (base | PWN_C_SPH | (ord << 16)) && ord == ord_seen && ord < cap_cells); ord_seen++;
		uint32_t ri = liststart[ord];
		REQ(ri == (uint32_t)off[c]);
		for(int j = 0; j < cnt; j++, ri++, k++)
		{
			REQ(ri + 1u <= (uint32_t)g_exp_mp);          // the read-ahead record lies inside the section
			const float *r = P->g_rec + 4 * (size_t)ri;
			uint32_t wb, rb; memcpy(&wb, &r[3], 4);
			REQ(((wb >> 31) != 0) == (j == cnt - 1));
			const uint32_t which = P->g_which[ri];
			REQ(which == (uint32_t)idx[off[c] + j]);
			const pwn_sphere &q = g_exp[which];
			float r2 = q.r * q.r; if(r2 < 1.17549435e-38f) r2 = 0.0f;
			memcpy(&rb, &r2, 4);
			REQ(memcmp(&r[0], &q.x, 12) == 0 && (wb & 0x7fffffffu) == (rb & 0x7fffffffu));
			const float *s = P->g_sph + 8 * (size_t)which;
			REQ(memcmp(&s[0], &q.x, 12) == 0 && memcmp(&s[3], &r2, 4) == 0 && memcmp(&s[4], &q.refl, 4) == 0 && memcmp(&s[5], &q.cb, 12) == 0);
		}
	}
	REQ(over || k == nb);
}

static const char *LEVEL = "###########\r\n#;;;;;;;;;#\r\n#;;*;;;;;;#\r\n#;;;;$$;;;#\r\n#;a;;;;;b;#\r\n#;;;;;;;;;#\r\n###########\r\n";
static const char *LEVEL2 = "#########\r\n#;;;;;;;#\r\n#;;*;$;;#\r\n#;;;;;;;#\r\n#########\r\n";
static unsigned rs = 777; static float rnd() { rs = rs * 1664525u + 1013904223u; return (float)(rs >> 8) / 16777216.0f; }
static void make(std::vector<pwn_sphere> &s, int n, float rlo, float rhi, float span)
{
	s.clear();
	for(int i = 0; i < n; i++) { pwn_sphere q = { rlo + (rhi - rlo) * rnd(), rnd(), -2.0f + span * rnd(), rnd(), -2.0f + span * rnd(), rnd(), rnd(), rnd() }; s.push_back(q); }
}
static int pairs_of(const std::vector<pwn_sphere> &s)
{
	std::vector<int32_t> off(4097, 0);
	return pwn_bin_spheres(s.data(), (int)s.size(), off.data(), NULL, 0);
}

int main()
{
	fakehip_call_hook = on_hip;
	pwn_fake_launch_hook = on_launch;
	pwn_fake_sphere_bins_hook = on_bins;
	pwn_fake_trace_hook = check_tables;
	pwn_ctx *c = NULL, *bare = NULL;
	REQ(pwn_init(&c, 0, 64, 48) == PWN_OK && pwn_init(&bare, 0, 64, 48) == PWN_OK);
	g_ctx = c;
	REQ(pwn_level_load_mem(c, LEVEL, (int)strlen(LEVEL)) == PWN_OK);
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
	std::vector<uint32_t> sb(64 * 48); std::vector<float> zb(64 * 48);
	const float cam[16] = { 1,0,0,0, 0,1,0,0, 0,0,1,0, 3.5f,0.5f,2.5f,1 };
	unsigned long long st[8], ts[6];
	REQ(pwn_spheres_device_state(c, st) == PWN_OK);
	for(int i = 0; i < 8; i++) REQ(st[i] == 0);
	pwn_stats s0, s1; unsigned long long w0 = 0, w1 = 0;

	// the host's table, which the device builds must leave alone
	std::vector<pwn_sphere> host;
	make(host, 9, .1f, .3f, 8);
	REQ(pwn_upload_spheres(c, host.data(), 9) == PWN_OK);
	g_dev = false;
	REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
	REQ(pwn_get_stats(c, &s0) == PWN_OK && pwn_launch_order_waits(c, &w0) == PWN_OK);

	// ---- growing and shrinking n / max_pairs; a launch behind every build reads the tables
	struct { int n; float rlo, rhi, span; int slack; } cases[] = { { 14, .1f, .3f, 8, 0 }, { 2100, .02f, .4f, 40, 100 }, { 0, 0, 0, 0, 0 }, { 1, .2f, .2f, 6, 5000 },
		{ 10000, .02f, .2f, 66, 7 }, { 65, 3.f, 9.f, 66, 0 }, { 800, 1.5f, 4.f, 66, 100000 }, { 14, .1f, .3f, 8, 1 }, { 3, 100.f, 100.f, 10, 0 } };
	std::vector<pwn_sphere> s;
	int uploads0 = g_uploads, ncase = 0;
	const void *blobs[16];
	for(auto &k : cases)
	{
		make(s, k.n, k.rlo, k.rhi, k.span);
		const int pairs = pairs_of(s), mp = pairs + k.slack;
		// (the records sit in a block of exactly their size: a read behind them is a report)
		std::vector<pwn_sphere> devmem(s);
		const int b0 = g_builds, sy0 = g_syncs;
		REQ(pwn_upload_spheres_device(c, k.n, devmem.data(), mp, ncase & 1 ? (void *)c->stream : NULL) == PWN_OK);
		REQ(g_builds == b0 + 1 && g_b_n == (size_t)k.n && g_b_mp == (size_t)mp && (k.n == 0 || g_b_src == devmem.data()));
		REQ(g_b_blob == c->d_blob[c->blob_cur] && g_b_big == c->d_big[c->blob_cur]);
		blobs[ncase] = g_b_blob;
		REQ(g_uploads == uploads0 + 1);          // the base copy: with the first build of the level, then never
		(void)sy0;
		g_dev = true; g_exp = s; g_exp_mp = mp;
		const int ch0 = g_checked;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(g_checked > ch0 && g_last_blob == g_b_blob);
		REQ(g_uploads == uploads0 + 1);                              // ... and no launch repacked anything
		REQ(pwn_spheres_device_state(c, st) == PWN_OK);
		REQ(st[0] == 1 && st[1] == (unsigned long long)k.n && st[2] == (unsigned long long)mp && st[3] == (unsigned long long)pairs && st[6] == 0 && st[7] == (unsigned long long)(ncase + 1));
		REQ(pwn_sphere_tables_state(c, ts) == PWN_OK);
		REQ(ts[0] == 2 && ts[1] == pwn_t_total_glb(mp < 4096 ? (uint32_t)mp : 4096u) + 16 && ts[2] == pwn_g_total((uint64_t)mp, (uint64_t)k.n));
		REQ(ts[3] == (unsigned long long)mp && ts[4] == (unsigned long long)(mp < 4096 ? mp : 4096) && ts[5] == (unsigned long long)(mp < PWN_LIST_MAX ? mp : PWN_LIST_MAX));
		// the host's queries go on describing the host's table
		std::vector<pwn_sphere> got(16);
		REQ(pwn_get_objects(c, got.data(), 16) == 9 && memcmp(got.data(), host.data(), 9 * sizeof(pwn_sphere)) == 0);
		std::vector<uint16_t> counts(4096);
		REQ(pwn_get_bins(c, counts.data(), NULL, 0) == pairs_of(host));
		ncase++;
	}
	// (nine builds: twice round the four copies and one more)
	for(int i = 4; i < ncase; i++) REQ(blobs[i] == blobs[i - 4]);
	for(int i = 1; i < 4; i++) for(int j = 0; j < i; j++) REQ(blobs[i] != blobs[j]);

	// ---- a build that fits allocates nothing and synchronises nothing; eight in a row
	{
		make(s, 300, .05f, .6f, 60);
		const int mp = pairs_of(s);
		const size_t allocs0 = g_alloc.size();
		std::map<const void *, size_t> before(g_alloc);
		const int sy0 = g_syncs;
		for(int i = 0; i < 8; i++) REQ(pwn_upload_spheres_device(c, 300, s.data(), mp, c->stream2) == PWN_OK);
		REQ(g_alloc.size() == allocs0 && g_alloc == before && g_syncs == sy0);
		g_dev = true; g_exp = s; g_exp_mp = mp;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
	}

	// ---- the build waits ON ITS STREAM for what still reads the copy it takes: the launches (tables_wait), the players' steps (ev_walk)
	// -- and the upload stream is put behind the build
	{
		make(s, 14, .1f, .3f, 8);
		std::vector<float> cams(16, 0.0f), grav(4, 0.0f); uint8_t key = 0;
		cams[0] = cams[5] = cams[10] = cams[15] = 1.0f; cams[12] = 3.5f; cams[14] = 2.5f;
		for(int i = 0; i < 2 * PWN_NBLOB; i++)
		{
			// a frame and a step read the copy in force, on the context's stream; three more builds later the ring is back at it
			g_dev = true; g_exp = s; g_exp_mp = 100;
			if(i == 0) REQ(pwn_upload_spheres_device(c, 14, s.data(), 100, NULL) == PWN_OK);
			REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
			REQ(pwn_players_step_device(c, 1, &key, 0.01f, 1, cams.data(), grav.data(), NULL, c->stream) == PWN_OK);
			const int nb = (c->blob_cur + 1) % PWN_NBLOB;
			const bool in_use = c->tables_in_use[nb], walk = c->walk_in_use[nb];
			const hipEvent_t ev_t = c->tables_wait[nb], ev_w = c->ev_walk[nb];
			g_waited.clear();
			REQ(pwn_upload_spheres_device(c, 14, s.data(), 100, c->stream2) == PWN_OK && c->blob_cur == nb);
			if(in_use) REQ(waited(c->stream2, ev_t));
			if(walk) REQ(waited(c->stream2, ev_w) && !c->walk_in_use[nb]);
			REQ(waited(c->up_stream, c->ev_upload[nb]));
			if(i >= PWN_NBLOB) REQ(in_use && walk);          // (from the second round on every copy has had its readers)
		}
	}

	// ---- capacity: one pair short, and a list longer than PWN_LIST_MAX
	{
		make(s, 200, .3f, .9f, 30);
		const int pairs = pairs_of(s);
		REQ(pwn_upload_spheres_device(c, 200, s.data(), pairs - 1, NULL) == PWN_OK);
		g_dev = true; g_exp = s; g_exp_mp = pairs - 1;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_spheres_device_state(c, st) == PWN_OK && st[0] == 1 && st[3] == (unsigned long long)pairs && st[6] == 1);
		make(s, PWN_LIST_MAX + 1, .1f, .1f, 0.0f);
		for(auto &q : s) { q.x = 5.5f; q.z = 5.5f; }
		REQ(pwn_upload_spheres_device(c, (int)s.size(), s.data(), 3 * PWN_LIST_MAX, NULL) == PWN_OK);
		g_exp = s; g_exp_mp = 3 * PWN_LIST_MAX;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_spheres_device_state(c, st) == PWN_OK && st[3] == PWN_LIST_MAX + 1 && st[4] == 1 && st[5] == PWN_LIST_MAX + 1 && st[6] == 2);
		s.pop_back();
		REQ(pwn_upload_spheres_device(c, (int)s.size(), s.data(), PWN_LIST_MAX, NULL) == PWN_OK);
		g_exp = s; g_exp_mp = PWN_LIST_MAX;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_spheres_device_state(c, st) == PWN_OK && st[5] == PWN_LIST_MAX && st[6] == 0);
	}

	// ---- refusals: nothing launched, the tables in force as they were
	{
		make(s, 14, .1f, .3f, 8);
		const int mp = pairs_of(s);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), mp, NULL) == PWN_OK);
		g_dev = true; g_exp = s; g_exp_mp = mp;
		const int b0 = g_builds, u0 = g_uploads, o0 = g_other, cur0 = c->blob_cur;
		const std::map<const void *, size_t> before(g_alloc);
		REQ(pwn_upload_spheres_device(NULL, 14, s.data(), mp, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, -1, s.data(), mp, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, PWN_OBJ_MAX + 1, s.data(), mp, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), -1, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, 14, NULL, mp, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, 14, (const char *)s.data() + 4, mp, NULL) == PWN_EINVAL);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), (int)(PWN_TABLES_MAX / 20u) + 1, NULL) == PWN_ETOOBIG);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 0x7fffffff, NULL) == PWN_ETOOBIG);
		REQ(pwn_upload_spheres_device(bare, 14, s.data(), mp, NULL) == PWN_ENOLEVEL);
		REQ(pwn_upload_spheres_device(bare, 0, NULL, 0, NULL) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(pwn_upload_spheres_device(c, 14, s.data(), mp, NULL) == PWN_EBUSY);
		REQ(pwn_spheres_device_state(c, st) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(pwn_spheres_device_state(NULL, st) == PWN_EINVAL && pwn_spheres_device_state(c, NULL) == PWN_EINVAL);
		{
			const int devs[2] = { 0, 0 };
			pwn_ctx *g = NULL;
			REQ(pwn_init_multi(&g, devs, 2, 64, 48) == PWN_OK);
			const int b1 = g_builds;
			REQ(pwn_upload_spheres_device(g, 14, s.data(), mp, NULL) == PWN_ENOTSUP && pwn_spheres_device_state(g, st) == PWN_ENOTSUP);
			REQ(g_builds == b1);
			pwn_destroy(g);
		}
		REQ(g_builds == b0 && g_uploads == u0 && g_other == o0 && c->blob_cur == cur0 && g_alloc == before);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);          // (still the 14 spheres' tables)
		// a buffer that cannot grow: refused, the tables as they were
		fakehip_alloc_fail_in = 1;
		REQ(pwn_upload_spheres_device(c, 14, s.data(), (int)(PWN_TABLES_MAX / 20u) - 64, NULL) == PWN_ENOMEM);
		fakehip_alloc_fail_in = 0;
		REQ(g_builds == b0 && c->blob_cur == cur0);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
	}

	// ---- who owns the tables: a scheduler change repacks nothing; the host's calls bring the host's table back
	{
		const int u0 = g_uploads, b0 = g_builds;
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL) == PWN_OK);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_UNITS) == PWN_OK);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(g_uploads == u0 && g_builds == b0 && c->sd.in_force);
		REQ(pwn_upload_spheres(c, host.data(), 9) == PWN_OK);
		g_dev = false;
		REQ(g_uploads == u0 + 1 && !c->sd.in_force);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_spheres_device_state(c, st) == PWN_OK && st[0] == 0 && st[1] == 14);
		REQ(pwn_sphere_tables_state(c, ts) == PWN_OK && ts[0] != 2 && ts[3] == (unsigned long long)pairs_of(host));
		// (a scheduler change with the host's tables in force repacks, as ever)
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL) == PWN_OK);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(g_uploads == u0 + 2);
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_UNITS) == PWN_OK);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, NULL) == PWN_OK && c->sd.in_force);
		REQ(pwn_prepare_render(c) == PWN_OK && !c->sd.in_force);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, NULL) == PWN_OK && c->sd.in_force);
		// a level call: the host's table again, and the next build brings a base copy of the NEW level first
		const int u1 = g_uploads;
		REQ(pwn_level_load_mem(c, LEVEL2, (int)strlen(LEVEL2)) == PWN_OK && !c->sd.in_force);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		const int u2 = g_uploads;
		REQ(u2 > u1);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, NULL) == PWN_OK);
		REQ(g_uploads == u2 + 1);
		g_dev = true; g_exp = s; g_exp_mp = 4000;
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);          // (cell words of LEVEL2 under the spheres)
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, NULL) == PWN_OK && g_uploads == u2 + 1);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
	}

	// ---- a players' step reads the walk table of the copy a build made current: handed on, never sent again
	{
		std::vector<float> cams(16, 0.0f), grav(4, 0.0f); uint8_t key = 0;
		cams[0] = cams[5] = cams[10] = cams[15] = 1.0f; cams[12] = 3.5f; cams[14] = 2.5f;
		const int u0 = g_uploads;
		for(int i = 0; i < 6; i++)
		{
			REQ(pwn_players_step_device(c, 1, &key, 0.01f, 1, cams.data(), grav.data(), NULL, c->stream) == PWN_OK);
			REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, i & 1 ? (void *)c->stream : (void *)c->stream2) == PWN_OK);
		}
		REQ(g_uploads == u0);
		for(int i = 0; i < PWN_NBLOB; i++) REQ(c->walk_of[i] == c->walk_of[c->blob_cur]);
	}

	REQ(pwn_get_stats(c, &s1) == PWN_OK && pwn_launch_order_waits(c, &w1) == PWN_OK);
	REQ(w0 == w1);          // (frames were traced in between; that the builds themselves count nowhere: below)
	(void)s0; (void)s1;
	{
		pwn_stats a, b;
		REQ(pwn_get_stats(c, &a) == PWN_OK);
		REQ(pwn_upload_spheres_device(c, 14, s.data(), 4000, NULL) == PWN_OK && pwn_spheres_device_state(c, st) == PWN_OK);
		REQ(pwn_get_stats(c, &b) == PWN_OK && memcmp(&a, &b, sizeof(a)) == 0);
		REQ(pwn_launch_order_waits(c, &w1) == PWN_OK && w0 == w1);
	}
	pwn_destroy(bare);
	pwn_destroy(c);
	fakehip_call_hook = NULL;
	printf("builds %d, launches checked %d\nok\n", g_builds, g_checked);
	return 0;
}
