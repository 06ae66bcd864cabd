// level_device_driver.cpp -- the host side of pwn_upload_level_device on the CPU, under AddressSanitizer + UBSan:
// pwn_level_device.cpp against the stand-in runtime and a stand-in for the bake's launch (fake_kernels.cpp) that runs level_bake.hip's
// algorithm sequentially over level_bake.h and reads and writes exactly what the kernel does ("device" memory is malloc'ed to the byte).
// What is looked at: every refusal launches nothing and changes nothing; a call is FIVE launches (one more in a context's first
// device build) and no host wait; the buffers the bake is handed; four calls go round the copies of the tables; the walk buffer
// chosen is never one another copy refers to; the tables a trace launch and the walk table a step read afterwards are the host's of the
// same level, byte for byte; a refused table leaves the level in force; pwn_upload_spheres_device keeps the device level; a host upload
// puts the host's level back with sd.base_ok cleared; the state words; no leak behind pwn_destroy.
//     level_device_asan        prints "ok"
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
extern void (*pwn_fake_players_hook)(const pwn_walk_table *walk, int n, int ticks, int stage);
extern void (*pwn_fake_level_bake_hook)(const void *d_data, const void *d_pmap, const void *d_base, const void *d_walk, const void *d_walk_prev, const void *d_status);
extern void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);
extern long fakehip_alloc_fail_in;
}
#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)

static std::map<const void *, size_t> g_alloc;
static int g_syncs;
static std::vector<std::pair<const void *, const void *>> g_waited;
static bool waited(const void *s, const void *e) { for(auto &w : g_waited) if(w.first == s && w.second == e) return true; return false; }
static void on_hip(const char *name, const void *a, const void *b, size_t bytes)
{
	if(strcmp(name, "hipStreamWaitEvent") == 0) g_waited.push_back({ a, b });
	if((strcmp(name, "hipMalloc") == 0 || strcmp(name, "hipHostMalloc") == 0) && a != NULL) g_alloc[a] = bytes;
	if(strcmp(name, "hipFree") == 0 || strcmp(name, "hipHostFree") == 0) g_alloc.erase(a);
	if(strcmp(name, "hipDeviceSynchronize") == 0 || strcmp(name, "hipStreamSynchronize") == 0 || strcmp(name, "hipEventSynchronize") == 0) g_syncs++;
}
static size_t room(const void *p) { auto it = g_alloc.find(p); return it == g_alloc.end() ? 0 : it->second; }

static int g_bakes, g_bins, g_uploads, g_other;
static size_t g_bins_n, g_bins_mp;
static void on_launch(const char *name, const void *, const void *, int ns, const size_t *sizes)
{
	if(strcmp(name, "level_bake") == 0) g_bakes++;
	else if(strcmp(name, "sphere_bins") == 0) { g_bins++; REQ(ns == 4); g_bins_n = sizes[0]; g_bins_mp = sizes[1]; }
	else if(strcmp(name, "upload") == 0) g_uploads++;
	else g_other++;
}
static pwn_ctx *g_ctx;
static const void *g_walk, *g_walk_prev;
static void on_bake(const void *d_data, const void *d_pmap, const void *d_base, const void *d_walk, const void *d_walk_prev, const void *d_status)
{
	(void)d_data; (void)d_pmap;
	REQ(d_base == g_ctx->sd.d_base && room(d_base) == PWN_T_BINIDX && room(d_status) == PWN_LD_STATUS_WORDS * 4u);
	REQ(room(d_walk) == sizeof(pwn_walk_table) && room(d_walk_prev) == sizeof(pwn_walk_table) && d_walk != d_walk_prev);
	// the buffer chosen: none that another copy of the tables refers to
	const int nb = (g_ctx->blob_cur + 1) % PWN_NBLOB;
	for(int i = 0; i < PWN_NBLOB; i++) if(i != nb) REQ(g_ctx->d_walk[g_ctx->walk_of[i]] != d_walk);
	REQ(d_walk_prev == g_ctx->d_walk[g_ctx->walk_of[g_ctx->blob_cur]]);
	g_walk = d_walk; g_walk_prev = d_walk_prev;
}

// what the next trace launch and the next step are to find: the level of context `ruler`, no sphere
static pwn_ctx *g_ruler;
static int g_checked, g_walks;
static const void *g_last_blob;
static void check_tables(const pwn_trace_params *P, int, size_t)
{
	g_checked++;
	g_last_blob = P->blob;
	const uint8_t *blob = (const uint8_t *)P->blob;
	REQ(memcmp(blob + PWN_T_RCP, g_ruler->tabs, 8192) == 0);
	REQ(memcmp(blob + PWN_T_CELLINFO, g_ruler->cell_base, sizeof(g_ruler->cell_base)) == 0);          // (no sphere bits: the words are the level's)
	REQ(memcmp(blob + PWN_T_EPREC, g_ruler->ep_recs, sizeof(g_ruler->ep_recs)) == 0);
	if(g_ctx->sd.in_force) REQ(P->g_rec != NULL && P->blob_bytes == pwn_t_total_glb(0u) && P->nbounds == 0);
}
static void check_walk(const pwn_walk_table *w, int, int, int)
{
	g_walks++;
	REQ(memcmp(w->cells, g_ruler->cells, 4096) == 0 && memcmp(w->pmap, g_ruler->pmap, sizeof(g_ruler->pmap)) == 0 && w->pad_[0] == 0 && w->pad_[1] == 0);
}

static const char *LEVEL_A = "###########\r\n#;;;;;;;;;#\r\n#;;*;;;;;;#\r\n#;;;;$$;;;#\r\n#;a;;;;;b;#\r\n#;;;;;;;;;#\r\n###########\r\n";
static const char *LEVEL_B = "#########\r\n#;;C;;;;#\r\n#;;*;$;;#\r\n#;;;;;C;#\r\n#D;;;;D;#\r\n#########\r\n";
static const char *LEVEL_C = "######\r\n#;E;;#\r\n#;;*E#\r\n######\r\n";

struct level { uint8_t *cells; pwn_portal *pmap; };          // (to the byte, 16-byte aligned: a read beside them is a report)
static level level_of(pwn_ctx *c)
{
	level l = { (uint8_t *)aligned_alloc(16, 4096), (pwn_portal *)aligned_alloc(16, 736) };
	REQ(pwn_get_level(c, l.cells, l.pmap, NULL) == PWN_OK);
	return l;
}
static void load(pwn_ctx *c, const char *text) { REQ(pwn_level_load_mem(c, text, (int)strlen(text)) == PWN_OK); }

int main()
{
	fakehip_call_hook = on_hip;
	pwn_fake_launch_hook = on_launch;
	pwn_fake_level_bake_hook = on_bake;
	pwn_fake_trace_hook = check_tables;
	pwn_fake_players_hook = check_walk;
	pwn_ctx *c = NULL, *ra = NULL, *rb = NULL, *rc = NULL, *bare = NULL;
	REQ(pwn_init(&c, 0, 64, 48) == PWN_OK && pwn_init(&ra, 0, 64, 48) == PWN_OK && pwn_init(&rb, 0, 64, 48) == PWN_OK && pwn_init(&rc, 0, 64, 48) == PWN_OK && pwn_init(&bare, 0, 64, 48) == PWN_OK);
	g_ctx = c;
	load(c, LEVEL_A); load(ra, LEVEL_A); load(rb, LEVEL_B); load(rc, LEVEL_C);
	REQ(pwn_set_option(c, PWN_OPT_BLUR_PASSES, 0) == PWN_OK);
	const level A = level_of(ra), B = level_of(rb), Cl = level_of(rc);
	std::vector<uint32_t> sb(64 * 48); std::vector<float> zb(64 * 48);
	const float cam[16] = { 1,0,0,0, 0,1,0,0, 0,0,1,0, 3.5f,0.5f,2.5f,1 };
	std::vector<float> cams(16, 0.0f), grav(4, 0.0f); uint8_t key = 0;
	cams[0] = cams[5] = cams[10] = cams[15] = 1.0f; cams[12] = 3.5f; cams[14] = 2.5f;
	unsigned long long st[8];
	REQ(pwn_level_device_state(c, st) == PWN_OK);
	for(int i = 0; i < 8; i++) REQ(st[i] == 0);
	REQ(pwn_get_level_device(c, A.cells, A.pmap) == PWN_EINVAL);
	auto frame = [&](pwn_ctx *ruler) { g_ruler = ruler; const int k = g_checked; REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK && g_checked > k); };
	auto step = [&](pwn_ctx *ruler, hipStream_t s) { g_ruler = ruler; const int k = g_walks; REQ(pwn_players_step_device(c, 1, &key, 0.01f, 1, cams.data(), grav.data(), NULL, s) == PWN_OK && g_walks == k + 1); };
	frame(ra); step(ra, c->stream);

	// ---- refusals: nothing launched, nothing changed
	{
		const int b0 = g_bakes, n0 = g_bins, u0 = g_uploads, o0 = g_other, cur0 = c->blob_cur;
		const std::map<const void *, size_t> before(g_alloc);
		g_waited.clear();
		REQ(pwn_upload_level_device(NULL, B.cells, B.pmap, NULL) == PWN_EINVAL);
		REQ(pwn_upload_level_device(c, NULL, B.pmap, NULL) == PWN_EINVAL);
		REQ(pwn_upload_level_device(c, NULL, NULL, NULL) == PWN_EINVAL);
		REQ(pwn_upload_level_device(c, B.cells + 4, B.pmap, NULL) == PWN_EINVAL);
		REQ(pwn_upload_level_device(c, B.cells, (const char *)B.pmap + 8, NULL) == PWN_EINVAL);
		REQ(pwn_upload_level_device(bare, B.cells, B.pmap, NULL) == PWN_ENOLEVEL && pwn_upload_level_device(bare, B.cells, NULL, NULL) == PWN_ENOLEVEL);
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		REQ(pwn_upload_level_device(c, B.cells, B.pmap, NULL) == PWN_EBUSY);
		REQ(pwn_level_device_state(c, st) == PWN_EBUSY && pwn_get_level_device(c, A.cells, A.pmap) == PWN_EBUSY);
		c->tiled = NULL;
		REQ(pwn_level_device_state(NULL, st) == PWN_EINVAL && pwn_level_device_state(c, NULL) == PWN_EINVAL && pwn_get_level_device(NULL, NULL, NULL) == PWN_EINVAL);
		{
			const int devs[2] = { 0, 0 };
			pwn_ctx *g = NULL;
			REQ(pwn_init_multi(&g, devs, 2, 64, 48) == PWN_OK);
			const int b1 = g_bakes;
			REQ(pwn_upload_level_device(g, B.cells, B.pmap, NULL) == PWN_ENOTSUP && pwn_level_device_state(g, st) == PWN_ENOTSUP && pwn_get_level_device(g, NULL, NULL) == PWN_ENOTSUP);
			REQ(g_bakes == b1);
			pwn_destroy(g);
		}
		// a buffer that cannot be had: refused, the tables as they were
		fakehip_alloc_fail_in = 1;
		REQ(pwn_upload_level_device(c, B.cells, B.pmap, NULL) == PWN_ENOMEM);
		fakehip_alloc_fail_in = 0;
		REQ(g_bakes == b0 && g_bins == n0 && g_uploads == u0 && g_other == o0 && c->blob_cur == cur0 && g_alloc == before && g_waited.empty());
		REQ(!c->sd.in_force && !c->ld.in_force);
		frame(ra); step(ra, c->stream);
	}

	// ---- a call: six launches in the context's first device build, five from then on; no host wait; the copies go round
	const void *blobs[8];
	{
		const level *lv[8] = { &B, &Cl, &A, &B, &Cl, &A, &B, &Cl };
		pwn_ctx *rl[8] = { rb, rc, ra, rb, rc, ra, rb, rc };
		for(int i = 0; i < 8; i++)
		{
			const int b0 = g_bakes, n0 = g_bins, u0 = g_uploads, o0 = g_other, sy0 = g_syncs;
			const int nb = (c->blob_cur + 1) % PWN_NBLOB;
			const bool in_use = c->tables_in_use[nb], walk = c->walk_in_use[nb];
			const hipEvent_t ev_t = c->tables_wait[nb], ev_w = c->ev_walk[nb];
			hipStream_t s = i & 1 ? c->stream2 : c->stream;
			g_waited.clear();
			// (odd calls derive the table: LEVEL_B / _C / _A have upper-case letters only where the grid is stored, so the derived table is the parser's)
			REQ(pwn_upload_level_device(c, lv[i]->cells, (i & 1) && rl[i] != ra ? NULL : lv[i]->pmap, s) == PWN_OK);
			REQ(g_bins_n == 0 && g_bins_mp == 0);          // (the sphere-less build)
			REQ(g_bakes == b0 + 1 && g_bins == n0 + 1 && g_uploads == u0 + (i == 0 ? 1 : 0) && g_other == o0 && g_syncs == sy0);
			REQ(c->blob_cur == nb && c->d_walk[c->walk_of[nb]] == g_walk && c->sd.in_force && c->ld.in_force && c->sd.base_ok);
			REQ(c->upload_pending[nb]);          // (what puts the launches and steps made from now on behind the build)
			if(in_use) REQ(waited(s, ev_t));
			if(walk) REQ(waited(s, ev_w) && !c->walk_in_use[nb]);
			REQ(waited(s, c->ld.ev_order) && waited(c->up_stream, c->ev_upload[nb]));
			if(i > 0) REQ(waited(s, c->sd.ev_build));          // (the build before went out on the other stream)
			frame(rl[i]); step(rl[i], c->stream);
			blobs[i] = g_last_blob;
			REQ(g_last_blob == c->d_blob[nb]);
			REQ(pwn_level_device_state(c, st) == PWN_OK);
			REQ(st[0] == 1 && st[1] == (unsigned long long)(i + 1) && st[2] == 0 && st[3] == 26 && st[6] == (unsigned long long)((i & 1) && rl[i] != ra ? 1 : 0) && st[7] == 0);
			int nrec = 0, paired = 0;
			for(int k = 0; k < (int)PWN_EP_MAX; k++) nrec += rl[i]->ep_recs[k] != 0;
			for(int k = 0; k < 26; k++) paired += rl[i]->pmap[k].x1 != -1 && rl[i]->pmap[k].x2 != -1;
			REQ(st[4] == (unsigned long long)nrec && st[5] == (unsigned long long)paired);
			// the host's queries go on describing the host's level
			uint8_t hc[4096]; pwn_portal hp[26];
			REQ(pwn_get_level(c, hc, hp, NULL) == PWN_OK && memcmp(hc, A.cells, 4096) == 0 && memcmp(hp, A.pmap, sizeof(hp)) == 0);
			REQ(pwn_get_level_device(c, hc, hp) == PWN_OK && memcmp(hc, lv[i]->cells, 4096) == 0 && memcmp(hp, lv[i]->pmap, sizeof(hp)) == 0);
		}
		for(int i = 4; i < 8; i++) REQ(blobs[i] == blobs[i - 4]);
		for(int i = 1; i < 4; i++) for(int j = 0; j < i; j++) REQ(blobs[i] != blobs[j]);
	}

	// ---- a refused table leaves the level in force (here: a device-built LEVEL_C), without spheres; a taken one afterwards works
	{
		pwn_portal *bad = (pwn_portal *)aligned_alloc(16, 736);
		memcpy(bad, B.pmap, 728);
		bad[7].x1 = 64;
		REQ(pwn_upload_level_device(c, B.cells, bad, NULL) == PWN_OK);
		frame(rc); step(rc, c->stream2);
		REQ(pwn_level_device_state(c, st) == PWN_OK && st[0] == 1 && st[1] == 9 && st[2] == 1 && st[3] == 7 && st[4] == 0 && st[6] == 0);
		bad[7].x1 = -1; bad[2].x1 = 0x7fffffff; bad[1].z2 = (int32_t)0x80000000u;
		REQ(pwn_upload_level_device(c, B.cells, bad, c->stream2) == PWN_OK);
		frame(rc); step(rc, c->stream);
		REQ(pwn_level_device_state(c, st) == PWN_OK && st[0] == 1 && st[2] == 1 && st[3] == 1);
		uint8_t hc[4096]; pwn_portal hp[26];
		REQ(pwn_get_level_device(c, hc, hp) == PWN_OK && memcmp(hc, Cl.cells, 4096) == 0 && memcmp(hp, Cl.pmap, sizeof(hp)) == 0);
		REQ(pwn_upload_level_device(c, B.cells, B.pmap, NULL) == PWN_OK);
		frame(rb); step(rb, c->stream);
		free(bad);
	}

	// ---- pwn_upload_spheres_device keeps the device level (its base copy and its walk table) and sends nothing from the host
	{
		const int u0 = g_uploads;
		pwn_fake_trace_hook = NULL;          // (cell words with sphere bits: spheres_device_driver.cpp looks at those)
		std::vector<pwn_sphere> s(3);
		for(int i = 0; i < 3; i++) { pwn_sphere q = { .2f, 0, 2.5f + i, .5f, 2.5f, 1, 1, 1 }; s[i] = q; }
		REQ(pwn_upload_spheres_device(c, 3, s.data(), 64, c->stream) == PWN_OK);
		REQ(pwn_trace_screen_centred(c, cam, 0.0f, sb.data(), zb.data()) == PWN_OK);
		step(rb, c->stream);
		REQ(g_uploads == u0 && c->ld.in_force && c->sd.in_force);
		REQ(pwn_level_device_state(c, st) == PWN_OK && st[0] == 1);
		REQ(pwn_upload_spheres_device(c, 0, NULL, 0, c->stream) == PWN_OK);
		pwn_fake_trace_hook = check_tables;
		frame(rb);
		REQ(g_uploads == u0);
	}

	// ---- a host upload puts the HOST's level back: sd.base_ok cleared, the walk table sent again; the next device build of spheres
	// brings the host's base copy first
	{
		const int u0 = g_uploads;
		REQ(pwn_upload_spheres(c, NULL, 0) == PWN_OK);
		REQ(!c->sd.in_force && !c->ld.in_force && !c->sd.base_ok && !c->walk_dirty && g_uploads == u0 + 2);
		frame(ra); step(ra, c->stream);
		REQ(pwn_level_device_state(c, st) == PWN_OK && st[0] == 0 && st[1] == 11);
		uint8_t hc[4096]; pwn_portal hp[26];
		REQ(pwn_get_level_device(c, hc, hp) == PWN_EINVAL);
		const int u1 = g_uploads;
		REQ(pwn_upload_spheres_device(c, 0, NULL, 0, c->stream) == PWN_OK && g_uploads == u1 + 1 && c->sd.base_ok);
		frame(ra); step(ra, c->stream);
		// a refused table over the host's level: still the host's level, and no device-built one in force
		pwn_portal *bad = (pwn_portal *)aligned_alloc(16, 736);
		memcpy(bad, B.pmap, 728);
		bad[0].z1 = -2;
		REQ(pwn_upload_level_device(c, B.cells, bad, NULL) == PWN_OK);
		frame(ra); step(ra, c->stream);
		REQ(pwn_level_device_state(c, st) == PWN_OK && st[0] == 0 && st[2] == 1 && st[3] == 0);
		REQ(pwn_get_level_device(c, hc, hp) == PWN_EINVAL);
		free(bad);
		// every host call that builds tables
		REQ(pwn_upload_level_device(c, B.cells, NULL, NULL) == PWN_OK); frame(rb);
		REQ(pwn_prepare_render(c) == PWN_OK && !c->ld.in_force); frame(ra); step(ra, c->stream);
		REQ(pwn_upload_level_device(c, B.cells, NULL, NULL) == PWN_OK); frame(rb);
		REQ(pwn_upload_level(c, Cl.cells, Cl.pmap) == PWN_OK && !c->ld.in_force); frame(rc); step(rc, c->stream);
		REQ(pwn_upload_level_device(c, B.cells, NULL, NULL) == PWN_OK); frame(rb); step(rb, c->stream);
		load(c, LEVEL_A); REQ(!c->ld.in_force); frame(ra); step(ra, c->stream);
		// a scheduler change repacks nothing while the device's tables are in force
		REQ(pwn_upload_level_device(c, Cl.cells, Cl.pmap, NULL) == PWN_OK);
		const int u2 = g_uploads;
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL) == PWN_OK); frame(rc);
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, PWN_SCHED_UNITS) == PWN_OK); frame(rc);
		REQ(g_uploads == u2 && c->ld.in_force);
	}

	// ---- left alone: pwn_stats and the launch rotation
	{
		pwn_stats a, b; unsigned long long w0 = 0, w1 = 0;
		REQ(pwn_get_stats(c, &a) == PWN_OK && pwn_launch_order_waits(c, &w0) == PWN_OK);
		REQ(pwn_upload_level_device(c, B.cells, B.pmap, c->stream2) == PWN_OK && pwn_level_device_state(c, st) == PWN_OK);
		REQ(pwn_get_stats(c, &b) == PWN_OK && memcmp(&a, &b, sizeof(a)) == 0 && pwn_launch_order_waits(c, &w1) == PWN_OK && w0 == w1);
	}
	free(A.cells); free(A.pmap); free(B.cells); free(B.pmap); free(Cl.cells); free(Cl.pmap);
	pwn_destroy(bare); pwn_destroy(ra); pwn_destroy(rb); pwn_destroy(rc);
	pwn_destroy(c);
	fakehip_call_hook = NULL;
	printf("bakes %d, launches checked %d, steps checked %d\nok\n", g_bakes, g_checked, g_walks);
	return 0;
}
