// players_driver.cpp -- the host side of pwn_players_step / pwn_players_step_device on the CPU, under AddressSanitizer + UBSan:
// pwn_players.cpp and pwn_tables.cpp against the stand-in runtime and a stand-in step (fake_kernels.cpp), which moves every player by a
// number made of its key byte, the ticks and the walk table it was handed ("device" memory is malloc'ed: a staging that is too small
// or a pointer that is off is a report).  What is looked at: the host form's arrays there and back as its staging grows, the walk
// table every step is handed -- the level in force, through level uploads, more sphere uploads than there are copies of the tables
// and a repack -- the wait of an upload for the steps that read the copy it fills, and for the steps of a second stream, every refusal with nothing launched and nothing
// written, no leak behind pwn_destroy.
//     players_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_players_hook)(const pwn_walk_table *walk, int n, int ticks, int stage);
extern "C" void (*fakehip_call_hook)(const char *name, const void *a, const void *b, size_t bytes);

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)
static int g_launches, g_n, g_ticks;
static pwn_walk_table g_walk;
static void on_step(const pwn_walk_table *w, int n, int ticks, int) { g_launches++; g_walk = *w; g_n = n; g_ticks = ticks; }
static const void *g_watch_event; static int g_watch_hits;
static void on_call(const char *name, const void *, const void *b, size_t) { if(strcmp(name, "hipStreamWaitEvent") == 0 && b == g_watch_event) g_watch_hits++; }

// the walk table the last step was handed is the level pwn_get_level returns
static void walk_is_level(pwn_ctx *c)
{
	uint8_t data[4096]; pwn_portal pm[26]; int32_t spawn[2];
	REQ(pwn_get_level(c, data, pm, spawn) == PWN_OK);
	REQ(memcmp(g_walk.cells, data, 4096) == 0);
	REQ(sizeof(pm) == 26 * 7 * 4 && memcmp(g_walk.pmap, pm, sizeof(pm)) == 0);
}

static const char HAND[] = "......\r\n.A;;A.\r\n.;*;;.\r\n.B;;..\r\n";

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_players_hook = on_step;
	pwn_ctx *c = NULL, *bare = NULL;
	REQ(pwn_init(&c, 0, 32, 16) == PWN_OK);
	REQ(pwn_level_load(c, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, 32, 16) == PWN_OK);                    // no level
	const int NMAX = 5000;
	std::vector<uint8_t> keys(NMAX);
	std::vector<float> cams(16 * (size_t)NMAX), grav(4 * (size_t)NMAX);
	std::vector<int32_t> trav(NMAX);
	auto fill = [&]() {
		for(int i = 0; i < NMAX; i++)
		{
			keys[i] = (uint8_t)(i * 7 + 1); trav[i] = i;
			for(int k = 0; k < 16; k++) cams[16 * (size_t)i + k] = (float)(i + k) * 0.25f;
			for(int k = 0; k < 4; k++) grav[4 * (size_t)i + k] = (float)(i - k) * 0.5f;
		}
	};

	// ---- the host form: there and back, the staging growing (3 players by the upload kernel, 5000 by a copy), with and without counts
	const int ns[4] = { 3, 65, NMAX, 7 };
	for(int k = 0; k < 4; k++)
		for(int with_trav = 1; with_trav >= 0; with_trav--)
		{
			fill();
			const std::vector<float> c0(cams), g0(grav);
			const int n = ns[k], before = g_launches;
			REQ(pwn_players_step(c, n, keys.data(), 0.5f, 4, cams.data(), grav.data(), with_trav ? trav.data() : NULL) == PWN_OK);
			REQ(g_launches == before + 1 && g_n == n && g_ticks == 4);
			walk_is_level(c);
			for(int i = 0; i < NMAX; i++)
			{
				const bool in = i < n;
				for(int q = 0; q < 16; q++) if(q != 12 || !in) REQ(cams[16 * (size_t)i + q] == c0[16 * (size_t)i + q]);
				if(in) REQ(cams[16 * (size_t)i + 12] != c0[16 * (size_t)i + 12]);
				for(int q = 0; q < 4; q++) REQ(grav[4 * (size_t)i + q] == g0[4 * (size_t)i + q] - ((in && q == 1) ? 0.5f : 0.0f));
				REQ(trav[i] == i + ((in && with_trav) ? 4 : 0));
			}
		}
	REQ(c->players_cap >= (size_t)NMAX);
	pwn_stats st0, st1;
	REQ(pwn_get_stats(c, &st0) == PWN_OK);

	// ---- the walk table is the level in force: through sphere uploads (more than copies), another level, a repack
	std::vector<pwn_sphere> sph;
	for(int i = 0; i < 8; i++) sph.push_back({ 0.2f, 0.5f, 3.0f + (float)i, 0.5f, 4.5f, 1.0f, 0.5f, 0.25f });
	fill();
	for(int i = 0; i < 2 * PWN_NBLOB + 1; i++)
	{
		REQ(pwn_upload_spheres(c, sph.data(), 1 + i % 8) == PWN_OK);
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), trav.data(), c->stream) == PWN_OK);
		walk_is_level(c);
	}
	for(int round = 0; round < 3; round++)
	{
		REQ(pwn_level_load_mem(c, HAND, (int)strlen(HAND)) == PWN_OK);
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL, c->stream) == PWN_OK);
		walk_is_level(c);
		REQ(g_walk.cells[64 + 1] == 'A' && g_walk.pmap[0] == 1 && g_walk.pmap[2] == 4 && g_walk.pmap[7 + 2] == -1);
		REQ(pwn_prepare_render(c) == PWN_OK);
		REQ(pwn_set_option(c, PWN_OPT_SCHEDULER, round % 2 ? PWN_SCHED_UNITS : PWN_SCHED_REFILL) == PWN_OK);      // (the tables are packed again by the next launch)
		REQ(pwn_players_step(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL) == PWN_OK);
		walk_is_level(c);
		REQ(pwn_level_load(c, argv[1]) == PWN_OK);
		REQ(pwn_upload_spheres(c, sph.data(), 3) == PWN_OK);
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), trav.data(), NULL) == PWN_OK);
		walk_is_level(c);
		REQ(g_walk.cells[64 + 1] != 'A');
	}
	// every buffer is some copy's, and the current copy's holds the level
	for(int i = 0; i < PWN_NBLOB; i++) REQ(c->walk_of[i] >= 0 && c->walk_of[i] < PWN_NBLOB);
	// a step on another stream than the last that read the copy puts the upload stream behind the record it replaces; on the same stream nothing
	{
		const int cur = c->blob_cur;
		REQ(c->walk_in_use[cur] && c->walk_stream[cur] == NULL);
		g_watch_event = c->ev_walk[cur]; g_watch_hits = 0;
		fakehip_call_hook = on_call;
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL, NULL) == PWN_OK);
		REQ(g_watch_hits == 0);
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL, c->stream2) == PWN_OK);
		REQ(g_watch_hits == 1 && c->walk_stream[cur] == c->stream2);
		REQ(pwn_players_step_device(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL, c->stream2) == PWN_OK);
		REQ(g_watch_hits == 1);
		REQ(pwn_players_step(c, 4, keys.data(), 0.5f, 1, cams.data(), grav.data(), NULL) == PWN_OK);          // (the host form: the context's stream)
		REQ(g_watch_hits == 2 && c->walk_stream[cur] == c->stream);
		fakehip_call_hook = NULL;
	}
	// an upload into the copy a step read waits for that step, once
	{
		const int cur = c->blob_cur;
		REQ(c->walk_in_use[cur]);
		g_watch_event = c->ev_walk[cur]; g_watch_hits = 0;
		fakehip_call_hook = on_call;
		for(int i = 0; i < PWN_NBLOB; i++) REQ(pwn_upload_spheres(c, sph.data(), 2 + i) == PWN_OK);
		REQ(c->blob_cur == cur && g_watch_hits == 1 && !c->walk_in_use[cur]);
		for(int i = 0; i < PWN_NBLOB; i++) REQ(pwn_upload_spheres(c, sph.data(), 2 + i) == PWN_OK);
		REQ(g_watch_hits == 1);
		fakehip_call_hook = NULL;
	}
	REQ(pwn_get_stats(c, &st1) == PWN_OK && memcmp(&st0, &st1, sizeof(st0)) == 0);          // no counters, no timings

	// ---- refusals: nothing launched, nothing written
	fill();
	const std::vector<float> c0(cams), g0(grav);
	const std::vector<int32_t> t0(trav);
	const int before = g_launches;
	float *pc = cams.data(), *pg = grav.data(); int32_t *pt = trav.data(); const uint8_t *pk = keys.data();
	REQ(((uintptr_t)pc & 15u) == 0 && ((uintptr_t)pg & 15u) == 0);
	const int n = 70;
#define BOTH(code, N, K, TD, TK, C, G, T) do { REQ(pwn_players_step(ctx, N, K, TD, TK, C, G, T) == code); REQ(pwn_players_step_device(ctx, N, K, TD, TK, C, G, T, NULL) == code); } while(0)
	pwn_ctx *ctxs[3] = { NULL, c, bare };
	for(int k = 0; k < 3; k++)
	{
		pwn_ctx *ctx = ctxs[k];
		BOTH(PWN_EINVAL, -1, pk, 0.5f, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, PWN_PLAYERS_MAX + 1, pk, 0.5f, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, 0.5f, 0, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, 0.5f, PWN_TICKS_MAX + 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, NAN, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, INFINITY, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, -INFINITY, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, NULL, 0.5f, 1, pc, pg, pt);
		BOTH(PWN_EINVAL, n, pk, 0.5f, 1, NULL, pg, pt);
		BOTH(PWN_EINVAL, n, pk, 0.5f, 1, pc, NULL, pt);
		if(ctx == NULL) continue;
		REQ(pwn_players_step_device(ctx, n, pk, 0.5f, 1, pc + 1, pg, pt, NULL) == PWN_EINVAL);          // misaligned
		REQ(pwn_players_step_device(ctx, n, pk, 0.5f, 1, pc, pg + 2, pt, NULL) == PWN_EINVAL);
		REQ(pwn_players_step_device(ctx, n, pk, 0.5f, 1, pc, pg, (int32_t *)((char *)pt + 2), NULL) == PWN_EINVAL);
		REQ(pwn_players_step_device(ctx, n, pk, 0.5f, 1, pc, pc + 16 * (n - 1), pt, NULL) == PWN_EINVAL);      // ranges overlap
		REQ(pwn_players_step_device(ctx, n, pk, 0.5f, 1, pc, pg, (int32_t *)(pg + 4 * (n - 1)), NULL) == PWN_EINVAL);
		REQ(pwn_players_step_device(ctx, n, (const uint8_t *)pc + 64 * n - 1, 0.5f, 1, pc, pg, pt, NULL) == PWN_EINVAL);
	}
	{
		pwn_ctx *ctx = bare;
		BOTH(PWN_ENOLEVEL, n, pk, 0.5f, 1, pc, pg, pt);
		BOTH(PWN_ENOLEVEL, 0, NULL, 0.5f, 1, NULL, NULL, NULL);
		ctx = c;
		c->tiled = (pwn_tiled *)(uintptr_t)16;          // (never looked at by a call that is refused)
		BOTH(PWN_EBUSY, n, pk, 0.5f, 1, pc, pg, pt);
		c->tiled = NULL;
		BOTH(PWN_OK, 0, NULL, 0.5f, 1, NULL, NULL, NULL);
	}
	REQ(g_launches == before);
	REQ(cams == c0 && grav == g0 && trav == t0);

	pwn_destroy(bare);
	pwn_destroy(c);
	printf("ok\n");
	return 0;
}
