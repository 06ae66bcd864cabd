// The sphere tables' device-memory form (tables.h PWN_LF_GLOBAL) as pwn_i_pack_blob lays it out, read the way the kernels read it -- on the
// CPU, under AddressSanitizer + UBSan, against the fake HIP runtime (README.txt).  A hook in the stand-in trace launch is handed
// every launch's pwn_trace_params.  For tables in the global form it walks every cell as trace_walk.inc does -- cell word, ordinal,
// liststart, records up to the end mark, the read-ahead behind the last one, which[], the sphere -- and holds each step to the
// context's own bins and object table; for all tables that the launch's LDS is the blob plus the kernel's 16 bytes.  The driver
// sends tables through that grow, shrink, change form, are refused, and change under frames in flight.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stddef.h>
#include <vector>
#include "pwn_internal.h"

extern "C" { extern void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes); }
static pwn_ctx *g_ctx;
static int g_checked_global, g_checked_lds;
#define REQ(x) do { if(!(x)) { fprintf(stderr, "CHECK FAILED %s line %d\n", #x, __LINE__); abort(); } } while(0)
static void check_tables(const pwn_trace_params *P, int, size_t lds_bytes)
{
	std::vector<uint16_t> counts(4096);
	int n = pwn_get_bins(g_ctx, counts.data(), NULL, 0);
	std::vector<int32_t> idx((size_t)(n > 0 ? n : 1));
	REQ(pwn_get_bins(g_ctx, counts.data(), idx.data(), n) == n);
	int ns = pwn_get_objects(g_ctx, NULL, 0);
	std::vector<pwn_sphere> sp((size_t)(ns > 0 ? ns : 1));
	pwn_get_objects(g_ctx, sp.data(), ns);
	const unsigned char *blob = (const unsigned char *)P->blob;
	const uint32_t *ci = (const uint32_t *)(blob + PWN_T_CELLINFO);
	REQ(P->blob_bytes % 16 == 0 && lds_bytes == P->blob_bytes + 16);
	if(P->g_rec != NULL)
	{
		g_checked_global++;
		const uint32_t *liststart = (const uint32_t *)(blob + PWN_T_BINIDX);
		const uint32_t ncell_cap = (P->blob_bytes - PWN_T_BINIDX) / 4;
		REQ((const unsigned char *)P->g_which - (const unsigned char *)P->g_rec == (ptrdiff_t)(((size_t)n + 1) * 16));
		REQ((const unsigned char *)P->g_sph - (const unsigned char *)P->g_which == (ptrdiff_t)((((size_t)n * 4) + 15) & ~(size_t)15));
		int k = 0; uint32_t ord_seen = 0;
		for(int c = 0; c < 4096; c++)
		{
			const uint32_t cw = ci[(c >> 6) * 65 + (c & 63)];
			REQ(((cw & PWN_C_SPH) != 0) == (counts[c] != 0));
			if(!counts[c]) continue;
			const uint32_t ord = (cw >> 16) & 0x7fffu;
			REQ(ord == ord_seen && ord < ncell_cap); ord_seen++;
			uint32_t ri = liststart[ord];
			REQ(ri == (uint32_t)k);
			for(int j = 0; j < counts[c]; j++, ri++, k++)
			{
				REQ(ri + 1u <= (uint32_t)n);                 // the read-ahead record exists
				const float *r = P->g_rec + 4 * (size_t)ri;
				uint32_t wb; memcpy(&wb, &r[3], 4);
				REQ(((wb >> 31) != 0) == (j == counts[c] - 1));
				const uint32_t which = P->g_which[ri];
				REQ(which == (uint32_t)idx[k] && which < (uint32_t)ns);
				const float *s = P->g_sph + 8 * (size_t)which;
				const pwn_sphere &q = sp[which];
				float r2 = q.r * q.r; uint32_t rb; memcpy(&rb, &r2, 4);
				REQ(r[0] == q.x && r[1] == q.y && r[2] == q.z && (wb & 0x7fffffffu) == rb);
				REQ(s[0] == q.x && s[1] == q.y && s[2] == q.z && s[3] == r2 && s[4] == q.refl && s[5] == q.cb && s[6] == q.cg && s[7] == q.cr);
			}
		}
		REQ(k == n);
		// row / column 64 never carry the sphere bit
		for(int i = 0; i <= 64; i++) { REQ(!(ci[64 * 65 + i] & PWN_C_SPH)); REQ(!(ci[i * 65 + 64] & PWN_C_SPH)); }
	}
	else g_checked_lds++;
}

static const char *LEVEL = "###########\r\n#;;;;;;;;;#\r\n#;;*;;;;;;#\r\n#;;;;$$;;;#\r\n#;a;;;;;b;#\r\n#;;;;;;;;;#\r\n###########\r\n";
#define CK(call) do { int rc_ = (call); if(rc_ < 0) { fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, ctx ? pwn_last_error(ctx) : ""); exit(1); } } while(0)
static unsigned rs = 12345; static float rnd() { rs = rs * 1664525u + 1013904223u; return (float)(rs >> 8) / 16777216.0f; }
static void make(std::vector<pwn_sphere> &s, int n, float rlo, float rhi, float span)
{
	s.clear();
	for(int i = 0; i < n; i++) { pwn_sphere q = { rlo + (rhi - rlo) * rnd(), rnd(), 1.0f + span * rnd(), rnd(), 1.0f + span * rnd(), rnd(), rnd(), rnd() }; s.push_back(q); }
}
int main()
{
	pwn_ctx *ctx = NULL;
	CK(pwn_init(&ctx, 0, 64, 48));
	g_ctx = ctx;
	pwn_fake_trace_hook = check_tables;
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_set_option(ctx, PWN_OPT_BLUR_PASSES, 0));
	std::vector<uint32_t> sb(64 * 48); std::vector<float> zb(64 * 48);
	float cam[16] = { 1,0,0,0, 0,1,0,0, 0,0,1,0, 3.5f,0.5f,2.5f,1 };
	std::vector<pwn_sphere> s;
	unsigned long long st[6];
	struct { int n; float rlo, rhi, span; int form; } cases[] = { {14, .1f, .3f, 8, 1}, {2100, .02f, .08f, 12, 2}, {14, .1f, .3f, 8, 1}, {10000, .02f, .2f, 62, 2},
		{800, 1.5f, 4.f, 62, 2}, {1500, .02f, .08f, 12, 2}, {10000, .02f, .2f, 62, 2}, {0, 0, 0, 0, 0}, {10000, 1.0f, 1.0f, 60, 2}, {4000, 0.1f, 0.1f, 0.0f, 2} };
	for(auto &c : cases)
	{
		make(s, c.n, c.rlo, c.rhi, c.span);
		CK(pwn_upload_spheres(ctx, s.data(), c.n));
		CK(pwn_sphere_tables_state(ctx, st));
		printf("n %d form %llu lds %llu dev %llu pairs %llu cells %llu longest %llu\n", c.n, st[0], st[1], st[2], st[3], st[4], st[5]);
		if((int)st[0] != c.form) { printf("unexpected form\n"); return 1; }
		CK(pwn_trace_screen_centred(ctx, cam, 0.0f, sb.data(), zb.data()));
	}
	// refused: previous stay
	make(s, 4096, 100.f, 100.f, 30);
	int rc = pwn_upload_spheres(ctx, s.data(), 4096);
	unsigned long long st2[6]; CK(pwn_sphere_tables_state(ctx, st2));
	printf("refused rc %d state same %d\n", rc, memcmp(st, st2, sizeof(st)) == 0);
	CK(pwn_trace_screen_centred(ctx, cam, 0.0f, sb.data(), zb.data()));
	// scheduler refill with big tables, and frames in flight
	CK(pwn_set_option(ctx, PWN_OPT_SCHEDULER, PWN_SCHED_REFILL));
	CK(pwn_trace_screen_centred(ctx, cam, 0.0f, sb.data(), zb.data()));
	CK(pwn_frames_config(ctx, 3, PWN_FRAME_SBUF, 1, 0));
	for(int f = 0; f < 12; f++)
	{
		pwn_frame fr;
		if(f >= 3) CK(pwn_wait_frame(ctx, f % 3, &fr));
		auto &c = cases[f % 8];
		make(s, c.n, c.rlo, c.rhi, c.span);
		CK(pwn_upload_spheres(ctx, s.data(), c.n));
		CK(pwn_submit_frame(ctx, cam, 0.0f, f % 3));
	}
	for(int f = 0; f < 3; f++) { pwn_frame fr; CK(pwn_wait_frame(ctx, f, &fr)); }
	pwn_destroy(ctx);
	printf("launches checked: %d with tables in device memory, %d with tables in LDS\n", g_checked_global, g_checked_lds);
	if(rc != PWN_ETOOBIG || memcmp(st, st2, sizeof(st)) != 0 || g_checked_global < 10 || g_checked_lds < 4) { printf("FAILED\n"); return 1; }
	printf("ok\n");
	return 0;
}
