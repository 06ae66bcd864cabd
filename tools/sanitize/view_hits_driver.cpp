// view_hits_driver.cpp -- the host side of pwn_trace_view_hits / pwn_trace_view_hits_device on the CPU, under AddressSanitizer + UBSan
// (README.txt 1d): pwn_calls.cpp and pwn_launch.cpp against the stand-in runtime and the stand-in trace launch, which writes every word of
// the planes it is handed and nothing else ("device" memory is malloc'ed: a plane that is too small, or a pointer that is off, is a report).
//     view_hits_asan LEVEL.txt        prints "ok"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pwn_internal.h"

extern "C" void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes);

#define REQ(x) do { if(!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while(0)
static const uint32_t POISON = 0x7fc12345u;
static int g_launches;
static pwn_trace_params g_last;
static void on_trace(const pwn_trace_params *P, int, size_t) { g_launches++; g_last = *P; }

static void camera(float *cam, int i)
{
	memset(cam, 0, 64);
	cam[0] = cam[5] = cam[10] = cam[15] = 1.0f;
	cam[12] = 5.5f + (float)i; cam[13] = 0.5f; cam[14] = 4.5f;
}

int main(int argc, char **argv)
{
	REQ(argc == 2);
	pwn_fake_trace_hook = on_trace;
	const int W = 40, H = 10, NMAX = 5;
	const size_t plane = (size_t)W * H;
	pwn_ctx *c = NULL, *bare = NULL, *wide = NULL;
	REQ(pwn_init(&c, 0, W, H) == PWN_OK);
	REQ(pwn_level_load(c, argv[1]) == PWN_OK);
	REQ(pwn_init(&bare, 0, W, H) == PWN_OK);                      // no level
	REQ(pwn_init(&wide, 0, 32768, 16) == PWN_OK);                 // 1024 views of it are more than 2^28 pixels
	REQ(pwn_level_load(wide, argv[1]) == PWN_OK);
	// (the blur stays on, and W is a multiple of 4 only by chance: the call never blurs)
	std::vector<float> cams(16 * 1024);
	for(int i = 0; i < 1024; i++) camera(&cams[16 * (size_t)i], i % 7);
	cams[3] = 0.25f;                                               // (view 0's camera has a w component: the batch runs the 4-lane variant)

	// ---- the host form: one view at a time, then batches that make the staging grow; planes left out
	std::vector<uint32_t> one[3];
	for(int k = 0; k < 3; k++) one[k].assign(NMAX * plane, POISON);
	for(int i = 0; i < NMAX; i++)
		REQ(pwn_trace_view_hits(c, 1, &cams[16 * (size_t)i], &one[0][i * plane], &one[1][i * plane], (float *)&one[2][i * plane]) == PWN_OK);
	for(int k = 0; k < 3; k++) for(size_t o = 0; o < NMAX * plane; o++) REQ(one[k][o] != POISON);
	for(size_t o = 0; o < NMAX * plane; o++) REQ(one[1][o] == (one[0][o] ^ 0x11111111u));
	REQ(g_last.has_w == 0 && g_last.hits != NULL && g_last.sbuf != NULL && g_last.zbuf != NULL && g_last.nviews == 1 && g_last.plane == plane);
	for(int n = 1; n <= NMAX; n++)
	{
		std::vector<uint32_t> got[3];
		for(int k = 0; k < 3; k++) got[k].assign(n * plane + 1, POISON);
		const int before = g_launches;
		REQ(pwn_trace_view_hits(c, n, cams.data(), got[0].data(), got[1].data(), (float *)got[2].data()) == PWN_OK);
		REQ(g_launches == before + 1 && g_last.nviews == n && g_last.has_w == 1);
		for(int k = 0; k < 3; k++) { REQ(memcmp(got[k].data(), one[k].data(), n * plane * 4) == 0); REQ(got[k][n * plane] == POISON); }
		pwn_stats st;
		REQ(pwn_get_stats(c, &st) == PWN_OK && st.blur_ms == 0.0f && st.total_ms >= st.trace_ms);
		// cell and / or dist left out: the others the same, the launch told so
		for(int mask = 0; mask < 3; mask++)
		{
			std::vector<uint32_t> a(n * plane, POISON), b(n * plane, POISON);
			REQ(pwn_trace_view_hits(c, n, cams.data(), a.data(), mask == 1 ? b.data() : NULL, mask == 2 ? (float *)b.data() : NULL) == PWN_OK);
			REQ((g_last.sbuf != NULL) == (mask == 1) && (g_last.zbuf != NULL) == (mask == 2));
			REQ(memcmp(a.data(), one[0].data(), n * plane * 4) == 0);
			if(mask != 0) REQ(memcmp(b.data(), one[mask].data(), n * plane * 4) == 0);
		}
	}
	REQ(c->hits_cap * 80 >= 12 * NMAX * plane && c->views_cap == 0 && c->d_vpre == NULL);       // (the view slots were not touched)

	// ---- the device form: "device" memory of exactly n x h x w words per plane, 16-byte aligned
	for(int n = 1; n <= NMAX; n += 2)
	{
		uint32_t *d[3];
		for(int k = 0; k < 3; k++) { REQ(posix_memalign((void **)&d[k], 16, n * plane * 4) == 0); for(size_t o = 0; o < n * plane; o++) d[k][o] = POISON; }
		float *dc;
		REQ(posix_memalign((void **)&dc, 16, (size_t)n * 64) == 0);
		memcpy(dc, cams.data(), (size_t)n * 64);
		const int before = g_launches;
		REQ(pwn_trace_view_hits_device(c, n, dc, PWN_VIEWS_HAS_W, d[0], d[1], d[2], c->stream) == PWN_OK);
		REQ(g_launches == before + 1 && g_last.has_w == 1);
		for(int k = 0; k < 3; k++) REQ(memcmp(d[k], one[k].data(), n * plane * 4) == 0);
		for(int k = 0; k < 3; k++) for(size_t o = 0; o < n * plane; o++) d[k][o] = POISON;
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0], NULL, d[2], NULL) == PWN_OK);
		REQ(g_last.has_w == 0 && g_last.sbuf == NULL);
		for(size_t o = 0; o < n * plane; o++) REQ(d[0][o] != POISON && d[1][o] == POISON && d[2][o] != POISON);
		// refusals of the device form: nothing is launched, nothing written
		for(int k = 0; k < 3; k++) for(size_t o = 0; o < n * plane; o++) d[k][o] = POISON;
		const int quiet = g_launches;
		REQ(pwn_trace_view_hits_device(NULL, n, dc, 0, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, NULL, 0, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, NULL, d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, 0, dc, 0, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, PWN_VIEWS_MAX + 1, dc, 0, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 2, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc + 1, 0, d[0], d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0] + 1, d[1], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0], d[1] + 2, d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0], d[1], (char *)d[2] + 8, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0], d[0], d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[0], d[1], d[1] + 4, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(c, n, dc, 0, d[2] + n * plane - 4, NULL, d[2], NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits_device(bare, n, dc, 0, d[0], d[1], d[2], NULL) == PWN_ENOLEVEL);
		REQ(pwn_trace_view_hits_device(wide, 1024, cams.data(), 0, d[0], NULL, NULL, NULL) == PWN_EINVAL);
		REQ(g_launches == quiet);
		for(int k = 0; k < 3; k++) for(size_t o = 0; o < n * plane; o++) REQ(d[k][o] == POISON);
		for(int k = 0; k < 3; k++) free(d[k]);
		free(dc);
	}

	// ---- refusals of the host form
	{
		std::vector<uint32_t> a(plane, POISON);
		const int quiet = g_launches;
		REQ(pwn_trace_view_hits(NULL, 1, cams.data(), a.data(), NULL, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits(c, 1, NULL, a.data(), NULL, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits(c, 1, cams.data(), NULL, a.data(), NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits(c, 0, cams.data(), a.data(), NULL, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits(c, PWN_VIEWS_MAX + 1, cams.data(), a.data(), NULL, NULL) == PWN_EINVAL);
		REQ(pwn_trace_view_hits(bare, 1, cams.data(), a.data(), NULL, NULL) == PWN_ENOLEVEL);
		REQ(pwn_trace_view_hits(wide, 1024, cams.data(), a.data(), NULL, NULL) == PWN_EINVAL);
		REQ(g_launches == quiet);
		for(size_t o = 0; o < plane; o++) REQ(a[o] == POISON);
	}
	pwn_destroy(c); pwn_destroy(bare); pwn_destroy(wide);
	printf("ok\n");
	return 0;
}
