/* Random and hostile rectangle lists through pwn_viewports_plan (pwnfps_amd/csrc/viewports_host.c) under ASan + UBSan:
 *   make -C tools/sanitize viewports OUT=/tmp/pwn_sanitize && /tmp/pwn_sanitize/fuzz_viewports
 * Small frames are checked against a painted grid (which rectangle is the first to leave the frame, to be empty, to break the
 * blur's alignment or to touch a painted pixel), hostile ones (negative values, INT32_MAX, n at its limits, NULL) for the
 * answer PWN_EINVAL and for what the sanitizers say about the arithmetic on the way. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "pwnhip.h"

static int32_t hostile(void)
{
	static const int32_t v[] = { INT32_MAX, INT32_MIN, INT32_MAX - 1, INT32_MIN + 1, -1, 0, 1, 32768, 32769, 65536, -32768, 1 << 30, -(1 << 30), 3, 4, 16 };
	return v[rand() % (int)(sizeof(v) / sizeof(v[0]))];
}

int main(void)
{
	srand(20261018);
	static pwn_viewport vp[PWN_VIEWS_MAX + 2];
	static unsigned char paint[64 * 64];
	unsigned long long out[4];
	/* 1. small frames against the painted grid */
	for(int it = 0; it < 40000; it++)
	{
		const int W = 1 + rand() % 64, H = 1 + rand() % 64, blur = rand() % 3, n = 1 + rand() % 6;
		memset(paint, 0, sizeof(paint));
		int bad = n;
		unsigned long long units = 0, pixels = 0, largest = 0;
		const int frame_ok = !(blur > 0 && (W & 3) != 0);
		for(int i = 0; i < n; i++)
		{
			pwn_viewport r;
			r.x = rand() % (W + 2) - 1; r.y = rand() % (H + 2) - 1;
			r.w = rand() % (W / 2 + 3) - 1; r.h = rand() % (H / 2 + 3) - 1;
			if(blur > 0 && rand() % 4 != 0) { r.x &= ~3; r.w &= ~3; }
			vp[i] = r;
			int ok = r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && r.x + r.w <= W && r.y + r.h <= H;
			if(ok && frame_ok)
			{
				const unsigned long long u = (unsigned long long)((r.w + 15) / 16) * (unsigned long long)((r.h + 3) / 4);
				units += u; pixels += (unsigned long long)r.w * (unsigned long long)r.h;
				if(u > largest) largest = u;
			}
			if(bad != n) continue;
			if(ok && blur > 0 && ((r.x & 3) || (r.w & 3))) ok = 0;
			if(ok)
				for(int y = r.y; y < r.y + r.h; y++)
					for(int x = r.x; x < r.x + r.w; x++)
						if(paint[y * 64 + x]++) ok = 0;
			if(!ok) bad = i;
		}
		const int rc = pwn_viewports_plan(W, H, blur, n, vp, out);
		const int want = frame_ok && bad == n ? PWN_OK : PWN_EINVAL;
		if(rc != want || out[3] != (unsigned long long)bad || out[0] != units || out[1] != pixels || out[2] != largest)
		{
			printf("case %d: W %d H %d blur %d n %d: rc %d (want %d), out %llu %llu %llu %llu (want %llu %llu %llu %d)\n", it, W, H, blur, n,
				rc, want, out[0], out[1], out[2], out[3], units, pixels, largest, bad);
			return 1;
		}
	}
	/* 2. hostile values: never PWN_OK unless every rectangle really lies inside the frame, never a sanitizer report */
	for(int it = 0; it < 40000; it++)
	{
		const int W = rand() % 3 ? hostile() : 1 + rand() % 32768, H = rand() % 3 ? hostile() : 1 + rand() % 32768;
		static const int ns[] = { 0, -1, 1, 2, 7, PWN_VIEWS_MAX - 1, PWN_VIEWS_MAX, PWN_VIEWS_MAX + 1, INT_MAX, INT_MIN };
		const int n = ns[rand() % 10], blur = rand() % 4 - 1;
		const int have = n < 0 ? 0 : n > PWN_VIEWS_MAX + 1 ? PWN_VIEWS_MAX + 1 : n;
		for(int i = 0; i < have; i++)
		{
			vp[i].x = rand() % 2 ? hostile() : rand() % 100; vp[i].y = rand() % 2 ? hostile() : rand() % 100;
			vp[i].w = rand() % 2 ? hostile() : rand() % 100; vp[i].h = rand() % 2 ? hostile() : rand() % 100;
		}
		const int rc = pwn_viewports_plan(W, H, blur, n, rand() % 50 ? vp : NULL, out);
		if(rc != PWN_OK && rc != PWN_EINVAL) return 2;
		if(rc == PWN_OK)
		{
			if(n < 1 || n > PWN_VIEWS_MAX || W < 1 || H < 1 || W > 32768 || H > 32768 || out[3] != (unsigned long long)n) return 3;
			unsigned long long px = 0;
			for(int i = 0; i < n; i++)
			{
				if(vp[i].w < 1 || vp[i].h < 1 || vp[i].x < 0 || vp[i].y < 0 || (long long)vp[i].x + vp[i].w > W || (long long)vp[i].y + vp[i].h > H) return 4;
				px += (unsigned long long)vp[i].w * (unsigned long long)vp[i].h;
			}
			if(px != out[1] || px > (unsigned long long)W * (unsigned long long)H) return 5;
		}
		else if(out[3] > (unsigned long long)(n > 0 ? n : 0)) return 6;
	}
	/* 3. PWN_VIEWS_MAX rectangles: a full grid is accepted, one more rectangle or one shifted by a pixel is not */
	{
		for(int i = 0; i < PWN_VIEWS_MAX; i++) { vp[i].x = (i % 32) * 8; vp[i].y = (i / 32) * 4; vp[i].w = 8; vp[i].h = 4; }
		if(pwn_viewports_plan(256, 128, 2, PWN_VIEWS_MAX, vp, out) != PWN_OK || out[0] != PWN_VIEWS_MAX || out[1] != 256 * 128 || out[2] != 1 || out[3] != PWN_VIEWS_MAX) return 7;
		vp[PWN_VIEWS_MAX - 1].y -= 1;
		if(pwn_viewports_plan(256, 128, 0, PWN_VIEWS_MAX, vp, out) != PWN_EINVAL || out[3] != PWN_VIEWS_MAX - 1) return 8;
		if(pwn_viewports_plan(256, 128, 0, PWN_VIEWS_MAX + 1, vp, out) != PWN_EINVAL) return 9;
		if(pwn_viewports_plan(256, 128, 0, 1, vp, NULL) != PWN_EINVAL) return 10;
	}
	puts("asan/ubsan fuzz of viewports_host.c: ok");
	return 0;
}
