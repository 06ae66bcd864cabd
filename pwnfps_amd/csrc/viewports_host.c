/* viewports_host.c -- the argument rules of pwn_trace_viewports that need no context (include/pwnhip.h: pwn_viewports_plan).
 * Plain C, no HIP, no allocation: pwn_trace_viewports calls this very function, and tools/sanitize/fuzz_viewports.c compiles
 * it stand-alone. */
#include <stddef.h>
#include <stdint.h>
#include "pwnhip.h"

/* Rectangles are judged in order; the first one that breaks a rule is the offender (for an overlap: the later of the two).
   All arithmetic on the caller's coordinates is 64-bit: x + w of two INT32_MAX does not wrap. */
int pwn_viewports_plan(int W, int H, int blur_passes, int n, const pwn_viewport *vp, unsigned long long out[4])
{
	if(out == NULL) return PWN_EINVAL;
	out[0] = out[1] = out[2] = 0ull;
	out[3] = n > 0 ? (unsigned long long)n : 0ull;
	if(vp == NULL || n < 1 || n > PWN_VIEWS_MAX) return PWN_EINVAL;
	/* (the frame itself: pwn_init's sizes; no rectangle is named) */
	const int frame_ok = W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && !(blur_passes > 0 && (W & 3) != 0);
	int bad = n;
	for(int i = 0; i < n; i++)
	{
		const int64_t x = vp[i].x, y = vp[i].y, w = vp[i].w, h = vp[i].h;
		int ok = w >= 1 && h >= 1 && x >= 0 && y >= 0 && x + w <= (int64_t)W && y + h <= (int64_t)H;
		if(ok && frame_ok)
		{
			/* what the launch would hold of this rectangle (inside a frame of at most 32768 x 32768: no overflow) */
			const unsigned long long u = (unsigned long long)((w + 15) / 16) * (unsigned long long)((h + 3) / 4);
			out[0] += u;
			out[1] += (unsigned long long)w * (unsigned long long)h;
			if(u > out[2]) out[2] = u;
		}
		if(bad != n) continue;
		/* blur on: 16-byte groups of a pitch-W plane (screen.h:88,117) */
		if(ok && blur_passes > 0 && ((x & 3) != 0 || (w & 3) != 0)) ok = 0;
		/* no pixel twice: against every rectangle before this one (those passed the rules above) */
		for(int j = 0; ok && j < i; j++)
		{
			const int64_t xj = vp[j].x, yj = vp[j].y, wj = vp[j].w, hj = vp[j].h;
			if(x < xj + wj && xj < x + w && y < yj + hj && yj < y + h) ok = 0;
		}
		if(!ok) bad = i;
	}
	out[3] = (unsigned long long)bad;
	return frame_ok && bad == n ? PWN_OK : PWN_EINVAL;
}
