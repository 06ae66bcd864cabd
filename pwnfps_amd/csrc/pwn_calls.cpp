// pwn_calls.cpp -- the calls that return with their result on the host, and their device forms: the blocking call
// (pwn_trace_screen_centred) in one piece and in row strips, host registration, the batches of views, viewports, rays and hits, the first-hit planes of views
// and of views of their own sizes.
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include "pwn_internal.h"
#include "launch_plan.h"

// ---- what the blocking call and the batch calls share (with the frames in flight: pwn_launch.cpp pwn_i_blur_passes_run) -----
// (tests/golden/host_calls.txt has, per entry point, what these send to the runtime and the launchers: tools/sanitize/calls_driver.cpp)

// The blocking calls (pwn_trace_screen_centred, pwn_trace_views) on compute stream s: behind the frames in flight, whichever
// compute stream their kernels are on
int pwn_i_wait_frames_in_flight(pwn_ctx *c, hipStream_t s)
{
	if(c->last_frame_done != NULL && c->last_frame_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->last_frame_done, 0));
	if(c->last_frame_done != NULL && c->stream2 != NULL && c->last_frame_stream != c->stream2) HIPCHK(c, hipStreamWaitEvent(c->stream2, c->last_frame_done, 0));      // (strips use both)
	c->last_frame_done = NULL;       // (the call ends with the stream empty)
	return PWN_OK;
}

// What refuses a batch call once its own arguments are in order (include/pwnhip.h), in the order that decides which code a caller
// with two faults gets.  views > 0: a call that traces that many views of w x h and blurs them, with the two rules of those
// (blurs = false: the first-hit planes of views, which are never blurred, with the first alone).
int pwn_i_batch_refuse(const pwn_ctx *c, int views, bool blurs)
{
	if(views > 0 && (size_t)views * (size_t)c->w * (size_t)c->h > ((size_t)1 << 28)) return PWN_EINVAL;
	if(views > 0 && blurs && c->blur_passes > 0 && (c->w & 3) != 0) return PWN_EINVAL;
	if(c->tiled != NULL) return PWN_EBUSY;
	if(!c->have_level) return PWN_ENOLEVEL;
	return PWN_OK;
}

// The end of a blocking call on stream s, in two steps: "kernels done" (ev[2]), `bytes` of colour and, where the caller wants it,
// of depth on their way down, "all done" (ev[3]) ...
static int blocking_copies(pwn_ctx *c, hipStream_t s, uint32_t *sbuf, const uint32_t *d_col, float *zbuf, const float *d_z, size_t bytes)
{
	HIPCHK(c, hipEventRecord(c->ev[2], s));
	HIPCHK(c, hipMemcpyAsync(sbuf, d_col, bytes, hipMemcpyDeviceToHost, s));
	if(zbuf != NULL) HIPCHK(c, hipMemcpyAsync(zbuf, d_z, bytes, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipEventRecord(c->ev[3], s));
	return PWN_OK;
}
// ... the call's times from its events: ev[0] start, [1] traced, [2] blurred (a call that does not blur records none), [3] all done
static void stats_from_events(pwn_ctx *c, bool blurred)
{
	(void)hipEventElapsedTime(&c->stats.trace_ms, c->ev[0], c->ev[1]);
	if(blurred) (void)hipEventElapsedTime(&c->stats.blur_ms, c->ev[1], c->ev[2]);
	else c->stats.blur_ms = 0.0f;
	(void)hipEventElapsedTime(&c->stats.total_ms, c->ev[0], c->ev[3]);
}
// ... and the wait for "all done" (what a call launches between the two steps it does not wait for)
static int blocking_wait(pwn_ctx *c, bool blurred)
{
	HIPCHK(c, hipEventSynchronize(c->ev[3]));
	stats_from_events(c, blurred);
	return PWN_OK;
}

// ---- the blocking call in row strips (PWN_OPT_CALL_STRIPS, include/pwnhip.h) ----
// One pwn_trace_screen_centred of a 4K frame is 0.32 ms of trace, 0.03 ms of blur and 0.64 ms of PCIe (33 MB at the
// link's 52 GB/s): one after the other the GPU idles for two thirds of the call.  In strips the copy starts when the
// first strips are blurred and runs beside the kernels of the rest: the call is the copy plus the first strips.
// Strips grow from the top -- the first ones small so that the copy starts early, each later one 1.2 times the one before.

// rows a blur tap of depth <= `depth` reaches (screen.h:100-102): 24 is the row tiling's halo; the strips of a blocking call begin with 8
// (level.txt from its spawn pose: taps reach 32 rows at 4K, depth 8 covers 36) and go to 24 after the first frame whose taps went further
static int blur_reach_rows(int h, double depth = 24.0) { return (int)(0.002 * h * depth) + 2; }

static int strip_cuts(const pwn_ctx *c, int want, int *cuts)
{
	const int h = c->h;
	int n = 0;
	cuts[0] = 0;
	if(want >= 2)
	{
		const int per = ((h + want - 1) / want + 31) & ~31;           // (the blur works in 32-row tiles)
		while(cuts[n] < h && n < PWN_CALL_STRIPS_MAX) { cuts[n + 1] = cuts[n] + per < h ? cuts[n] + per : h; n++; }
		cuts[n] = h;
		return n;
	}
	// (measured at 4K, profiles/r5/call_strips.txt: first strip 96 / 128 / 160 / 192 rows x growth 1.2 / 1.4 / 1.6 -- 128 x 1.2, eight
	// strips, was the fastest; 1.6 costs 10 %: the last chunk's copy starts when everything else is done.  With the round's final trace
	// kernel 160 rows, seven strips, is 0.5-0.8 % faster at 4K on one copy stream and on two, 128 against 96 rows 2.8 % at 1440p,
	// 320 against 256 equal at 8K: the first strip is 2/27 of the frame)
	double grow = 1.2;
	int rows = (h * 2 / 27 + 31) & ~31;
	if(const char *e = getenv("PWN_DBG_STRIP_FIRST")) if(atoi(e) >= 8) rows = (atoi(e) + 7) & ~7;        // (experiments)
	if(const char *e = getenv("PWN_DBG_STRIP_GROW")) if(atof(e) >= 1.0) grow = atof(e);
	while(cuts[n] < h)
	{
		int y = cuts[n] + rows;
		if(n == PWN_CALL_STRIPS_MAX - 1 || h - y < rows / 2) y = h;     // (a rest of less than half a strip goes with this one)
		cuts[++n] = y;
		rows = ((int)((double)rows * grow) + 31) & ~31;
	}
	return n;
}

// registered (pwn_host_register, hipHostRegister) or allocated pinned: a copy into it is DMA that does not hold the caller
static bool host_is_pinned(const void *p, size_t bytes)
{
	if(p == NULL) return true;
	const void *ends[2] = { p, (const char *)p + bytes - 1 };
	for(int i = 0; i < 2; i++)
	{
		hipPointerAttribute_t a;
		memset(&a, 0, sizeof(a));
		if(hipPointerGetAttributes(&a, ends[i]) != hipSuccess) { (void)hipGetLastError(); return false; }
		if(a.type != hipMemoryTypeHost) return false;
	}
	return true;
}

extern "C" int pwn_host_register(pwn_ctx *c, void *base, size_t bytes)
{
	if(GRP_HEAD(c)) return (base == NULL || bytes == 0) ? PWN_EINVAL : pwn_group_host_register(c, base, bytes);
	if(c == NULL || base == NULL || bytes == 0) return PWN_EINVAL;
	for(int i = 0; i < c->host_regs_n; i++) if(c->host_regs[i].base == base) return c->host_regs[i].bytes >= bytes ? PWN_OK : PWN_EINVAL;
	if(c->host_regs_n >= PWN_HOST_REGS_MAX) return PWN_EBUSY;
	(void)hipSetDevice(c->device);
	const hipError_t e = hipHostRegister(base, bytes, hipHostRegisterPortable);
	if(e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return PWN_OK; }       // (somebody else's registration: theirs to undo)
	if(e != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "hipHostRegister(%zu bytes): %s", bytes, hipGetErrorString(e)); return PWN_EHIP; }
	c->host_regs[c->host_regs_n].base = base; c->host_regs[c->host_regs_n].bytes = bytes; c->host_regs_n++;
	return PWN_OK;
}

extern "C" int pwn_host_unregister(pwn_ctx *c, void *base)
{
	if(GRP_HEAD(c)) return base == NULL ? PWN_EINVAL : pwn_group_host_unregister(c, base);
	if(c == NULL || base == NULL) return PWN_EINVAL;
	for(int i = 0; i < c->host_regs_n; i++)
		if(c->host_regs[i].base == base)
		{
			(void)hipSetDevice(c->device);
			// (a copy of an earlier call into it is complete: the blocking call returns behind its copies)
			const hipError_t e = hipHostUnregister(base);
			c->host_regs[i] = c->host_regs[--c->host_regs_n];
			if(e != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "hipHostUnregister: %s", hipGetErrorString(e)); return PWN_EHIP; }
			return PWN_OK;
		}
	return PWN_EINVAL;
}

extern "C" int pwn_call_strips_state(pwn_ctx *c, unsigned long long out[6])
{
	if(GRP_HEAD(c)) return pwn_call_strips_state(GRP_M0(c), out);
	if(c == NULL || out == NULL) return PWN_EINVAL;
	out[0] = (unsigned long long)(long long)c->call_strips; out[1] = (unsigned long long)c->strips_last; out[2] = c->strip_calls; out[3] = c->strip_redone;
	out[4] = (unsigned long long)c->strip_copy_streams; out[5] = c->strip_reach ? 24ull : 8ull;
	return PWN_OK;
}

static int call_in_strips(pwn_ctx *c, const float cam[16], float sec, uint32_t *sbuf, float *zbuf, const int *cuts, int K)
{
	// Chunks go to the host on ONE copy stream or on TWO in turn.  A DMA copy behind another on one stream starts ~11 us after that one
	// ended, and small copies run at 35-47 GB/s; on two streams the next copy's start-up hides behind the current one's bytes -- on
	// some boxes: 0.745-0.755 against 0.77-0.79 ms per 4K call on three of them, 0.805 against 0.773 on a fourth
	// (profiles/r5/call_strips.txt).  So a context finds out once: its first 8 calls in strips use one stream, the next 8 two, and the
	// faster (by the median of the calls' own wall times, the first of each eight left out) is kept.  PWN_CALL_COPY_STREAMS=1|2 in the
	// environment fixes it.
	if(c->copy_stream2 == NULL && hipStreamCreateWithFlags(&c->copy_stream2, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->copy_stream2 = NULL; }
	int ncopy = c->strip_copy_streams;
	if(ncopy == 0) ncopy = c->strip_calib_n < 8 ? 1 : 2;               // (finding out)
	if(c->copy_stream2 == NULL) ncopy = 1;
	hipStream_t cs = c->copy_stream, cpy[2] = { c->copy_stream, ncopy == 2 ? c->copy_stream2 : c->copy_stream };
	struct timespec t_call0;
	clock_gettime(CLOCK_MONOTONIC, &t_call0);
	// Successive strips' trace launches alternate between the context's two compute streams (the pattern the work-queue
	// counters are made for, include/pwnhip.h): strip k + 1's grid moves onto the CUs as strip k's waves run out of units.
	// On one stream every launch waits for the tail of the one before it: 8 strips of a 4K frame took 0.61 ms where the
	// whole frame takes 0.35 (two streams: 0.43).
	hipStream_t st[2] = { c->stream, (c->frame_overlap && c->stream2 != NULL) ? c->stream2 : c->stream };
	if(const char *e = getenv("PWN_DBG_STRIP_STREAMS")) if(atoi(e) == 1) st[1] = st[0];
	const bool two = st[1] != st[0];
	const size_t W = (size_t)c->w, n = W * (size_t)c->h;
	const bool blur = c->blur_passes == 1;
	for(; c->strip_ev_n < 2 * K; c->strip_ev_n++) HIPCHK(c, hipEventCreateWithFlags(&c->strip_ev[c->strip_ev_n], hipEventDisableTiming));
	if(c->d_strip_miss == NULL)
	{
		HIPCHK(c, hipMalloc((void **)&c->d_strip_miss, 64));
		HIPCHK(c, hipMemset(c->d_strip_miss, 0, 64));
		HIPCHK(c, hipHostMalloc((void **)&c->h_strip_miss, 64, hipHostMallocDefault));
		HIPCHK(c, hipDeviceSynchronize());
	}
	*c->h_strip_miss = 0u;
	uint32_t *pre = c->d_pre, *fin = blur ? c->d_out : c->d_pre;
	// The blur is cut apart from the trace: behind strip k's trace the rows [0, cuts[k + 1]) are there, and every row whose
	// taps of depth <= 8 (24 once a frame's taps went further) stay inside them is blurred and sent -- chunk k = rows [sent, cuts[k + 1] - H), the last one to the end.
	// So the first bytes leave behind the FIRST strip's trace, not the second's.
	int H = blur ? blur_reach_rows(c->h, c->strip_reach ? 24.0 : 8.0) : 0;
	if(const char *e = getenv("PWN_DBG_STRIP_REACH")) if(*e && blur) H = atoi(e);
	// A copy into memory the device does not know is staged by the runtime and holds this thread until it is through:
	// two strips of kernels are then enqueued ahead of every copy, so that the GPU has work while the host waits in it.
	// (Measured and dropped, profiles/r5/call_strips.txt: the blur storing its pixels into the registered buffer itself, and a
	// copy kernel per chunk in place of the DMA copy -- stores to host memory that come from the CUs back up into the trace
	// grids' own stores: the strips' traces of a 4K frame went from 0.43 to 0.9 ms.)
	const bool pinned = host_is_pinned(sbuf, n * 4) && host_is_pinned(zbuf, n * 4);
	int ahead = pinned ? 0 : 2;
	if(const char *e = getenv("PWN_DBG_STRIP_AHEAD")) if(*e) ahead = atoi(e);
	// (workgroups the grids leave free for the other stream's kernels: the blurs find a place at once.  One per CU was the best of
	// 0 / 128 / 256 / 512 / 768 when the plan was made; with the round's final kernels 384 is 2 % faster than 256 on two copy streams
	// (0.732 -> 0.716 ms per 4K call), 512 nearly so, and equal on one: tools/r5/strip_plan_ab.py, profiles/r5/call_strips.txt)
	int room = two ? c->num_cus + c->num_cus / 2 : 0;
	if(const char *e = getenv("PWN_DBG_STRIP_ROOM")) if(*e) room = atoi(e);
	int traced = 0, chunks = 0, copied = 0, rc;
	int chunk_y[PWN_CALL_STRIPS_MAX + 1];          // chunk j = rows [chunk_y[j], chunk_y[j + 1]), blurred behind the trace of strip chunk_k[j]
	chunk_y[0] = 0;
	// PWN_DBG_STRIP_TIMELINE: when every strip's trace, every chunk's blur and copy ended (experiments: timing events between the kernels cost a few us each)
	static hipEvent_t tl[4 * PWN_CALL_STRIPS_MAX];
	const bool timeline = getenv("PWN_DBG_STRIP_TIMELINE") != NULL;
	if(timeline && tl[0] == NULL) for(int i = 0; i < 4 * PWN_CALL_STRIPS_MAX; i++) HIPCHK(c, hipEventCreate(&tl[i]));
#define STRIPS_FAIL(code) do { (void)hipStreamSynchronize(st[0]); (void)hipStreamSynchronize(st[1]); (void)hipStreamSynchronize(cpy[0]); (void)hipStreamSynchronize(cpy[1]); return (code); } while(0)
	HIPCHK(c, hipEventRecord(c->ev[0], st[0]));
	while(traced < K || copied < chunks)
	{
		if(traced < K)
		{
			const int k = traced;
			hipStream_t ts = st[k & 1];
			pwn_trace_launch T = { .cam = cam, .sec = sec, .y0 = cuts[k], .y1 = cuts[k + 1], .d_sbuf = pre, .d_zbuf = c->d_z, .stream = ts,
				.clear_word = (k == 0 && blur) ? c->d_strip_miss : NULL,      // (cleared by the first strip's launch, in front of every blur)
				.tables_event = c->strip_ev[2 * k],                           // recorded right behind the launch; its previous record is a call that returned
				.room = room };
			rc = pwn_i_launch_trace(c, &T);
			if(rc != PWN_OK) { (void)hipEventRecord(c->strip_ev[2 * k], ts); STRIPS_FAIL(rc); }
			HIPCHK(c, hipEventRecord(c->strip_ev[2 * k], ts));
			if(timeline) HIPCHK(c, hipEventRecord(tl[4 * k], ts));
			traced++;
			if(traced == K) HIPCHK(c, hipEventRecord(c->ev[1], ts));
			// the chunk this trace completes, on its stream: behind it and -- one wait between the streams -- behind the newest
			// trace of the other stream (older ones are in front of those)
			int to = traced == K ? c->h : ((cuts[traced] - H) & ~31);
			if(to > chunk_y[chunks] || traced == K)
			{
				const int j = chunks, y0 = chunk_y[j];
				if(to < y0) to = y0;
				if(blur && to > y0)
				{
					if(two && k >= 1) HIPCHK(c, hipStreamWaitEvent(ts, c->strip_ev[2 * (k - 1)], 0));
					const bool whole = traced == K;
					const pwn_blur_launch B = { .y0 = y0, .y1 = to, .d_pre = pre, .d_z = c->d_z, .d_out = fin, .stream = ts,
						.avail_y1 = whole ? 0 : cuts[traced], .d_miss = whole ? NULL : c->d_strip_miss };
					rc = pwn_i_launch_blur(c, &B);
					if(rc != PWN_OK) STRIPS_FAIL(rc);
				}
				else if(!blur && two && k >= 1) HIPCHK(c, hipStreamWaitEvent(ts, c->strip_ev[2 * (k - 1)], 0));      // (the chunk's rows may be the other stream's)
				HIPCHK(c, hipEventRecord(c->strip_ev[2 * j + 1], ts));
				if(timeline) HIPCHK(c, hipEventRecord(tl[4 * j + 1], ts));
				chunk_y[j + 1] = to;
				chunks++;
				if(traced == K) HIPCHK(c, hipEventRecord(c->ev[2], ts));
			}
		}
		while(copied < chunks && (traced == K || traced - copied > ahead))
		{
			const int j = copied;
			const size_t off = (size_t)chunk_y[j] * W, cnt = (size_t)(chunk_y[j + 1] - chunk_y[j]) * W * 4;
			hipStream_t xs = cpy[j & 1];
			HIPCHK(c, hipStreamWaitEvent(xs, c->strip_ev[2 * j + 1], 0));
			if(timeline) HIPCHK(c, hipEventRecord(tl[4 * j + 2], xs));
			if(cnt != 0)
			{
				if(zbuf != NULL) HIPCHK(c, hipMemcpyAsync(zbuf + off, c->d_z + off, cnt, hipMemcpyDeviceToHost, xs));
				HIPCHK(c, hipMemcpyAsync(sbuf + off, fin + off, cnt, hipMemcpyDeviceToHost, xs));
			}
			if(timeline) HIPCHK(c, hipEventRecord(tl[4 * j + 3], xs));
			copied++;
		}
	}
	if(cpy[1] != cpy[0])
	{
		// (the first copy stream behind the second's last copy; strip_ev[0] -- strip 0's trace, long over -- is free for it)
		HIPCHK(c, hipEventRecord(c->strip_ev[0], cpy[1]));
		HIPCHK(c, hipStreamWaitEvent(cs, c->strip_ev[0], 0));
	}
	if(blur && chunks > 0) HIPCHK(c, hipStreamWaitEvent(cs, c->strip_ev[2 * (chunks - 1) + 1], 0));       // (the last chunk's blur)
	if(blur) HIPCHK(c, hipMemcpyAsync(c->h_strip_miss, c->d_strip_miss, 4, hipMemcpyDeviceToHost, cs));
	HIPCHK(c, hipEventRecord(c->ev[3], cs));
	HIPCHK(c, hipEventSynchronize(c->ev[3]));
	if(c->strip_copy_streams == 0)
	{
		struct timespec t1;
		clock_gettime(CLOCK_MONOTONIC, &t1);
		c->strip_calib_ms[c->strip_calib_n++] = (double)(t1.tv_sec - t_call0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t_call0.tv_nsec) * 1e-6;
		if(c->strip_calib_n == 16)
		{
			double med[2];
			for(int m = 0; m < 2; m++)
			{
				double v[7];
				for(int i = 0; i < 7; i++) v[i] = c->strip_calib_ms[8 * m + 1 + i];
				for(int i = 1; i < 7; i++) for(int k = i; k > 0 && v[k] < v[k - 1]; k--) { const double t = v[k]; v[k] = v[k - 1]; v[k - 1] = t; }
				med[m] = v[3];
			}
			c->strip_copy_streams = med[1] < med[0] ? 2 : 1;
		}
	}
	if(timeline)
	{
		fprintf(stderr, "strips %d, chunks %d:", K, chunks);
		for(int k = 0; k < K; k++) { float a = 0; (void)hipEventElapsedTime(&a, c->ev[0], tl[4 * k]); fprintf(stderr, " T%d(%d rows) %.3f", k, cuts[k + 1] - cuts[k], a); }
		for(int j = 0; j < chunks; j++)
		{
			float b = 0, d = 0, e = 0;
			(void)hipEventElapsedTime(&b, c->ev[0], tl[4 * j + 1]); (void)hipEventElapsedTime(&d, c->ev[0], tl[4 * j + 2]); (void)hipEventElapsedTime(&e, c->ev[0], tl[4 * j + 3]);
			fprintf(stderr, "\n   chunk %d rows %d: blur end %.3f copy %.3f..%.3f", j, chunk_y[j + 1] - chunk_y[j], b, d, e);
		}
		fprintf(stderr, "\n");
	}
	c->strip_calls++;
	if(blur && *c->h_strip_miss != 0u)
	{
		// a tap landed below the rows that were traced when its chunk was blurred: the whole pre-blur frame is there now, so
		// the pass again in one piece, and the frame again to the host (depth is what it was); the next calls in one piece
		c->strip_redone++;
		// (the short reach was not enough for this view: the long one from now on; that one too: one-piece calls for a while)
		if(c->strip_reach == 0) c->strip_reach = 1; else c->strip_backoff = 64;
		const pwn_blur_launch B = { .y0 = 0, .y1 = c->h, .d_pre = pre, .d_z = c->d_z, .d_out = fin, .stream = st[0] };
		rc = pwn_i_launch_blur(c, &B);
		if(rc != PWN_OK) return rc;
		rc = blocking_copies(c, st[0], sbuf, fin, NULL, NULL, n * 4);
		if(rc != PWN_OK) return rc;
		HIPCHK(c, hipEventSynchronize(c->ev[3]));
	}
#undef STRIPS_FAIL
	return PWN_OK;
}

extern "C" int pwn_trace_screen_centred(pwn_ctx *c, const float cam[16], float sec, uint32_t *sbuf, float *zbuf)
{
	if(GRP_HEAD(c)) return pwn_group_trace_screen_centred(c, cam, sec, sbuf, zbuf);
	if(c == NULL || cam == NULL || sbuf == NULL) return PWN_EINVAL;
	if(c->blur_passes > 0 && (c->w & 3) != 0) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	size_t n = (size_t)c->w * (size_t)c->h;
	hipStream_t s = c->stream;
	{ const int rc = pwn_i_wait_frames_in_flight(c, s); if(rc != PWN_OK) return rc; }
	// ---- in row strips, the copies beside the kernels (PWN_OPT_CALL_STRIPS)
	{
		int cuts[PWN_CALL_STRIPS_MAX + 1], K = 1;
		const bool can = c->blur_passes <= 1 && !c->counters_on && !c->wave_log_on && !c->unit_order && c->have_level;
		if(can && c->call_strips >= 2) K = strip_cuts(c, c->call_strips, cuts);
		// by frame size (profiles/r5/call_strips.txt): into registered buffers strips pay from 2560 x 1440 on (0.43 against 0.51 ms; 4K
		// 0.76 against 0.99, 8K 2.66 against 3.93) and not at 1080p (0.32 / 0.31); into pageable ones, where every chunk's copy holds
		// the caller, from 4K on (0.88 against 1.02 ms; 1440p equal, 1080p 0.44 against 0.33)
		else if(can && c->call_strips < 0 && c->h >= 256 &&
		        n >= ((host_is_pinned(sbuf, n * 4) && host_is_pinned(zbuf, n * 4)) ? 3000000u : 6000000u))
		{
			if(c->strip_backoff > 0) c->strip_backoff--;
			else K = strip_cuts(c, 0, cuts);
		}
		c->strips_last = K >= 2 ? K : 1;
		if(K >= 2)
		{
			const int rc = call_in_strips(c, cam, sec, sbuf, zbuf, cuts, K);
			if(rc != PWN_OK) return rc;
			if(c->blur_passes == 0) { uint32_t *t = c->d_pre; c->d_pre = c->d_out; c->d_out = t; }      // (the final frame stays addressable as d_out)
			stats_from_events(c, true);
			return PWN_OK;
		}
	}
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	// trace into d_pre; with blur on, d_pre plays tsbuf and d_out plays sbuf
	// (the memcpy of screen.h:75 becomes a pointer swap per pass)
	uint32_t *cur = c->d_pre, *other = c->d_out;
	pwn_trace_launch T = { .cam = cam, .sec = sec, .y0 = 0, .y1 = c->h, .d_sbuf = cur, .d_zbuf = c->d_z, .stream = s };
	int rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	for(int p = 0; p < c->blur_passes; p++)
	{
		const pwn_blur_launch B = { .y0 = 0, .y1 = c->h, .d_pre = cur, .d_z = c->d_z, .d_out = other, .stream = s };
		rc = pwn_i_launch_blur(c, &B);
		if(rc != PWN_OK) return rc;
		uint32_t *t = cur; cur = other; other = t;
	}
	HIPCHK(c, hipEventRecord(c->ev[2], s));
	HIPCHK(c, hipMemcpyAsync(sbuf, cur, n * 4, hipMemcpyDeviceToHost, s));
	if(zbuf != NULL) HIPCHK(c, hipMemcpyAsync(zbuf, c->d_z, n * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipEventRecord(c->ev[3], s));
	// (the units' order for the next call: behind the copies, and this call does not wait for it)
	rc = pwn_i_launch_order(c, s);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventSynchronize(c->ev[3]));
	// keep the final frame addressable as d_out for pwn_screen_upscale(NULL,...)
	if(cur != c->d_out) { c->d_pre = c->d_out; c->d_out = cur; }
	(void)hipEventElapsedTime(&c->stats.trace_ms, c->ev[0], c->ev[1]);
	(void)hipEventElapsedTime(&c->stats.blur_ms, c->ev[1], c->ev[2]);
	(void)hipEventElapsedTime(&c->stats.total_ms, c->ev[0], c->ev[3]);
	return PWN_OK;
}

// ---- a batch of views (pwn_trace_views) ----------------------------------------

// Three planes of `bytes` (pre-blur, colour, depth) or none: PWN_ENOMEM with nothing kept, the message is the caller's
static int planes3_alloc(size_t bytes, uint32_t **pre, uint32_t **out, float **z)
{
	*pre = *out = NULL; *z = NULL;
	if(hipMalloc((void **)pre, bytes) == hipSuccess && hipMalloc((void **)out, bytes) == hipSuccess && hipMalloc((void **)z, bytes) == hipSuccess) return PWN_OK;
	(void)hipGetLastError();
	(void)hipFree(*pre); (void)hipFree(*out); (void)hipFree(*z);
	return PWN_ENOMEM;
}

// Room for n views: the records (PWN_VIEWS_MAX of them, with the first batch) and n planes of each kind.  A larger n moves the
// depth planes of the slots so far into the new allocation and starts the new slots' planes at 0; the stream is idle behind
// that before the old planes go (no kernel of an earlier batch reads them: every batch ends with its stream drained).
static int view_recs_reserve(pwn_ctx *c)
{
	if(c->h_vrec == NULL)
	{
		HIPCHK(c, hipHostMalloc((void **)&c->h_vrec, PWN_VIEWS_MAX * sizeof(pwn_view_rec), hipHostMallocDefault));
		HIPCHK(c, hipMalloc((void **)&c->d_vrec, PWN_VIEWS_MAX * sizeof(pwn_view_rec)));
	}
	return PWN_OK;
}
static int views_reserve(pwn_ctx *c, int n, hipStream_t s)
{
	{ const int rc = view_recs_reserve(c); if(rc != PWN_OK) return rc; }
	if(n <= c->views_cap) return PWN_OK;
	const size_t plane = (size_t)c->w * (size_t)c->h, bytes = (size_t)n * plane * 4;
	uint32_t *pre, *out; float *z;
	if(planes3_alloc(bytes, &pre, &out, &z) != PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "pwn_trace_views: no room for %d views of %d x %d", n, c->w, c->h);
		return PWN_ENOMEM;
	}
	const size_t kept = (size_t)c->views_cap * plane * 4;
	if(kept > 0) HIPCHK(c, hipMemcpyAsync(z, c->d_vz, kept, hipMemcpyDeviceToDevice, s));
	HIPCHK(c, hipMemsetAsync((uint8_t *)z + kept, 0, bytes - kept, s));
	HIPCHK(c, hipStreamSynchronize(s));
	(void)hipFree(c->d_vpre); (void)hipFree(c->d_vout); (void)hipFree(c->d_vz);
	c->d_vpre = pre; c->d_vout = out; c->d_vz = z; c->views_cap = n;
	return PWN_OK;
}

extern "C" int pwn_trace_views(pwn_ctx *c, int n, const float *cams, const float *secs, uint32_t *sbuf, float *zbuf)
{
	GRP_REFUSE(c, "pwn_trace_views");
	if(c == NULL || cams == NULL || secs == NULL || sbuf == NULL || n < 1 || n > PWN_VIEWS_MAX) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c, n);
	if(rc != PWN_OK) return rc;
	const size_t plane = (size_t)c->w * (size_t)c->h;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = views_reserve(c, n, s);
	if(rc != PWN_OK) return rc;
	// every view's record from the blocking call's own set-up (frame_setup: this file's operation order is part of the bit-exact path)
	bool has_w = false;
	for(int i = 0; i < n; i++)
	{
		const float *cam = cams + 16 * (size_t)i;
		pwn_view_rec &r = c->h_vrec[i];
		frame_setup(c->w, c->h, cam, &r);
		r.sec_current = secs[i];
		r.hide = 0u; r.pad_[0] = r.pad_[1] = 0.0f;
		if(camera_has_w(cam)) has_w = true;
	}
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	// (the staging is free again: the call before this one ended with the stream drained)
	HIPCHK(c, pwn_launch_upload(c->h_vrec, c->d_vrec, (size_t)n * sizeof(pwn_view_rec), s));
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .views = { c->d_vrec, n, has_w, plane }, .d_sbuf = c->d_vpre, .d_zbuf = c->d_vz, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	uint32_t *cur = c->d_vpre;
	rc = pwn_i_blur_passes_run(c, { .y0 = 0, .y1 = c->h, .d_z = c->d_vz, .stream = s, .views = n }, &cur, c->d_vout);
	if(rc != PWN_OK) return rc;
	rc = blocking_copies(c, s, sbuf, cur, zbuf, c->d_vz, (size_t)n * plane * 4);
	if(rc != PWN_OK) return rc;
	return blocking_wait(c, true);
}

// d_hide of the *_hide_device calls (include/pwnhip.h): n int32 in device memory, 4-byte aligned, apart from every range the call
// writes -- wr[k] .. + wr_bytes (NULL: not given)
bool pwn_i_hide_array_ok(const void *d_hide, size_t n, const void *const *wr, int nwr, size_t wr_bytes)
{
	if(d_hide == NULL || ((uintptr_t)d_hide & 3u) != 0) return false;
	const uintptr_t h = (uintptr_t)d_hide, hb = (uintptr_t)n * 4;
	for(int k = 0; k < nwr; k++)
		if(wr[k] != NULL && h < (uintptr_t)wr[k] + wr_bytes && (uintptr_t)wr[k] < h + hb) return false;
	return true;
}

// The device form: cameras and planes of the caller's in device memory, everything on the caller's stream, nothing waited for.
// frame_setup runs on the device (view_setup.hip), into records of the library's.
// hide: pwn_trace_views_hide_device -- d_hide goes into the records with the cameras, and the launch is one of the HIDE kernels.
static int views_device(pwn_ctx *c, int n, const void *d_cams, const void *d_secs, bool hide, const void *d_hide, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream)
{
	if(c == NULL || d_cams == NULL || d_secs == NULL || d_sbuf == NULL || d_zbuf == NULL || n < 1 || n > PWN_VIEWS_MAX ||
	   (flags & ~PWN_VIEWS_HAS_W) != 0) return PWN_EINVAL;
	const size_t plane = (size_t)c->w * (size_t)c->h;
	if(c->blur_passes > 0 && d_work == NULL) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_secs | (uintptr_t)d_work | (uintptr_t)d_sbuf | (uintptr_t)d_zbuf) & 15u) != 0) return PWN_EINVAL;
	{
		const uintptr_t bytes = (uintptr_t)n * plane * 4, p[3] = { (uintptr_t)d_sbuf, (uintptr_t)d_zbuf, (uintptr_t)d_work };
		for(int i = 0; i < 3; i++) for(int k = i + 1; k < 3; k++)
			if(p[i] != 0 && p[k] != 0 && p[i] < p[k] + bytes && p[k] < p[i] + bytes) return PWN_EINVAL;
		const void *const wr[3] = { d_sbuf, d_zbuf, d_work };
		if(hide && !pwn_i_hide_array_ok(d_hide, (size_t)n, wr, 3, bytes)) return PWN_EINVAL;
	}
	// (the rules above and the first two of pwn_i_batch_refuse all answer PWN_EINVAL: their order among themselves decides nothing)
	int rc = pwn_i_batch_refuse(c, n);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	// (tables that cannot be packed refuse the call before anything is launched)
	if(c->blob_dirty) { rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	if(c->d_vrec_dev == NULL) HIPCHK(c, hipMalloc((void **)&c->d_vrec_dev, (size_t)PWN_TICKET_SETS * PWN_VIEWS_MAX * sizeof(pwn_view_rec)));
	// The records of the ticket set the trace launch below counts in (pwn_i_launch_trace): the launch that read them last is the
	// one 2R launches back, and launch n - R is behind it.  On one stream and in the rotation over R this stream is behind launch
	// n - R by itself; a call that leaves the pattern is put there before its set-up kernel writes, as its trace launch will be.
	const unsigned rot = (unsigned)c->launch_rot;
	if(c->launch_event[rot - 1] != NULL && c->launch_stream[rot - 1] != s) HIPCHK(c, hipStreamWaitEvent(s, c->launch_event[rot - 1], 0));
	pwn_view_rec *recs = c->d_vrec_dev + (size_t)(c->ticket_set % (2u * rot)) * PWN_VIEWS_MAX;
	if(hide) HIPCHK(c, pwn_launch_view_setup_hide((const float *)d_cams, (const float *)d_secs, (const int32_t *)d_hide, recs, n, c->w, c->h, s));
	else HIPCHK(c, pwn_launch_view_setup((const float *)d_cams, (const float *)d_secs, recs, n, c->w, c->h, s));
	// the trace into the plane from which the last blur pass lands in d_sbuf
	uint32_t *cur = (c->blur_passes & 1) ? (uint32_t *)d_work : (uint32_t *)d_sbuf;
	uint32_t *other = (c->blur_passes & 1) ? (uint32_t *)d_sbuf : (uint32_t *)d_work;
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .views = { recs, n, (flags & PWN_VIEWS_HAS_W) != 0, plane, NULL, hide }, .d_sbuf = cur, .d_zbuf = (float *)d_zbuf, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	return pwn_i_blur_passes_run(c, { .y0 = 0, .y1 = c->h, .d_z = (const float *)d_zbuf, .stream = s, .views = n }, &cur, other);
}
extern "C" int pwn_trace_views_device(pwn_ctx *c, int n, const void *d_cams, const void *d_secs, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_views_device");
	return views_device(c, n, d_cams, d_secs, false, NULL, flags, d_work, d_sbuf, d_zbuf, stream);
}
extern "C" int pwn_trace_views_hide_device(pwn_ctx *c, int n, const void *d_cams, const void *d_secs, const void *d_hide, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_views_hide_device");
	return views_device(c, n, d_cams, d_secs, true, d_hide, flags, d_work, d_sbuf, d_zbuf, stream);
}

// ---- views of their own sizes in one frame (pwn_trace_viewports) ----------------

// The records (PWN_VIEWS_MAX of them) and the three planes of w x h, with the first call.  The depth plane starts at zero and
// is never cleared again: it persists by destination pixel.
static int viewport_recs_reserve(pwn_ctx *c)
{
	if(c->h_prec == NULL)
	{
		HIPCHK(c, hipHostMalloc((void **)&c->h_prec, PWN_VIEWS_MAX * sizeof(pwn_viewport_rec), hipHostMallocDefault));
		HIPCHK(c, hipMalloc((void **)&c->d_prec, PWN_VIEWS_MAX * sizeof(pwn_viewport_rec)));
	}
	return PWN_OK;
}
static int viewports_reserve(pwn_ctx *c, hipStream_t s)
{
	{ const int rc = viewport_recs_reserve(c); if(rc != PWN_OK) return rc; }
	if(c->d_pz != NULL) return PWN_OK;
	const size_t bytes = (size_t)c->w * (size_t)c->h * 4;
	uint32_t *pre, *out; float *z;
	if(planes3_alloc(bytes, &pre, &out, &z) != PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "pwn_trace_viewports: no room for three planes of %d x %d", c->w, c->h);
		return PWN_ENOMEM;
	}
	c->d_ppre = pre; c->d_pout = out; c->d_pz = z;
	HIPCHK(c, hipMemsetAsync(z, 0, bytes, s));
	return PWN_OK;
}

// The order of the records and their geometry words (pwn_internal.h): what the host form makes per call and a layout of the device
// form bakes once.  Rising units (tables.h pwn_viewport_rec: the kernel's rounds), ties in the given order.
uint32_t pwn_i_viewport_recs_bake(int n, const pwn_viewport *vp, pwn_viewport_rec *recs, int *ord)
{
	uint32_t vu[PWN_VIEWS_MAX];
	for(int i = 0; i < n; i++) { ord[i] = i; vu[i] = (uint32_t)((vp[i].w + 15) / 16) * (uint32_t)((vp[i].h + 3) / 4); }
	std::stable_sort(ord, ord + n, [&vu](int a, int b) { return vu[a] < vu[b]; });
	uint32_t first = 0u, prev = 0u;
	for(int j = 0; j < n; j++)
	{
		const int i = ord[j];
		pwn_viewport_rec &r = recs[j];
		r.x = vp[i].x; r.y = vp[i].y; r.w = vp[i].w; r.h = vp[i].h;
		r.units_x = (uint32_t)((vp[i].w + 15) / 16); r.rows_u = (uint32_t)((vp[i].h + 3) / 4); r.units = vu[i];
		int sh;
		pwn_unit_div_magic(r.units_x, &r.ux_magic, &sh); r.ux_shift = sh;
		// segment j: rounds [prev, units) of the views j .. n-1
		r.seg_first = first; r.seg_round = prev;
		pwn_unit_div_magic((uint32_t)(n - j), &r.seg_magic, &sh); r.seg_shift = sh;
		first += (uint32_t)(n - j) * (r.units - prev); prev = r.units;
		r.hide = 0u; r.pad_ = 0u;
	}
	return first;
}

extern "C" int pwn_trace_viewports(pwn_ctx *c, int n, const pwn_viewport *vp, const float *cams, const float *secs, uint32_t *sbuf, float *zbuf)
{
	GRP_REFUSE(c, "pwn_trace_viewports");
	if(c == NULL || vp == NULL || cams == NULL || secs == NULL || sbuf == NULL) return PWN_EINVAL;
	// (the rules that need no context: the one function a host can ask beforehand)
	unsigned long long plan[4];
	if(pwn_viewports_plan(c->w, c->h, c->blur_passes, n, vp, plan) != PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "pwn_trace_viewports: %d rectangles of a %d x %d frame refused (the first offender: %llu)", n, c->w, c->h, plan[3]);
		return PWN_EINVAL;
	}
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = viewports_reserve(c, s);
	if(rc != PWN_OK) return rc;
	// The records, in order of rising units (tables.h pwn_viewport_rec: the kernel's rounds), each view's set-up from the blocking
	// call's own frame_setup for a frame of the VIEW's size (this file's operation order is part of the bit-exact path).
	// (the staging is free: the call before this one ended with the stream drained)
	int ord[PWN_VIEWS_MAX];
	const uint32_t first = pwn_i_viewport_recs_bake(n, vp, c->h_prec, ord);
	bool has_w = false;
	for(int j = 0; j < n; j++)
	{
		const int i = ord[j];
		const float *cam = cams + 16 * (size_t)i;
		pwn_viewport_rec &r = c->h_prec[j];
		frame_setup(vp[i].w, vp[i].h, cam, &r);
		r.sec_current = secs[i];
		if(camera_has_w(cam)) has_w = true;
	}
	if((unsigned long long)first != plan[0]) { snprintf(c->err, sizeof(c->err), "pwn_trace_viewports: %u units in the records, %llu planned", first, plan[0]); return PWN_EINVAL; }
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	HIPCHK(c, pwn_launch_upload(c->h_prec, c->d_prec, (size_t)n * sizeof(pwn_viewport_rec), s));
	// where no rectangle covers the frame colour reads 0: in the plane the trace writes and in the one the blur passes write
	// (with several passes the two take turns)
	const size_t plane = (size_t)c->w * (size_t)c->h;
	if(plan[1] < (unsigned long long)plane)
	{
		HIPCHK(c, hipMemsetAsync(c->d_ppre, 0, plane * 4, s));
		if(c->blur_passes > 0) HIPCHK(c, hipMemsetAsync(c->d_pout, 0, plane * 4, s));
	}
	const pwn_vps_launch V = { c->d_prec, c->h_prec, n, has_w, first, 0, 0, NULL };
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .vps = V, .d_sbuf = c->d_ppre, .d_zbuf = c->d_pz, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	uint32_t *cur = c->d_ppre;
	rc = pwn_i_blur_passes_run(c, { .y0 = 0, .y1 = c->h, .d_z = c->d_pz, .stream = s, .vps = V }, &cur, c->d_pout);
	if(rc != PWN_OK) return rc;
	rc = blocking_copies(c, s, sbuf, cur, zbuf, c->d_pz, plane * 4);
	if(rc != PWN_OK) return rc;
	return blocking_wait(c, true);
}

// ---- batches of rays (pwn_trace_rays, pwn_trace_hits) ----------------------------

// Room for n rays of a blocking ray call, kept across calls: pinned staging *h and a device buffer *d of the same layout, `per_ray`
// bytes a ray.  Grows to at least twice the old size; no kernel uses the old buffers (every call ends with its stream drained).
int pwn_i_staging_reserve(pwn_ctx *c, size_t n, size_t per_ray, const char *who, unsigned char **h, unsigned char **d, size_t *cap_io, size_t cap_max, const char *unit)
{
	if(n <= *cap_io) return PWN_OK;
	size_t cap = *cap_io * 2;
	if(cap < 4096) cap = 4096;
	if(cap > cap_max) cap = cap_max;
	if(cap < n) cap = n;
	const size_t bytes = cap * per_ray + 16;            // (+16: the upload kernel copies whole 16-byte words)
	unsigned char *nh = NULL, *nd = NULL;
	if(hipHostMalloc((void **)&nh, bytes, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&nd, bytes) != hipSuccess)
	{
		(void)hipGetLastError();
		if(nh != NULL) (void)hipHostFree(nh);
		(void)hipFree(nd);
		snprintf(c->err, sizeof(c->err), "%s: no room for %zu %s", who, n, unit);
		return PWN_ENOMEM;
	}
	if(*h != NULL) (void)hipHostFree(*h);
	(void)hipFree(*d);
	*h = nh; *d = nd; *cap_io = cap;
	return PWN_OK;
}

// What the blocking ray calls (the two here and pwn_reach.cpp's) do between filling their staging and reading it: N records into the staging's head, whether any
// has the w lanes of anything but an ordinary camera's rays (camera_has_w's rule for rays: origin.w 1, direction.w 0), the first
// `up` bytes of the staging to the device, the launch T of them, bytes [lo, hi) back, the wait and the times.
int pwn_i_rays_stage_and_launch(pwn_ctx *c, hipStream_t s, const float *rays, size_t N, unsigned char *h, unsigned char *d, size_t up,
	pwn_trace_launch *T, size_t lo, size_t hi)
{
	memcpy(h, rays, 32 * N);
	bool has_w = false;
	for(size_t i = 0; i < N && !has_w; i++) has_w = !(rays[8 * i + 3] == 1.0f && rays[8 * i + 7] == 0.0f);
	T->rays.has_w = has_w;
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	// (small batches by the upload kernel, as the view records: a DMA copy queues behind other copies of the device)
	if(up <= 65536) HIPCHK(c, pwn_launch_upload(h, d, up, s));
	else HIPCHK(c, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s));
	const int rc = pwn_i_launch_trace(c, T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	HIPCHK(c, hipMemcpyAsync(h + lo, d + lo, hi - lo, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipEventRecord(c->ev[3], s));
	return blocking_wait(c, false);
}

// pwn_trace_rays' staging for a call of n rays: the records at 0, the seeds at 32 n, the depths at 36 n and the colours at 40 n --
// one copy up (records, seeds, depths) and one down (depths, colours), 44 B a ray
extern "C" int pwn_trace_rays(pwn_ctx *c, int n, const float *rays, const uint32_t *seeds, float sec, uint32_t *col, float *depth)
{
	GRP_REFUSE(c, "pwn_trace_rays");
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && rays == NULL) || (col == NULL && depth == NULL)) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = pwn_i_staging_reserve(c, (size_t)n, 44, "pwn_trace_rays", &c->h_rays, &c->d_rays, &c->rays_cap);
	if(rc != PWN_OK) return rc;
	const size_t N = (size_t)n;
	unsigned char *h = c->h_rays, *d = c->d_rays;
	if(seeds != NULL) memcpy(h + 32 * N, seeds, 4 * N); else memset(h + 32 * N, 0, 4 * N);
	if(depth != NULL) memcpy(h + 36 * N, depth, 4 * N); else memset(h + 36 * N, 0, 4 * N);
	pwn_trace_launch T = { .sec = sec, .rays = { (const float *)d, (const uint32_t *)(d + 32 * N), (uint32_t)n },
		.d_sbuf = (uint32_t *)(d + 40 * N), .d_zbuf = (float *)(d + 36 * N), .stream = s };
	rc = pwn_i_rays_stage_and_launch(c, s, rays, N, h, d, 40 * N, &T, depth != NULL ? 36 * N : 40 * N, col != NULL ? 44 * N : 40 * N);
	if(rc != PWN_OK) return rc;
	if(depth != NULL) memcpy(depth, h + 36 * N, 4 * N);
	if(col != NULL) memcpy(col, h + 40 * N, 4 * N);
	return PWN_OK;
}

// hide: pwn_trace_rays_hide_device -- the launch reads ray i's hidden sphere from d_hide beside its record and is one of the HIDE kernels
static int rays_device(pwn_ctx *c, int n, const void *d_rays, const void *d_seeds, bool hide, const void *d_hide, float sec, int flags,
	void *d_col, void *d_depth, void *stream)
{
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && (d_rays == NULL || d_col == NULL || d_depth == NULL)) ||
	   (flags & ~PWN_RAYS_HAS_W) != 0) return PWN_EINVAL;
	if(((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_seeds & 3u) != 0 || ((uintptr_t)d_col & 3u) != 0 || ((uintptr_t)d_depth & 3u) != 0)
		return PWN_EINVAL;
	if(hide && n > 0)
	{
		const void *const wr[2] = { d_col, d_depth };
		if(!pwn_i_hide_array_ok(d_hide, (size_t)n, wr, 2, (size_t)n * 4)) return PWN_EINVAL;
	}
	const int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	pwn_trace_launch T = { .sec = sec, .rays = { (const float *)d_rays, (const uint32_t *)d_seeds, (uint32_t)n, (flags & PWN_RAYS_HAS_W) != 0, NULL, hide ? (const int32_t *)d_hide : NULL },
		.d_sbuf = (uint32_t *)d_col, .d_zbuf = (float *)d_depth, .stream = (hipStream_t)stream };
	return pwn_i_launch_trace(c, &T);
}
extern "C" int pwn_trace_rays_device(pwn_ctx *c, int n, const void *d_rays, const void *d_seeds, float sec, int flags,
	void *d_col, void *d_depth, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_rays_device");
	return rays_device(c, n, d_rays, d_seeds, false, NULL, sec, flags, d_col, d_depth, stream);
}
extern "C" int pwn_trace_rays_hide_device(pwn_ctx *c, int n, const void *d_rays, const void *d_seeds, const void *d_hide, float sec, int flags,
	void *d_col, void *d_depth, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_rays_hide_device");
	return rays_device(c, n, d_rays, d_seeds, true, d_hide, sec, flags, d_col, d_depth, stream);
}

static_assert(sizeof(pwn_hit) == PWN_HIT_REC_BYTES, "the kernel writes a pwn_hit as three 16-byte words (trace_kernel.hip trace_hit)");

// pwn_trace_hits' staging for a call of n rays: the records at 0 (32 B a ray), the hit records behind them at 32 n (48 B a ray;
// 16-byte aligned) -- one copy up, one down
extern "C" int pwn_trace_hits(pwn_ctx *c, int n, const float *rays, pwn_hit *hits)
{
	GRP_REFUSE(c, "pwn_trace_hits");
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && (rays == NULL || hits == NULL))) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = pwn_i_staging_reserve(c, (size_t)n, 32 + sizeof(pwn_hit), "pwn_trace_hits", &c->h_hits, &c->d_hits, &c->hits_cap);
	if(rc != PWN_OK) return rc;
	const size_t N = (size_t)n;
	unsigned char *h = c->h_hits, *d = c->d_hits;
	pwn_trace_launch T = { .rays = { (const float *)d, NULL, (uint32_t)n, false, d + 32 * N }, .stream = s };
	rc = pwn_i_rays_stage_and_launch(c, s, rays, N, h, d, 32 * N, &T, 32 * N, (32 + sizeof(pwn_hit)) * N);
	if(rc != PWN_OK) return rc;
	memcpy(hits, h + 32 * N, sizeof(pwn_hit) * N);
	return PWN_OK;
}

// hide: pwn_trace_hits_hide_device -- the launch reads ray i's hidden sphere from d_hide beside its record and is one of the HIDE kernels
static int hits_device(pwn_ctx *c, int n, const void *d_rays, bool hide, const void *d_hide, int flags, void *d_hits, void *stream)
{
	if(c == NULL || n < 0 || n > PWN_RAYS_MAX || (n > 0 && (d_rays == NULL || d_hits == NULL)) || (flags & ~PWN_RAYS_HAS_W) != 0) return PWN_EINVAL;
	if(((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_hits & 15u) != 0) return PWN_EINVAL;
	if(hide && n > 0 && !pwn_i_hide_array_ok(d_hide, (size_t)n, &d_hits, 1, (size_t)n * sizeof(pwn_hit))) return PWN_EINVAL;
	const int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	pwn_trace_launch T = { .rays = { (const float *)d_rays, NULL, (uint32_t)n, (flags & PWN_RAYS_HAS_W) != 0, d_hits, hide ? (const int32_t *)d_hide : NULL }, .stream = (hipStream_t)stream };
	return pwn_i_launch_trace(c, &T);
}
extern "C" int pwn_trace_hits_device(pwn_ctx *c, int n, const void *d_rays, int flags, void *d_hits, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_hits_device");
	return hits_device(c, n, d_rays, false, NULL, flags, d_hits, stream);
}
extern "C" int pwn_trace_hits_hide_device(pwn_ctx *c, int n, const void *d_rays, const void *d_hide, int flags, void *d_hits, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_hits_hide_device");
	return hits_device(c, n, d_rays, true, d_hide, flags, d_hits, stream);
}

// ---- first-hit planes of a batch of views (pwn_trace_view_hits) ------------------

// The staging of a call of N = n x w x h pixels: the label plane at 0, the cell plane at 4 N, the distance plane at 8 N, on the
// device and in pinned memory alike; the planes the caller wants come down, each in one copy, and go to the caller from there.
// It is pwn_trace_hits' staging (80 B a ray there: 12 N bytes are ceil(12 N / 80) rays of it), which is free between calls.
extern "C" int pwn_trace_view_hits(pwn_ctx *c, int n, const float *cams, uint32_t *label, uint32_t *cell, float *dist)
{
	GRP_REFUSE(c, "pwn_trace_view_hits");
	if(c == NULL || cams == NULL || label == NULL || n < 1 || n > PWN_VIEWS_MAX) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c, n, false);
	if(rc != PWN_OK) return rc;
	const size_t plane = (size_t)c->w * (size_t)c->h, N = (size_t)n * plane;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = view_recs_reserve(c);
	if(rc != PWN_OK) return rc;
	rc = pwn_i_staging_reserve(c, (12 * N + 79) / 80, 32 + sizeof(pwn_hit), "pwn_trace_view_hits", &c->h_hits, &c->d_hits, &c->hits_cap);
	if(rc != PWN_OK) return rc;
	// every view's record from the blocking call's own set-up, as pwn_trace_views; the primary segment reads no time
	bool has_w = false;
	for(int i = 0; i < n; i++)
	{
		const float *cam = cams + 16 * (size_t)i;
		pwn_view_rec &r = c->h_vrec[i];
		frame_setup(c->w, c->h, cam, &r);
		r.sec_current = 0.0f;
		r.hide = 0u; r.pad_[0] = r.pad_[1] = 0.0f;
		if(camera_has_w(cam)) has_w = true;
	}
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	// (the staging is free again: the call before this one ended with the stream drained)
	HIPCHK(c, pwn_launch_upload(c->h_vrec, c->d_vrec, (size_t)n * sizeof(pwn_view_rec), s));
	unsigned char *h = c->h_hits, *d = c->d_hits;
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .views = { c->d_vrec, n, has_w, plane, (uint32_t *)d },
		.d_sbuf = cell != NULL ? (uint32_t *)(d + 4 * N) : NULL, .d_zbuf = dist != NULL ? (float *)(d + 8 * N) : NULL, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	HIPCHK(c, hipMemcpyAsync(h, d, 4 * N, hipMemcpyDeviceToHost, s));
	if(cell != NULL) HIPCHK(c, hipMemcpyAsync(h + 4 * N, d + 4 * N, 4 * N, hipMemcpyDeviceToHost, s));
	if(dist != NULL) HIPCHK(c, hipMemcpyAsync(h + 8 * N, d + 8 * N, 4 * N, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipEventRecord(c->ev[3], s));
	rc = blocking_wait(c, false);
	if(rc != PWN_OK) return rc;
	memcpy(label, h, 4 * N);
	if(cell != NULL) memcpy(cell, h + 4 * N, 4 * N);
	if(dist != NULL) memcpy(dist, h + 8 * N, 4 * N);
	return PWN_OK;
}

// The device form: cameras and planes of the caller's in device memory, the set-up kernel (no times) and the trace launch on the
// caller's stream, nothing waited for -- pwn_trace_views_device without its blur
// hide: pwn_trace_view_hits_hide_device, as views_device
static int view_hits_device(pwn_ctx *c, int n, const void *d_cams, bool hide, const void *d_hide, int flags, void *d_label, void *d_cell, void *d_dist, void *stream)
{
	if(c == NULL || d_cams == NULL || d_label == NULL || n < 1 || n > PWN_VIEWS_MAX || (flags & ~PWN_VIEWS_HAS_W) != 0) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_label | (uintptr_t)d_cell | (uintptr_t)d_dist) & 15u) != 0) return PWN_EINVAL;
	const size_t plane = (size_t)c->w * (size_t)c->h;
	{
		const uintptr_t bytes = (uintptr_t)n * plane * 4, p[3] = { (uintptr_t)d_label, (uintptr_t)d_cell, (uintptr_t)d_dist };
		for(int i = 0; i < 3; i++) for(int k = i + 1; k < 3; k++)
			if(p[i] != 0 && p[k] != 0 && p[i] < p[k] + bytes && p[k] < p[i] + bytes) return PWN_EINVAL;
		const void *const wr[3] = { d_label, d_cell, d_dist };
		if(hide && !pwn_i_hide_array_ok(d_hide, (size_t)n, wr, 3, bytes)) return PWN_EINVAL;
	}
	int rc = pwn_i_batch_refuse(c, n, false);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	// (tables that cannot be packed refuse the call before anything is launched)
	if(c->blob_dirty) { rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	if(c->d_vrec_dev == NULL) HIPCHK(c, hipMalloc((void **)&c->d_vrec_dev, (size_t)PWN_TICKET_SETS * PWN_VIEWS_MAX * sizeof(pwn_view_rec)));
	// (the records of the ticket set the trace launch counts in, and the wait of a call that leaves the rotation: pwn_trace_views_device)
	const unsigned rot = (unsigned)c->launch_rot;
	if(c->launch_event[rot - 1] != NULL && c->launch_stream[rot - 1] != s) HIPCHK(c, hipStreamWaitEvent(s, c->launch_event[rot - 1], 0));
	pwn_view_rec *recs = c->d_vrec_dev + (size_t)(c->ticket_set % (2u * rot)) * PWN_VIEWS_MAX;
	if(hide) HIPCHK(c, pwn_launch_view_setup_hide((const float *)d_cams, NULL, (const int32_t *)d_hide, recs, n, c->w, c->h, s));
	else HIPCHK(c, pwn_launch_view_setup((const float *)d_cams, NULL, recs, n, c->w, c->h, s));
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .views = { recs, n, (flags & PWN_VIEWS_HAS_W) != 0, plane, (uint32_t *)d_label, hide },
		.d_sbuf = (uint32_t *)d_cell, .d_zbuf = (float *)d_dist, .stream = s };
	return pwn_i_launch_trace(c, &T);
}
extern "C" int pwn_trace_view_hits_device(pwn_ctx *c, int n, const void *d_cams, int flags, void *d_label, void *d_cell, void *d_dist, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_view_hits_device");
	return view_hits_device(c, n, d_cams, false, NULL, flags, d_label, d_cell, d_dist, stream);
}
extern "C" int pwn_trace_view_hits_hide_device(pwn_ctx *c, int n, const void *d_cams, const void *d_hide, int flags, void *d_label, void *d_cell, void *d_dist, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_view_hits_hide_device");
	return view_hits_device(c, n, d_cams, true, d_hide, flags, d_label, d_cell, d_dist, stream);
}

// ---- first-hit planes of views of their own sizes (pwn_trace_viewport_hits) -------

// pwn_trace_viewports' records (their times 0: the primary segment reads none) and launch geometry, pwn_trace_view_hits' planes and
// staging: N = w x h pixels, the label plane at 0, the cell plane at 4 N, the distance plane at 8 N of pwn_trace_hits' buffers.
// Where the rectangles leave some of the frame uncovered, the staging of every plane given is cleared on the device first: the
// planes come back 0 there.  The context grows by the records (pwn_trace_viewports' own, with the first call of either) and the
// staging; the planes and the depth plane of pwn_trace_viewports are neither made nor touched.
extern "C" int pwn_trace_viewport_hits(pwn_ctx *c, int n, const pwn_viewport *vp, const float *cams, uint32_t *label, uint32_t *cell, float *dist)
{
	GRP_REFUSE(c, "pwn_trace_viewport_hits");
	if(c == NULL || vp == NULL || cams == NULL || label == NULL) return PWN_EINVAL;
	// (the rules of pwn_trace_viewports with blur off, by the function a host can ask beforehand: these planes are never blurred)
	unsigned long long plan[4];
	if(pwn_viewports_plan(c->w, c->h, 0, n, vp, plan) != PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "pwn_trace_viewport_hits: %d rectangles of a %d x %d frame refused (the first offender: %llu)", n, c->w, c->h, plan[3]);
		return PWN_EINVAL;
	}
	int rc = pwn_i_batch_refuse(c, 0, false);
	if(rc != PWN_OK) return rc;
	const size_t N = (size_t)c->w * (size_t)c->h;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = viewport_recs_reserve(c);
	if(rc != PWN_OK) return rc;
	rc = pwn_i_staging_reserve(c, (12 * N + 79) / 80, 32 + sizeof(pwn_hit), "pwn_trace_viewport_hits", &c->h_hits, &c->d_hits, &c->hits_cap);
	if(rc != PWN_OK) return rc;
	// (the staging and the records are free: the call before this one ended with the stream drained)
	int ord[PWN_VIEWS_MAX];
	const uint32_t first = pwn_i_viewport_recs_bake(n, vp, c->h_prec, ord);
	bool has_w = false;
	for(int j = 0; j < n; j++)
	{
		const int i = ord[j];
		const float *cam = cams + 16 * (size_t)i;
		pwn_viewport_rec &r = c->h_prec[j];
		frame_setup(vp[i].w, vp[i].h, cam, &r);
		r.sec_current = 0.0f;
		if(camera_has_w(cam)) has_w = true;
	}
	if((unsigned long long)first != plan[0]) { snprintf(c->err, sizeof(c->err), "pwn_trace_viewport_hits: %u units in the records, %llu planned", first, plan[0]); return PWN_EINVAL; }
	HIPCHK(c, hipEventRecord(c->ev[0], s));
	HIPCHK(c, pwn_launch_upload(c->h_prec, c->d_prec, (size_t)n * sizeof(pwn_viewport_rec), s));
	unsigned char *h = c->h_hits, *d = c->d_hits;
	if(plan[1] < (unsigned long long)N)
	{
		HIPCHK(c, hipMemsetAsync(d, 0, 4 * N, s));
		if(cell != NULL) HIPCHK(c, hipMemsetAsync(d + 4 * N, 0, 4 * N, s));
		if(dist != NULL) HIPCHK(c, hipMemsetAsync(d + 8 * N, 0, 4 * N, s));
	}
	const pwn_vps_launch V = { c->d_prec, c->h_prec, n, has_w, first, 0, 0, NULL, (uint32_t *)d };
	pwn_trace_launch T = { .y0 = 0, .y1 = c->h, .vps = V,
		.d_sbuf = cell != NULL ? (uint32_t *)(d + 4 * N) : NULL, .d_zbuf = dist != NULL ? (float *)(d + 8 * N) : NULL, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	HIPCHK(c, hipEventRecord(c->ev[1], s));
	HIPCHK(c, hipMemcpyAsync(h, d, 4 * N, hipMemcpyDeviceToHost, s));
	if(cell != NULL) HIPCHK(c, hipMemcpyAsync(h + 4 * N, d + 4 * N, 4 * N, hipMemcpyDeviceToHost, s));
	if(dist != NULL) HIPCHK(c, hipMemcpyAsync(h + 8 * N, d + 8 * N, 4 * N, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipEventRecord(c->ev[3], s));
	rc = blocking_wait(c, false);
	if(rc != PWN_OK) return rc;
	memcpy(label, h, 4 * N);
	if(cell != NULL) memcpy(cell, h + 4 * N, 4 * N);
	if(dist != NULL) memcpy(dist, h + 8 * N, 4 * N);
	return PWN_OK;
}
