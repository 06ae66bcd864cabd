// pwn_frames.cpp -- frames in flight (pwn_frames_config, pwn_submit_frame, pwn_frame_ready, pwn_wait_frame).
#include <string.h>
#include "pwn_internal.h"

// ---- frames in flight ---------------------------------------------------------
// The reference's loop presents every frame on the host (main.c:107-109).  Over PCIe that
// copy takes longer than the kernels of a 4K frame, so a host that wants throughput keeps
// two or three frames in flight: while frame i travels to its pinned host buffers on the
// copy stream, the kernels of frame i+1 run on the compute stream.

static void slot_release(pwn_slot &sl)
{
	(void)hipFree(sl.d_out); (void)hipFree(sl.d_z); (void)hipFree(sl.d_surface);
	if(sl.h_sbuf) (void)hipHostFree(sl.h_sbuf);
	if(sl.h_zbuf) (void)hipHostFree(sl.h_zbuf);
	if(sl.h_surface) (void)hipHostFree(sl.h_surface);
	for(int k = 0; k < 4; k++) if(sl.ev_k[k]) (void)hipEventDestroy(sl.ev_k[k]);
	if(sl.ev_done) (void)hipEventDestroy(sl.ev_done);
	memset(&sl, 0, sizeof(sl));
}

void pwn_i_frames_release(pwn_ctx *c)
{
	// A slot's "kernels done" event may be what an upload would wait for (pwn_trace_launch.tables_event): no frame
	// is in flight here, so once the compute stream is empty no copy of the tables is in use any more
	if(c->nslots > 0)
	{
		if(c->stream) (void)hipStreamSynchronize(c->stream);
		if(c->stream2) (void)hipStreamSynchronize(c->stream2);
		for(int i = 0; i < PWN_NBLOB; i++) c->tables_in_use[i] = false;
	}
	c->last_frame_done = NULL;       // (a slot's event, destroyed below)
	pwn_launch_history_clear(c);
	for(int i = 0; i < PWN_MAX_SLOTS; i++) slot_release(c->slot[i]);
	c->nslots = 0;
}

extern "C" int pwn_frames_config(pwn_ctx *c, int nslots, int flags, int scale, int pitch_bytes)
{
	if(GRP_HEAD(c)) return pwn_group_frames_config(c, nslots, flags, scale, pitch_bytes);
	if(c == NULL || nslots < 0 || nslots > PWN_MAX_SLOTS || (flags & ~(PWN_FRAME_SBUF | PWN_FRAME_ZBUF | PWN_FRAME_SURFACE)) != 0) return PWN_EINVAL;
	if(flags & PWN_FRAME_SURFACE)
	{
		if(scale <= 0) return PWN_EINVAL;
		if(pitch_bytes == 0) pitch_bytes = c->w * scale * 4;
		if((pitch_bytes & 3) != 0 || (long long)pitch_bytes < (long long)c->w * scale * 4) return PWN_EINVAL;
	}
	else { scale = 1; pitch_bytes = 0; }
	(void)hipSetDevice(c->device);
	for(int i = 0; i < c->nslots; i++) if(c->slot[i].in_flight) return PWN_EBUSY;
	if(pwn_tiled_busy(c)) return PWN_EBUSY;            // (pwn_i_frames_release drops the guards of the tables their launches read)
	pwn_i_frames_release(c);
	const size_t n = (size_t)c->w * (size_t)c->h;
	const size_t surf_bytes = (size_t)pitch_bytes * (size_t)c->h * (size_t)scale;
	int rc = PWN_OK;
	for(int i = 0; i < nslots && rc == PWN_OK; i++)
	{
		pwn_slot &sl = c->slot[i];
		// every slot has its own final colour and depth planes: they are copied out (or looked at
		// by the caller) while the next frames are traced
		if(hipMalloc((void **)&sl.d_out, n * 4) != hipSuccess || hipMalloc((void **)&sl.d_z, n * 4) != hipSuccess) rc = PWN_ENOMEM;
		// like the context's depth plane: zero, and kept at pixels whose primary ray runs out of steps
		else if(hipMemset(sl.d_z, 0, n * 4) != hipSuccess || hipMemset(sl.d_out, 0, n * 4) != hipSuccess) rc = PWN_EHIP;
		if(rc == PWN_OK && (flags & PWN_FRAME_SBUF) && hipHostMalloc((void **)&sl.h_sbuf, n * 4, hipHostMallocDefault) != hipSuccess) rc = PWN_ENOMEM;
		if(rc == PWN_OK && (flags & PWN_FRAME_ZBUF) && hipHostMalloc((void **)&sl.h_zbuf, n * 4, hipHostMallocDefault) != hipSuccess) rc = PWN_ENOMEM;
		if(rc == PWN_OK && (flags & PWN_FRAME_SURFACE))
		{
			if(hipMalloc((void **)&sl.d_surface, surf_bytes) != hipSuccess || hipHostMalloc((void **)&sl.h_surface, surf_bytes, hipHostMallocDefault) != hipSuccess) rc = PWN_ENOMEM;
			else if(hipMemset(sl.d_surface, 0, surf_bytes) != hipSuccess) rc = PWN_EHIP;   // bytes between rows of a padded pitch stay 0
		}
		for(int k = 0; k < 4 && rc == PWN_OK; k++) if(hipEventCreate(&sl.ev_k[k]) != hipSuccess) rc = PWN_EHIP;
		if(rc == PWN_OK && hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming) != hipSuccess) rc = PWN_EHIP;
	}
	// the pre-blur plane of the frames on the second compute stream (PWN_OPT_FRAME_OVERLAP)
	if(rc == PWN_OK && nslots >= 2 && c->d_pre2 == NULL)
	{
		if(hipMalloc((void **)&c->d_pre2, n * 4) != hipSuccess) rc = PWN_ENOMEM;
		else if(hipMemset(c->d_pre2, 0, n * 4) != hipSuccess) rc = PWN_EHIP;
	}
	// (the memsets above run on the null stream, which the non-blocking streams of the frames do not wait for)
	if(rc == PWN_OK && hipDeviceSynchronize() != hipSuccess) rc = PWN_EHIP;
	if(rc != PWN_OK) { pwn_i_frames_release(c); return rc; }
	c->nslots = nslots; c->frame_flags = flags; c->frame_scale = scale; c->frame_pitch = pitch_bytes;
	return PWN_OK;
}

extern "C" int pwn_submit_frame(pwn_ctx *c, const float cam[16], float sec, int slot)
{
	if(GRP_HEAD(c)) return pwn_group_submit_frame(c, cam, sec, slot);
	if(c == NULL || cam == NULL || slot < 0 || slot >= c->nslots) return PWN_EINVAL;
	if(c->blur_passes > 0 && (c->w & 3) != 0) return PWN_EINVAL;
	pwn_slot &sl = c->slot[slot];
	if(sl.in_flight) return PWN_EBUSY;
	(void)hipSetDevice(c->device);
	const size_t n = (size_t)c->w * (size_t)c->h;
	// The kernels of a frame go one after the other on a compute stream, the copies to the host on the copy
	// stream behind their frame's last kernel.  Frames ALTERNATE between two compute streams (PWN_OPT_FRAME_OVERLAP,
	// the default): the trace grid of frame f+1 moves onto the CUs as the waves of frame f's grid run out of units
	// and leave, and the blur of frame f runs beside it -- what a single queue leaves idle in the tail of every
	// launch (mean wave residency 0.93 at 4K, 0.65 on a strip of an 8-way tiling).  For that a frame has its own
	// pre-blur plane (by parity), its own set of work-queue counters (four sets, pwn_i_launch_trace) and its own
	// copy of the tables if they changed (PWN_NBLOB).  (Blur and sink of frame i on a stream of their own beside the
	// trace of frame i+1 -- the kernels of ONE frame split over two queues -- measured nothing: 0.4433 against
	// 0.4429 ms per 4K frame.)  Every event between two kernels costs a few microseconds of pipeline, so only the
	// ones somebody reads are recorded.
	const bool counted = c->counters_on || c->wave_log_on;           // one set of counters: no second grid beside a counted one
	const bool overlap = c->frame_overlap && c->nslots >= 2 && !counted && c->blur_passes <= 1 && (c->d_pre2 != NULL || c->blur_passes == 0);
	const int par = overlap ? (int)(c->frame_seq & 1u) : 0;
	hipStream_t s = par ? c->stream2 : c->stream;
	uint32_t *pre = par ? c->d_pre2 : c->d_pre;
	// timing events: on every frame_timing-th frame (each event between two kernels is a few microseconds of
	// pipeline: 0.428 against 0.417 ms per 4K frame with all frames timed).  With two compute streams the
	// durations are those of kernels that share the chip with the neighbour frames' kernels: a host that wants
	// the duration of a launch by itself times frames with PWN_OPT_FRAME_OVERLAP 0 (bench.py's roofline leg).
	// (Making a timed frame run alone -- its stream waits for the frame before it, the next frame's for it -- was
	// tried: with the per-frame table upload in the picture the two waits between the streams cost 50 us per
	// frame at 4K, 0.4335 against 0.3629 ms.)
	const bool timing = c->frame_timing > 0 && (c->frame_seq % (uint64_t)c->frame_timing) == 0;
	// a frame on the other stream than the one before it is ordered behind that one only where the streams are
	// not meant to run side by side
	if(c->last_frame_done != NULL && c->last_frame_stream != s && !overlap) HIPCHK(c, hipStreamWaitEvent(s, c->last_frame_done, 0));
	if(timing) HIPCHK(c, hipEventRecord(sl.ev_k[0], s));
	// the last pass writes into the slot's own plane, which is what the copy stream reads while
	// the next frame's kernels reuse the context's d_pre / d_out
	uint32_t *cur = c->blur_passes > 0 ? pre : sl.d_out;
	pwn_trace_launch T = { .cam = cam, .sec = sec, .y0 = 0, .y1 = c->h, .d_sbuf = cur, .d_zbuf = sl.d_z, .stream = s,
		.tables_event = sl.ev_k[2],        // recorded below, behind the frame's last kernel
		.room = overlap ? pwn_room_for_launch(c) : 0 };
	int rc = pwn_i_launch_trace(c, &T);
	if(rc != PWN_OK) return rc;
	if(timing) HIPCHK(c, hipEventRecord(sl.ev_k[1], s));
	// (several passes: one stream, so `pre` is d_pre and takes turns with d_out)
	rc = pwn_i_blur_passes_run(c, { .y0 = 0, .y1 = c->h, .d_z = sl.d_z, .stream = s }, &cur, c->d_out, sl.d_out);
	if(rc != PWN_OK) { (void)hipEventRecord(sl.ev_k[2], s); return rc; }     // (the trace launch counts on this event)
	HIPCHK(c, hipEventRecord(sl.ev_k[2], s));
	c->last_frame_done = sl.ev_k[2]; c->last_frame_stream = s;
	hipEvent_t last = sl.ev_k[2];
	if(!(c->frame_flags & PWN_FRAME_SURFACE)) { rc = pwn_i_launch_order(c, s); if(rc != PWN_OK) return rc; }      // (behind the frame's "kernels done": nobody waits for it)
	if(c->frame_flags & PWN_FRAME_SURFACE)
	{
		HIPCHK(c, pwn_launch_upscale(sl.d_out, sl.d_surface, c->w, c->h, c->frame_scale, c->frame_pitch / 4, s));
		HIPCHK(c, hipEventRecord(sl.ev_k[3], s));
		last = sl.ev_k[3];
		rc = pwn_i_launch_order(c, s);
		if(rc != PWN_OK) return rc;
	}
	if(c->frame_flags != 0)
	{
		HIPCHK(c, hipStreamWaitEvent(c->copy_stream, last, 0));
		if(c->frame_flags & PWN_FRAME_SBUF) HIPCHK(c, hipMemcpyAsync(sl.h_sbuf, sl.d_out, n * 4, hipMemcpyDeviceToHost, c->copy_stream));
		if(c->frame_flags & PWN_FRAME_ZBUF) HIPCHK(c, hipMemcpyAsync(sl.h_zbuf, sl.d_z, n * 4, hipMemcpyDeviceToHost, c->copy_stream));
		if(c->frame_flags & PWN_FRAME_SURFACE)
			HIPCHK(c, hipMemcpyAsync(sl.h_surface, sl.d_surface, (size_t)c->frame_pitch * (size_t)c->h * (size_t)c->frame_scale,
				hipMemcpyDeviceToHost, c->copy_stream));
		HIPCHK(c, hipEventRecord(sl.ev_done, c->copy_stream));
	}
	sl.in_flight = true; sl.sec = sec; sl.seq = ++c->frame_seq; sl.timed = timing; sl.beside = overlap;
	return PWN_OK;
}

extern "C" int pwn_frame_ready(pwn_ctx *c, int slot)
{
	if(GRP_HEAD(c)) return pwn_group_frame_ready(c, slot);
	if(c == NULL || slot < 0 || slot >= c->nslots) return PWN_EINVAL;
	if(!c->slot[slot].in_flight) return 1;
	(void)hipSetDevice(c->device);
	hipError_t e = hipEventQuery(c->frame_flags != 0 ? c->slot[slot].ev_done : c->slot[slot].ev_k[2]);
	if(e == hipSuccess) return 1;
	if(e == hipErrorNotReady) return 0;
	snprintf(c->err, sizeof(c->err), "hipEventQuery: %s", hipGetErrorString(e));
	return PWN_EHIP;
}

extern "C" int pwn_wait_frame(pwn_ctx *c, int slot, pwn_frame *out)
{
	if(GRP_HEAD(c)) return pwn_group_wait_frame(c, slot, out);
	if(c == NULL || slot < 0 || slot >= c->nslots) return PWN_EINVAL;
	pwn_slot &sl = c->slot[slot];
	if(sl.seq == 0) return PWN_EINVAL;            // nothing was ever submitted here
	(void)hipSetDevice(c->device);
	if(sl.in_flight)
	{
		HIPCHK(c, hipEventSynchronize(c->frame_flags != 0 ? sl.ev_done : sl.ev_k[2]));
		sl.in_flight = false;
		if(sl.beside) pwn_room_frame_done(c);          // PWN_OPT_TRACE_ROOM: one more delivered frame of a two-stream sequence
	}
	if(out != NULL)
	{
		memset(out, 0, sizeof(*out));
		out->sbuf = sl.h_sbuf; out->zbuf = sl.h_zbuf; out->surface = sl.h_surface;
		out->surface_pitch_bytes = c->frame_pitch;
		out->d_sbuf = sl.d_out; out->d_zbuf = sl.d_z; out->d_surface = sl.d_surface;
		out->sec_current = sl.sec; out->seq = sl.seq;
		if(sl.timed)
		{
			(void)hipEventElapsedTime(&out->trace_ms, sl.ev_k[0], sl.ev_k[1]);
			(void)hipEventElapsedTime(&out->blur_ms, sl.ev_k[1], sl.ev_k[2]);
			if(c->frame_flags & PWN_FRAME_SURFACE) (void)hipEventElapsedTime(&out->sink_ms, sl.ev_k[2], sl.ev_k[3]);
			c->stats.trace_ms = out->trace_ms; c->stats.blur_ms = out->blur_ms;
		}
		out->timed = sl.timed ? 1 : 0;
	}
	return PWN_OK;
}
