// pwn_viewports_device.cpp -- views of their own sizes from cameras in device memory into planes of the caller's
// (pwn_trace_viewports_device), their first-hit planes (pwn_trace_viewport_hits_device), and the layouts that hold what such a call
// knows beforehand (pwn_viewports_layout).
#include <stdlib.h>
#include <string.h>
#include <new>
#include <algorithm>
#include "pwn_internal.h"

// What is known of a call without its cameras: the frame size and the rectangles, as records in the order the trace kernel wants
// them, their geometry words baked by the code the host form runs per call (pwn_calls.cpp pwn_i_viewport_recs_bake).
//   h_recs   the records on the host, heads zero: the blur launcher sizes its grid from them
//   d_mem    one device allocation: the same records (the set-up kernel's master copy), behind them per record the set-up scalars
//            of the view's own size (-yrat, xsrat, ysrat, 0) and the rectangle it stands for (perm), then the blur's skip-ahead
//            table of max(w_i) / 4 + 1 entries (the context's has w / 4 + 1 and is indexed by a view's LOCAL group)
//   use      per stream that calls have used the layout on, an event behind the last of them: pwn_viewports_layout_free waits for
//            these on the host.  An event holds one record, and a later call on the SAME stream is behind the earlier ones; a call on
//            a fifth stream takes over the oldest entry and is put behind that entry's record on the device first.
#define PWN_VPL_STREAMS 4
struct pwn_vp_layout
{
	pwn_ctx *ctx;
	int W, H, n;
	uint32_t units; unsigned long long pixels;
	bool blur_ok;
	pwn_viewport_rec *h_recs;
	uint8_t *d_mem;
	const pwn_viewport_rec *d_master; const float *d_scal; const uint32_t *d_perm; const uint2 *d_skip;
	int skip_n;
	struct { hipStream_t stream; hipEvent_t ev; bool used; unsigned long long stamp; } use[PWN_VPL_STREAMS];
	unsigned long long stamp;
};

static void layout_release(pwn_vp_layout *l)
{
	for(int i = 0; i < PWN_VPL_STREAMS; i++) if(l->use[i].ev != NULL) (void)hipEventDestroy(l->use[i].ev);
	(void)hipFree(l->d_mem);
	free(l->h_recs);
	delete l;
}

extern "C" int pwn_viewports_layout(pwn_ctx *c, int W, int H, int n, const pwn_viewport *vp, pwn_vp_layout **out)
{
	GRP_REFUSE(c, "pwn_viewports_layout");
	if(c == NULL || out == NULL) return PWN_EINVAL;
	*out = NULL;
	// (the rules of the host form with blur off, by the function the host form calls; the blur rules are recorded, not enforced here)
	unsigned long long plan[4];
	if(pwn_viewports_plan(W, H, 0, n, vp, plan) != PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "pwn_viewports_layout: %d rectangles of a %d x %d frame refused (the first offender: %llu)", n, W, H, plan[3]);
		return PWN_EINVAL;
	}
	pwn_vp_layout *l = new(std::nothrow) pwn_vp_layout();
	if(l == NULL) return PWN_ENOMEM;
	l->ctx = c; l->W = W; l->H = H; l->n = n; l->pixels = plan[1];
	l->h_recs = (pwn_viewport_rec *)calloc((size_t)n, sizeof(pwn_viewport_rec));
	if(l->h_recs == NULL) { layout_release(l); return PWN_ENOMEM; }
	int ord[PWN_VIEWS_MAX];
	l->units = pwn_i_viewport_recs_bake(n, vp, l->h_recs, ord);
	if((unsigned long long)l->units != plan[0])
	{
		snprintf(c->err, sizeof(c->err), "pwn_viewports_layout: %u units in the records, %llu planned", l->units, plan[0]);
		layout_release(l);
		return PWN_EINVAL;
	}
	int wide = 0;
	l->blur_ok = (W & 3) == 0;
	for(int i = 0; i < n; i++)
	{
		if(vp[i].w > wide) wide = vp[i].w;
		if((vp[i].x & 3) != 0 || (vp[i].w & 3) != 0) l->blur_ok = false;
	}
	l->skip_n = wide / 4 + 1;
	// the device image, built on the host: records | scalars | perm (padded to 16 bytes) | skip
	const size_t off_scal = (size_t)n * sizeof(pwn_viewport_rec), off_perm = off_scal + (size_t)n * 16,
		off_skip = off_perm + (((size_t)n * 4 + 15) & ~(size_t)15), bytes = off_skip + (size_t)l->skip_n * sizeof(uint2);
	uint8_t *img = (uint8_t *)calloc(1, bytes);
	if(img == NULL) { layout_release(l); return PWN_ENOMEM; }
	memcpy(img, l->h_recs, off_scal);
	for(int j = 0; j < n; j++)
	{
		const int i = ord[j];
		if(i < 0 || i >= n) { free(img); layout_release(l); return PWN_EINVAL; }       // (the set-up kernel indexes the cameras with it)
		const pwn_setup_scalars S = pwn_frame_setup_scalars(vp[i].w, vp[i].h);
		const float sc[4] = { -S.yrat, S.xsrat, S.ysrat, 0.0f };
		memcpy(img + off_scal + 16 * (size_t)j, sc, 16);
		const uint32_t p = (uint32_t)i;
		memcpy(img + off_perm + 4 * (size_t)j, &p, 4);
	}
	{
		// (pwn_init's table, to this layout's length: entry g maps a row seed to the seed 32 g draws later, whatever the width)
		uint32_t A = 1, C = 0;
		for(int g = 0; g < l->skip_n; g++)
		{
			const uint2 e = { A, C };
			memcpy(img + off_skip + sizeof(uint2) * (size_t)g, &e, sizeof(e));
			for(int k = 0; k < 32; k++) { A = (A * 25739u) & 0x7FFFFFFFu; C = (C * 25739u + 4u) & 0x7FFFFFFFu; }
		}
	}
	(void)hipSetDevice(c->device);
	int rc = PWN_OK;
	if(hipMalloc((void **)&l->d_mem, bytes) != hipSuccess) { (void)hipGetLastError(); l->d_mem = NULL; rc = PWN_ENOMEM; }
	for(int i = 0; i < PWN_VPL_STREAMS && rc == PWN_OK; i++)
		if(hipEventCreateWithFlags(&l->use[i].ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); l->use[i].ev = NULL; rc = PWN_ENOMEM; }
	// (a blocking copy from pageable memory: through when it returns, whatever stream the first call comes on)
	if(rc == PWN_OK && hipMemcpy(l->d_mem, img, bytes, hipMemcpyHostToDevice) != hipSuccess)
	{
		snprintf(c->err, sizeof(c->err), "pwn_viewports_layout: hipMemcpy of %zu bytes: %s", bytes, hipGetErrorString(hipGetLastError()));
		rc = PWN_EHIP;
	}
	free(img);
	if(rc == PWN_OK) { try { c->vp_layouts.push_back(l); } catch(const std::bad_alloc &) { rc = PWN_ENOMEM; } }
	if(rc != PWN_OK)
	{
		if(rc == PWN_ENOMEM) snprintf(c->err, sizeof(c->err), "pwn_viewports_layout: no room for %d records", n);
		layout_release(l);
		return rc;
	}
	l->d_master = (const pwn_viewport_rec *)l->d_mem; l->d_scal = (const float *)(l->d_mem + off_scal);
	l->d_perm = (const uint32_t *)(l->d_mem + off_perm); l->d_skip = (const uint2 *)(l->d_mem + off_skip);
	*out = l;
	return PWN_OK;
}

// (a layout is looked at only once it is found among the context's: one that was freed, or another context's, is never dereferenced)
static bool layout_of(const pwn_ctx *c, const pwn_vp_layout *l)
{
	return std::find(c->vp_layouts.begin(), c->vp_layouts.end(), l) != c->vp_layouts.end();
}

extern "C" int pwn_viewports_layout_free(pwn_ctx *c, pwn_vp_layout *l)
{
	GRP_REFUSE(c, "pwn_viewports_layout_free");
	if(c == NULL || l == NULL || !layout_of(c, l)) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	// behind the last launch that reads the master copy, the skip-ahead table or -- the blur launcher, on the host -- h_recs
	int rc = PWN_OK;
	for(int i = 0; i < PWN_VPL_STREAMS; i++)
		if(l->use[i].used && hipEventSynchronize(l->use[i].ev) != hipSuccess)
		{
			snprintf(c->err, sizeof(c->err), "pwn_viewports_layout_free: hipEventSynchronize: %s", hipGetErrorString(hipGetLastError()));
			rc = PWN_EHIP;
		}
	c->vp_layouts.erase(std::find(c->vp_layouts.begin(), c->vp_layouts.end(), l));
	layout_release(l);
	return rc;
}

extern "C" int pwn_viewports_layout_info(const pwn_vp_layout *l, unsigned long long out[6])
{
	if(l == NULL || out == NULL) return PWN_EINVAL;
	out[0] = (unsigned long long)l->W; out[1] = (unsigned long long)l->H; out[2] = (unsigned long long)l->n;
	out[3] = l->units; out[4] = l->pixels; out[5] = l->blur_ok ? 1ull : 0ull;
	return PWN_OK;
}

// (pwn_destroy, every stream idle)
void pwn_i_viewports_device_release(pwn_ctx *c)
{
	for(pwn_vp_layout *l : c->vp_layouts) layout_release(l);
	c->vp_layouts.clear();
	(void)hipFree(c->d_prec_dev);
	c->d_prec_dev = NULL;
}

// What the two device forms share once a call's own arguments are in order: the records of the ticket set the trace launch will count
// in, made on the device (viewport_setup.hip) on the caller's stream, and the layout's entry for that stream.  d_secs NULL: every
// time 0 (the first-hit planes read none).  *slot is the entry whose event vps_device_used records behind whatever the call launches.
// hide: the *_hide_device forms -- d_hide goes into the records with the cameras.  A call without it writes 0 into every record's
// word (the master copy's), so a set that held a hide call's records before holds nothing of them.
static int vps_device_records(pwn_ctx *c, pwn_vp_layout *lw, const void *d_cams, const void *d_secs, bool hide, const void *d_hide, hipStream_t s, int *slot_out, pwn_viewport_rec **recs_out)
{
	int rc;
	// (tables that cannot be packed refuse the call before anything is launched)
	if(c->blob_dirty) { rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	if(c->d_prec_dev == NULL) HIPCHK(c, hipMalloc((void **)&c->d_prec_dev, (size_t)PWN_TICKET_SETS * PWN_VIEWS_MAX * sizeof(pwn_viewport_rec)));
	// the layout's entry for this stream: its own, a free one, or the oldest -- behind whose record this stream is put, so that the
	// record made below stands for that one too
	int slot = -1;
	for(int i = 0; i < PWN_VPL_STREAMS && slot < 0; i++) if(lw->use[i].used && lw->use[i].stream == s) slot = i;
	for(int i = 0; i < PWN_VPL_STREAMS && slot < 0; i++) if(!lw->use[i].used) slot = i;
	if(slot < 0)
	{
		slot = 0;
		for(int i = 1; i < PWN_VPL_STREAMS; i++) if(lw->use[i].stamp < lw->use[slot].stamp) slot = i;
		HIPCHK(c, hipStreamWaitEvent(s, lw->use[slot].ev, 0));
	}
	// (the records of the ticket set the trace launch counts in, and the wait of a call that leaves the rotation: pwn_trace_views_device)
	const unsigned rot = (unsigned)c->launch_rot;
	if(c->launch_event[rot - 1] != NULL && c->launch_stream[rot - 1] != s) HIPCHK(c, hipStreamWaitEvent(s, c->launch_event[rot - 1], 0));
	pwn_viewport_rec *recs = c->d_prec_dev + (size_t)(c->ticket_set % (2u * rot)) * PWN_VIEWS_MAX;
	if(hide) HIPCHK(c, pwn_launch_viewport_setup_hide(lw->d_master, lw->d_scal, lw->d_perm, (const float *)d_cams, (const float *)d_secs, (const int32_t *)d_hide, recs, lw->n, s));
	else HIPCHK(c, pwn_launch_viewport_setup(lw->d_master, lw->d_scal, lw->d_perm, (const float *)d_cams, (const float *)d_secs, recs, lw->n, s));
	lw->use[slot].stream = s; lw->use[slot].used = true; lw->use[slot].stamp = ++lw->stamp;
	*slot_out = slot; *recs_out = recs;
	return PWN_OK;
}
// (behind whatever went out, also where a launch failed: the set-up kernel has read the master copy)
static int vps_device_used(pwn_ctx *c, pwn_vp_layout *lw, int slot, hipStream_t s, int rc, const char *who)
{
	if(hipEventRecord(lw->use[slot].ev, s) != hipSuccess && rc == PWN_OK)
	{
		snprintf(c->err, sizeof(c->err), "%s: hipEventRecord: %s", who, hipGetErrorString(hipGetLastError()));
		rc = PWN_EHIP;
	}
	return rc;
}
// (no two of up to three plane ranges of `bytes` bytes overlap; a NULL plane is none)
static bool planes_apart(uintptr_t bytes, const void *a, const void *b, const void *d)
{
	const uintptr_t p[3] = { (uintptr_t)a, (uintptr_t)b, (uintptr_t)d };
	for(int i = 0; i < 3; i++) for(int k = i + 1; k < 3; k++)
		if(p[i] != 0 && p[k] != 0 && p[i] < p[k] + bytes && p[k] < p[i] + bytes) return false;
	return true;
}

// The device form of pwn_trace_viewports: cameras and planes of the caller's in device memory, everything on the caller's stream,
// nothing waited for.  The records are made on the device (viewport_setup.hip) into the library's, per ticket set as
// pwn_trace_views_device's; the planes are of the LAYOUT's size, which the launchers are told (pwn_vps_launch.fw / fh).
// hide: pwn_trace_viewports_hide_device -- d_hide, one entry per rectangle in the caller's order, goes into the records with the
// cameras, and the trace launch is one of the HIDE kernels; `who` names the entry in messages.
static int viewports_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, const void *d_secs, bool hide, const void *d_hide, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream, const char *who)
{
	if(c == NULL || l == NULL || d_cams == NULL || d_secs == NULL || d_sbuf == NULL || d_zbuf == NULL || (flags & ~PWN_VIEWS_HAS_W) != 0) return PWN_EINVAL;
	if(!layout_of(c, l)) return PWN_EINVAL;
	if(c->blur_passes > 0 && (d_work == NULL || !l->blur_ok)) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_secs | (uintptr_t)d_work | (uintptr_t)d_sbuf | (uintptr_t)d_zbuf) & 15u) != 0) return PWN_EINVAL;
	if(!planes_apart((uintptr_t)l->W * (uintptr_t)l->H * 4, d_sbuf, d_zbuf, d_work)) return PWN_EINVAL;
	{
		const void *const wr[3] = { d_sbuf, d_zbuf, d_work };
		if(hide && !pwn_i_hide_array_ok(d_hide, (size_t)l->n, wr, 3, (size_t)l->W * (size_t)l->H * 4)) return PWN_EINVAL;
	}
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	pwn_vp_layout *lw = const_cast<pwn_vp_layout *>(l);
	int slot; pwn_viewport_rec *recs;
	rc = vps_device_records(c, lw, d_cams, d_secs, hide, d_hide, s, &slot, &recs);
	if(rc != PWN_OK) return rc;
	// the trace into the plane from which the last blur pass lands in d_sbuf
	uint32_t *cur = (c->blur_passes & 1) ? (uint32_t *)d_work : (uint32_t *)d_sbuf;
	uint32_t *other = (c->blur_passes & 1) ? (uint32_t *)d_sbuf : (uint32_t *)d_work;
	const pwn_vps_launch V = { recs, l->h_recs, l->n, (flags & PWN_VIEWS_HAS_W) != 0, l->units, l->W, l->H, l->d_skip, NULL, hide };
	pwn_trace_launch T = { .y0 = 0, .y1 = l->H, .vps = V, .d_sbuf = cur, .d_zbuf = (float *)d_zbuf, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	// The blur reads a record's rectangle alone, and reads it from the layout's master copy, which nothing ever writes: the trace launch
	// is what the rotation's waits order, so a call two launches on, on another stream, may be handed this call's records for its set-up
	// while this call's blur passes are still to run.
	const pwn_vps_launch VB = { l->d_master, l->h_recs, l->n, V.has_w, l->units, l->W, l->H, l->d_skip, NULL };
	if(rc == PWN_OK) rc = pwn_i_blur_passes_run(c, { .y0 = 0, .y1 = l->H, .d_z = (const float *)d_zbuf, .stream = s, .vps = VB }, &cur, other);
	return vps_device_used(c, lw, slot, s, rc, who);
}
extern "C" int pwn_trace_viewports_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, const void *d_secs, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_viewports_device");
	return viewports_device(c, l, d_cams, d_secs, false, NULL, flags, d_work, d_sbuf, d_zbuf, stream, "pwn_trace_viewports_device");
}
extern "C" int pwn_trace_viewports_hide_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, const void *d_secs, const void *d_hide, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_viewports_hide_device");
	return viewports_device(c, l, d_cams, d_secs, true, d_hide, flags, d_work, d_sbuf, d_zbuf, stream, "pwn_trace_viewports_hide_device");
}

// The device form of pwn_trace_viewport_hits: the call above with the first-hit planes in the place of colour and depth -- the same
// records (their times 0), rotation and layout-use event, one set-up launch and one trace launch, no blur.  Every layout qualifies.
// hide: pwn_trace_viewport_hits_hide_device, as viewports_device
static int viewport_hits_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, bool hide, const void *d_hide, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream, const char *who)
{
	if(c == NULL || l == NULL || d_cams == NULL || d_label == NULL || (flags & ~PWN_VIEWS_HAS_W) != 0) return PWN_EINVAL;
	if(!layout_of(c, l)) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_label | (uintptr_t)d_cell | (uintptr_t)d_dist) & 15u) != 0) return PWN_EINVAL;
	if(!planes_apart((uintptr_t)l->W * (uintptr_t)l->H * 4, d_label, d_cell, d_dist)) return PWN_EINVAL;
	{
		const void *const wr[3] = { d_label, d_cell, d_dist };
		if(hide && !pwn_i_hide_array_ok(d_hide, (size_t)l->n, wr, 3, (size_t)l->W * (size_t)l->H * 4)) return PWN_EINVAL;
	}
	int rc = pwn_i_batch_refuse(c, 0, false);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	pwn_vp_layout *lw = const_cast<pwn_vp_layout *>(l);
	int slot; pwn_viewport_rec *recs;
	rc = vps_device_records(c, lw, d_cams, NULL, hide, d_hide, s, &slot, &recs);
	if(rc != PWN_OK) return rc;
	const pwn_vps_launch V = { recs, l->h_recs, l->n, (flags & PWN_VIEWS_HAS_W) != 0, l->units, l->W, l->H, NULL, (uint32_t *)d_label, hide };
	pwn_trace_launch T = { .y0 = 0, .y1 = l->H, .vps = V, .d_sbuf = (uint32_t *)d_cell, .d_zbuf = (float *)d_dist, .stream = s };
	rc = pwn_i_launch_trace(c, &T);
	return vps_device_used(c, lw, slot, s, rc, who);
}
extern "C" int pwn_trace_viewport_hits_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_viewport_hits_device");
	return viewport_hits_device(c, l, d_cams, false, NULL, flags, d_label, d_cell, d_dist, stream, "pwn_trace_viewport_hits_device");
}
extern "C" int pwn_trace_viewport_hits_hide_device(pwn_ctx *c, const pwn_vp_layout *l, const void *d_cams, const void *d_hide, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_viewport_hits_hide_device");
	return viewport_hits_device(c, l, d_cams, true, d_hide, flags, d_label, d_cell, d_dist, stream, "pwn_trace_viewport_hits_hide_device");
}
