// pwn_launch.cpp -- what goes out to the device per launch: the trace launcher (pwn_i_launch_trace, its geometry from
// launch_plan.h), the unit order behind it, the blur launcher, and the entry points that are one launch (pwn_*_rows_device).
#include <stdlib.h>
#include <string.h>
#include <xmmintrin.h>      // pwn_pixel_rays: FTZ|DAZ
#include "pwn_internal.h"
#include "launch_plan.h"

// The ray record and seed of pixels (x, y) of a frame, exactly as the trace kernel makes them: frame_setup, then screen.h:12-18
// in the reference build's order, rayl = (cx*rdx + rayb) + y*rdy and one "+= rdx" per pixel of the 32-wide tile up to and
// including this one.  The chain runs under FTZ|DAZ, as the device does and as the reference executable does (crtfastmath.o), so
// that a denormal camera gives the frame's rays; frame_setup runs in the default mode, as for the frame launches.
extern "C" int pwn_pixel_rays(int width, int height, const float cam[16], int n, const int32_t *xy, float *rays, uint32_t *seeds)
{
	if(cam == NULL || n < 0 || n > PWN_RAYS_MAX || width <= 0 || height <= 0 || width > 32768 || height > 32768) return PWN_EINVAL;
	if(n > 0 && (xy == NULL || rays == NULL)) return PWN_EINVAL;
	for(int i = 0; i < n; i++)
		if(xy[2 * i] < 0 || xy[2 * i] >= width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= height) return PWN_EINVAL;
	pwn_trace_params P;
	frame_setup(width, height, cam, &P);
	const unsigned csr = _mm_getcsr();
	_mm_setcsr(csr | 0x8040u);
	for(int i = 0; i < n; i++)
	{
		const int x = xy[2 * i], y = xy[2 * i + 1], cx0 = x & ~31;
		float *r = rays + 8 * (size_t)i;
		for(int k = 0; k < 4; k++)
		{
			float v = ((float)cx0 * P.rdx[k] + P.rayb[k]) + (float)y * P.rdy[k];
			for(int j = cx0; j <= x; j++) v += P.rdx[k];
			r[k] = P.from[k];
			r[4 + k] = v;
		}
		if(seeds != NULL)
		{
			// screen.h:19-21 (uint32 wrap-around)
			uint32_t sd = (uint32_t)x + (uint32_t)y * (uint32_t)y * ((uint32_t)width + 1u);
			sd *= sd * sd;
			sd *= sd * sd;
			seeds[i] = sd;
		}
	}
	_mm_setcsr(csr);
	return PWN_OK;
}

// the unit-order entry of a stream (pwn_internal.h); NULL: none to spare right now
static pwn_ctx::unit_order_state *order_entry(pwn_ctx *c, hipStream_t stream, bool make)
{
	if(stream == c->stream) { c->order[0].key = stream; c->order[0].used = true; return &c->order[0]; }
	if(c->stream2 != NULL && stream == c->stream2) { c->order[1].key = stream; c->order[1].used = true; return &c->order[1]; }
	for(int i = 2; i < 4; i++) if(c->order[i].used && c->order[i].key == stream) { c->order[i].stamp = ++c->order_stamp; return &c->order[i]; }
	if(!make) return NULL;
	int pick = -1;
	for(int i = 2; i < 4; i++) if(!c->order[i].used) { pick = i; break; }
	if(pick < 0)
	{
		// both spare entries belong to other streams of the caller, whose kernels may still be using them: the older one is
		// taken over once the device is idle (a host that rotates over many streams pays for it; two are free)
		pick = c->order[2].stamp < c->order[3].stamp ? 2 : 3;
		if(hipDeviceSynchronize() != hipSuccess) return NULL;
	}
	pwn_ctx::unit_order_state &e = c->order[pick];
	e.key = stream; e.used = true; e.stamp = ++c->order_stamp; e.perm_valid = e.cost_fresh = false;
	return &e;
}

// (the events of the launch history belong to frame slots / the row tiling: forget them where those go, with the
// compute streams idle)
void pwn_launch_history_clear(pwn_ctx *c)
{
	for(int i = 0; i < 3; i++) { c->launch_stream[i] = NULL; c->launch_event[i] = NULL; }
}

// How many streams successive trace launches rotate over (pwn_tiled.cpp: 3 for a tiling on three compute streams, else 2).
// The work-queue counters are used in turn, 2R sets: a change starts them afresh, with the device idle.
int pwn_i_set_launch_rotation(pwn_ctx *c, int rot)
{
	if(rot != 2 && rot != 3) return PWN_EINVAL;
	if(c->launch_rot == rot) return PWN_OK;
	HIPCHK(c, hipDeviceSynchronize());
	HIPCHK(c, hipMemset(c->d_tickets, 0, PWN_TICKET_SETS * PWN_QUEUES * PWN_QUEUE_STRIDE * sizeof(uint32_t)));
	c->ticket_set = 0; c->launch_rot = rot;
	pwn_launch_history_clear(c);
	return PWN_OK;
}

// ---- the trace launch: pwn_i_launch_trace and its parts, in the order it goes through them ----

// What a launch reads of the tables in force (copy `cur`): the blob, the sections of the lists' global form, the balls
static void params_tables(const pwn_ctx *c, int cur, pwn_trace_params *P)
{
	P->blob_bytes = (uint32_t)c->blob.size();
	P->off_sph = c->off_sph;
	P->off_recsph = c->off_recsph;
	P->blob = (const uint32_t *)c->d_blob[cur];
	// the lists' global form (tables.h): blob_bytes is the LDS part, the rest is read where it lies.  Nothing in the launcher but the
	// choice of the kernel knows the form.
	if(c->lists_form == PWN_LF_GLOBAL)
	{
		P->g_rec = (const float *)c->d_big[cur];
		P->g_which = (const uint32_t *)(c->d_big[cur] + c->big_which);
		P->g_sph = (const float *)(c->d_big[cur] + c->big_sph);
	}
	// the balls of these tables' longest lists (pwn_i_pack_blob made them with the tables; a launch reads no tables but c->blob_cur's)
	P->nbounds = c->dbg_sphere_bounds ? c->nbounds : 0;
	for(int i = 0; i < PWN_BOUNDS_MAX; i++)
	{
		P->bound_ids[i] = 0xffffffffu;
		if(i < P->nbounds) { P->bounds[i] = c->bounds[i]; P->bound_ids[i] = c->bounds[i].id; }
	}
}

// Resident workgroups per CU of the kernel a launch runs: they depend on (LDS bytes, kernel variant) only, asked once per
// combination; never more than pwn_lds_fit allows
static int resident_per_cu(pwn_ctx *c, bool glb, bool refill, bool has_w, size_t lds_bytes)
{
	const int variant = (glb ? 8 : 0) | (refill ? 4 : 0) | (c->counters_on ? 2 : 0) | (has_w ? 1 : 0);
	if(c->occ_lds[variant] != lds_bytes)
	{
		c->occ_blocks[variant] = refill ? pwn_trace_refill_blocks_per_cu(lds_bytes, c->counters_on != 0, has_w)
		                       : glb ? pwn_trace_global_blocks_per_cu(lds_bytes, c->counters_on != 0, has_w)
		                             : pwn_trace_blocks_per_cu(lds_bytes, c->counters_on != 0, has_w);
		c->occ_lds[variant] = lds_bytes;
	}
	int per_cu = c->occ_blocks[variant];
	const int lds_fit = (int)pwn_lds_fit((uint32_t)lds_bytes);
	if(per_cu > lds_fit) per_cu = lds_fit;
	if(per_cu < 1) per_cu = 1;
	if(c->dbg_blocks_per_cu > 0) per_cu = c->dbg_blocks_per_cu;                                      // experiments
	return per_cu;
}

// the upload of the tables (copy `cur`) runs on its own stream: a launch on `stream` comes after it
int pwn_i_tables_uploaded(pwn_ctx *c, int cur, hipStream_t stream)
{
	if(!c->upload_pending[cur]) return PWN_OK;
	if(hipEventQuery(c->ev_upload[cur]) == hipSuccess) c->upload_pending[cur] = false;
	else HIPCHK(c, hipStreamWaitEvent(stream, c->ev_upload[cur], 0));
	return PWN_OK;
}

// PWN_OPT_WAVE_LOG: every wave of a launch of `grid` workgroups writes its start and end time; entry 0 is unused, entry
// 1 + 4 * workgroup + SIMD is a wave's (the buffer follows the grid of the launch)
static int wave_log_for_launch(pwn_ctx *c, int grid, hipStream_t stream, pwn_trace_params *P)
{
	const size_t entries = (size_t)grid * 4 + 1;
	if(entries > c->wave_log_cap)
	{
		// (a kernel of an earlier launch that writes the old buffer may be on either compute stream)
		if(c->d_wave_log) { HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(c->d_wave_log); c->d_wave_log = NULL; c->wave_log_cap = 0; }
		HIPCHK(c, hipMalloc((void **)&c->d_wave_log, entries * 16));
		c->wave_log_cap = entries;
	}
	HIPCHK(c, hipMemsetAsync(c->d_wave_log, 0, c->wave_log_cap * 16, stream));
	P->wave_log = c->d_wave_log;
	return PWN_OK;
}

// PWN_OPT_UNIT_ORDER (and the wave log, for tools/unit_order_sim.py): this launch writes what every unit cost its wave,
// and hands its units out in the order sorted from the last launch of the same rows on this stream
// (with the wave log only where the dump is asked for, PWN_DBG_UNIT_COST: the kernel variant that writes the costs is 2-3 % slower,
// and the wave log's span and residency are figures of the ordinary launch)
// (a batch of views or rays neither writes nor reads nor invalidates any of this)
// (nor do tables in the global form: their kernels have no ordered variant, PWN_OPT_UNIT_ORDER is ignored)
static int unit_order_for_launch(pwn_ctx *c, hipStream_t stream, bool batch, bool want_cost, pwn_trace_params *P)
{
	pwn_ctx::unit_order_state *uop = batch ? NULL : order_entry(c, stream, want_cost);
	if(uop != NULL && want_cost)
	{
		pwn_ctx::unit_order_state &uo = *uop;
		const int y0 = P->y0, y1 = P->y1;
		const size_t units = (size_t)P->tiles_total;
		const uint32_t qcap = (uint32_t)((units + PWN_QUEUES - 1u) / PWN_QUEUES);
		if(units > uo.cost_cap || (size_t)qcap * PWN_QUEUES > uo.perm_cap)
		{
			// (kernels that use the old buffers may still run, on either stream)
			if(uo.d_cost || uo.d_perm) HIPCHK(c, hipDeviceSynchronize());
			(void)hipFree(uo.d_cost); (void)hipFree(uo.d_perm);
			uo.d_cost = NULL; uo.d_perm = NULL; uo.cost_cap = uo.perm_cap = 0; uo.perm_valid = uo.cost_fresh = false;
			HIPCHK(c, hipMalloc((void **)&uo.d_cost, units * 2));
			HIPCHK(c, hipMalloc((void **)&uo.d_perm, (size_t)qcap * PWN_QUEUES * 4));
			uo.cost_cap = units; uo.perm_cap = (size_t)qcap * PWN_QUEUES;
		}
		P->unit_cost = uo.d_cost;
		if(c->unit_order && uo.perm_valid && uo.perm_units == (uint32_t)units && uo.perm_y0 == y0 && uo.perm_y1 == y1)
		{
			P->perm = uo.d_perm; P->perm_cap = qcap;
			c->order_used++;
		}
		uo.units = (uint32_t)units; uo.qcap = qcap; uo.y0 = y0; uo.y1 = y1; uo.cost_fresh = true;
	}
	else if(uop != NULL) uop->cost_fresh = false;
	return PWN_OK;
}

// A launch clears the ticket set that the launch R before it drew from (pwn_internal.h, launch_stream): it has to come after that
// one.  On one stream and in the rotation over R it does by itself; a launch that leaves the pattern waits.
static int rotation_wait(pwn_ctx *c, hipStream_t stream)
{
	const int rot = c->launch_rot;
	if(c->launch_event[rot - 1] != NULL && c->launch_stream[rot - 1] != stream)
	{
		HIPCHK(c, hipStreamWaitEvent(stream, c->launch_event[rot - 1], 0));
		c->launch_waits++;
	}
	return PWN_OK;
}

// Behind a launch that went out on `stream` and read copy `cur` of the tables: the rotation moves on, and the copy is guarded by
// the caller's event or one recorded here
static int launch_went_out(pwn_ctx *c, int cur, hipStream_t stream, hipEvent_t caller_event)
{
	c->ticket_set++;                     // only a launch that went out has cleared the other set
	c->launch_stream[2] = c->launch_stream[1]; c->launch_event[2] = c->launch_event[1];
	c->launch_stream[1] = c->launch_stream[0]; c->launch_event[1] = c->launch_event[0];
	c->launch_stream[0] = stream; c->launch_event[0] = caller_event != NULL ? caller_event : c->ev_tables[cur];
	if(caller_event != NULL)
	{
		// The caller is about to record this event again.  Its last record was behind a frame the caller has since
		// waited for on the host (a free slot), so a copy of the tables still guarded by that record is not in
		// use any more -- and must stop pointing at the event, or its next upload would wait for THIS frame,
		// the newest one in flight (four copies with three slots did exactly that: 20 us of idle GPU per frame).
		for(int i = 0; i < PWN_NBLOB; i++)
			if(c->tables_in_use[i] && c->tables_wait[i] == caller_event) c->tables_in_use[i] = false;
		c->tables_wait[cur] = caller_event;
	}
	else
	{
		HIPCHK(c, hipEventRecord(c->ev_tables[cur], stream));
		c->tables_wait[cur] = c->ev_tables[cur];
	}
	c->tables_in_use[cur] = true;
	return PWN_OK;
}

int pwn_i_launch_trace(pwn_ctx *c, pwn_trace_launch *L)
{
	const pwn_views_launch *views = L->views.n > 0 ? &L->views : NULL;
	const pwn_rays_launch *rays = L->rays.n > 0 ? &L->rays : NULL;
	const pwn_vps_launch *vps = L->vps.n > 0 ? &L->vps : NULL;
	const bool batch = views != NULL || rays != NULL || vps != NULL;
	// what is traced, once: the plan's kind and the kernel's mode (launch_plan.h)
	// (a launch is one of the three batches at the most)
	pwn_launch_what what = { PWN_LAUNCH_FRAME, false, false, false };
	if(views != NULL) what = { PWN_LAUNCH_VIEWS, views->d_label != NULL, views->hide, false };
	if(vps != NULL) what = { PWN_LAUNCH_VIEWPORTS, vps->d_label != NULL, vps->hide, false };
	if(rays != NULL) what = { PWN_LAUNCH_RAYS, rays->d_hits != NULL, rays->d_hide != NULL, rays->d_reach != NULL };
	const int mode = pwn_launch_mode(what);
	const int y0 = L->y0, y1 = L->y1;
	const hipStream_t stream = L->stream;
	L->cost_mul = L->cost_div = 1u;
	if(!c->have_level) return PWN_ENOLEVEL;
	if(c->blob_dirty) { int rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	if(y1 == y0 && rays == NULL) return PWN_OK;

	// the parameters: what is traced and where to ...
	pwn_trace_params P;
	memset(&P, 0, sizeof(P));
	// (a batch has every view's camera set-up and time in its record, every ray's origin and direction in its own)
	if(!batch) frame_setup(c->w, c->h, L->cam, &P);
	P.sec_current = L->sec;
	// (views of their own sizes in planes of the caller's, pwn_trace_viewports_device: the planes' size, not the context's)
	const int fw = vps != NULL && vps->fw > 0 ? vps->fw : c->w, fh = vps != NULL && vps->fh > 0 ? vps->fh : c->h;
	P.w = fw; P.h = fh; P.y0 = y0; P.y1 = y1;
	if(views != NULL)
	{
		P.views = views->d_recs; P.nviews = views->n; P.plane = views->plane;
		P.hits = views->d_label;        // (first-hit planes, pwn_trace_view_hits: the label plane; d_sbuf is then the cell plane, d_zbuf the distance plane)
		P.view_hide = views->hide ? 1 : 0;
	}
	if(vps != NULL)
	{
		P.vps = vps->d_recs; P.nvp = vps->n;
		P.hits = vps->d_label;          // (first-hit planes, pwn_trace_viewport_hits: the label plane; d_sbuf is then the cell plane, d_zbuf the distance plane)
		P.view_hide = vps->hide ? 1 : 0;
	}
	if(rays != NULL)
	{
		P.rays = rays->d_rays; P.ray_seeds = rays->d_seeds; P.nrays = rays->n; P.ray_w = rays->has_w ? 1 : 0;
		P.hits = rays->d_hits;
		P.ray_hide = rays->d_hide;
		P.ray_reach = rays->d_reach;
	}
	P.sbuf = L->d_sbuf; P.zbuf = L->d_zbuf;
	P.counters = c->d_counters;
	P.clear_word = L->clear_word;
	P.cost_word = L->cost_word;
	// ... from which tables ...
	const int cur = c->blob_cur;
	const bool glb = c->lists_form == PWN_LF_GLOBAL;
	params_tables(c, cur, &P);
	// ... the kernel's work queues: this launch's set and the one it clears (the rotation over 2R sets: pwn_internal.h, launch_stream) ...
	const unsigned rot = (unsigned)c->launch_rot, nsets = 2u * rot;
	P.tickets = c->d_tickets + (c->ticket_set % nsets) * PWN_QUEUES * PWN_QUEUE_STRIDE;
	P.tickets_next = c->d_tickets + ((c->ticket_set + rot) % nsets) * PWN_QUEUES * PWN_QUEUE_STRIDE;
	// ... and the kernel variant: the 3-lane or the 4-lane one (camera_has_w)
	if(views != NULL) P.has_w = views->has_w;        // (the same rule over all the batch's cameras)
	else if(rays != NULL) P.has_w = rays->has_w;     // (the rule over the batch's rays: pwn_trace_rays)
	else if(vps != NULL) P.has_w = vps->has_w;
	else P.has_w = camera_has_w(L->cam);
	// test hook (tests/test_gpu_fuzz.py): send every camera through the general variant
	if(c->dbg_force_hasw) P.has_w = 1;
	// (a batch of views or rays always runs the units scheduler)
	// (so do tables in the global form: the refill kernel has none)
	const bool refill = c->scheduler == PWN_SCHED_REFILL && !batch && !glb;
	const size_t lds_bytes = ((P.blob_bytes + 15u) & ~15u) + (refill ? pwn_trace_refill_lds_extra(P.has_w != 0) : pwn_trace_lds_extra());
	P.scheduler = c->scheduler;
	P.refill_limit = c->refill_limit;

	// the geometry (launch_plan.h): the units, how they are handed out, the grid
	pwn_launch_shape S = { .w = fw, .y0 = y0, .y1 = y1, .tile_w = pwn_trace_tile_w(), .tile_h = pwn_trace_tile_h() };
	S.kind = what.kind;
	if(views != NULL) S.n = (uint32_t)views->n;
	if(vps != NULL) { S.n = (uint32_t)vps->n; S.vp_units = vps->units; }
	if(rays != NULL) S.n = rays->n;
	S.resident = c->num_cus * resident_per_cu(c, glb, refill, P.has_w != 0, lds_bytes);
	const int room = c->room.mode >= 0 ? c->room.mode : L->room;        // (a host that set a number gets it for every launch)
	S.reserve = c->grid_reserve > room ? c->grid_reserve : room;
	S.refill = refill;
	// (what the unit order needs: a launch with an order keeps single units)
	S.want_cost = !refill && !batch && !glb && (c->unit_order || (c->wave_log_on && getenv("PWN_DBG_UNIT_COST") != NULL));
	S.tile_pairs = c->tile_pairs;
	pwn_launch_plan plan;
	if(pwn_launch_plan_make(S, &plan) != 0) { snprintf(c->err, sizeof(c->err), "no division constant for %d units per row", plan.tiles_x); return PWN_EINVAL; }
	P.tiles_x = plan.tiles_x; P.tiles_total = plan.tiles_total; P.ux_magic = plan.ux_magic; P.ux_shift = plan.ux_shift;
	P.views_magic = plan.views_magic; P.views_shift = plan.views_shift; P.vp_step0 = plan.vp_step0;
	P.tile_pairs = plan.tile_pairs; P.pair_single_rows = plan.pair_single_rows; P.tx_magic = plan.tx_magic; P.tx_shift = plan.tx_shift;

	// from here on the runtime is talked to, in the order tests/golden/host_calls.txt records
	int rc = pwn_i_tables_uploaded(c, cur, stream);
	if(rc != PWN_OK) return rc;
	if(c->counters_on) HIPCHK(c, hipMemsetAsync(c->d_counters, 0, PWN_NCOUNTERS * sizeof(unsigned long long), stream));
	L->cost_mul = plan.cost_mul; L->cost_div = plan.cost_div;
	if(c->wave_log_on && !batch) { rc = wave_log_for_launch(c, plan.grid, stream, &P); if(rc != PWN_OK) return rc; }
	rc = unit_order_for_launch(c, stream, batch, S.want_cost, &P);
	if(rc != PWN_OK) return rc;
	rc = rotation_wait(c, stream);
	if(rc != PWN_OK) return rc;
	if(refill) HIPCHK(c, pwn_launch_trace_refill(&P, plan.grid, lds_bytes, c->counters_on != 0, stream));
	else
	{
		// the units kernel's variant (trace_variants.h): the mode, the form of the tables' per-cell lists (pwn_i_pack_blob says which the
		// blob has), and whether the launch reads an order or writes its units' costs.  A combination without a kernel is refused there.
		const int lists = glb ? PWN_LF_GLOBAL : P.off_recsph != 0u ? PWN_LF_INLINE : PWN_LF_INDEXED;
		const bool order = P.perm != NULL || P.unit_cost != NULL;
		HIPCHK(c, pwn_launch_trace(mode, lists, order, &P, plan.grid, lds_bytes, c->counters_on != 0, stream));
	}
	return launch_went_out(c, cur, stream, L->tables_event);
}

// Behind the last kernel of a frame on `stream`: the costs its trace launch wrote become the hand-out order of the next
// launch of the same rows on that stream.  ~10 us of 64 workgroups at 4K, which the caller puts where nobody waits for
// it (behind the frame's "done" event / its copies to the host).
int pwn_i_launch_order(pwn_ctx *c, hipStream_t stream)
{
	pwn_ctx::unit_order_state *uop = order_entry(c, stream, false);
	if(uop == NULL) return PWN_OK;
	pwn_ctx::unit_order_state &uo = *uop;
	if(!c->unit_order || !uo.cost_fresh || uo.units < 4u * PWN_QUEUES) return PWN_OK;
	uo.cost_fresh = false;
	HIPCHK(c, pwn_launch_order(uo.d_cost, uo.units, uo.qcap, uo.d_perm, stream));
	uo.perm_valid = true; uo.perm_units = uo.units; uo.perm_y0 = uo.y0; uo.perm_y1 = uo.y1;
	c->order_sorts++;
	return PWN_OK;
}

// the sort by itself, host arrays in and out (tests): perm_out has 64 * ceil(units / 64) entries, queue q's at [q * cap, q * cap + its length)
extern "C" int pwn_unit_order_probe(pwn_ctx *c, const uint16_t *cost, uint32_t units, uint32_t *perm_out)
{
	if(GRP_HEAD(c)) return pwn_group_on_member0(c, [cost, units, perm_out](pwn_ctx *m0) { return pwn_unit_order_probe(m0, cost, units, perm_out); });
	if(c == NULL || cost == NULL || perm_out == NULL || units == 0u) return PWN_EINVAL;
	const uint32_t cap = (units + PWN_QUEUES - 1u) / PWN_QUEUES;
	(void)hipSetDevice(c->device);
	uint16_t *d_cost = NULL; uint32_t *d_perm = NULL;
	int rc = PWN_OK;
	if(hipMalloc((void **)&d_cost, (size_t)units * 2) != hipSuccess || hipMalloc((void **)&d_perm, (size_t)cap * PWN_QUEUES * 4) != hipSuccess) rc = PWN_ENOMEM;
	if(rc == PWN_OK && (hipMemcpy(d_cost, cost, (size_t)units * 2, hipMemcpyHostToDevice) != hipSuccess ||
	   hipMemset(d_perm, 0xff, (size_t)cap * PWN_QUEUES * 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = PWN_EHIP;
	if(rc == PWN_OK && pwn_launch_order(d_cost, units, cap, d_perm, c->stream) != hipSuccess) rc = PWN_EHIP;
	if(rc == PWN_OK && (hipStreamSynchronize(c->stream) != hipSuccess ||
	   hipMemcpy(perm_out, d_perm, (size_t)cap * PWN_QUEUES * 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = PWN_EHIP;
	(void)hipFree(d_cost); (void)hipFree(d_perm);
	return rc;
}

extern "C" int pwn_launch_order_waits(pwn_ctx *c, unsigned long long *out)
{
	if(GRP_HEAD(c)) return pwn_launch_order_waits(GRP_M0(c), out);
	if(c == NULL || out == NULL) return PWN_EINVAL;
	*out = c->launch_waits;
	return PWN_OK;
}

extern "C" int pwn_unit_order_state(pwn_ctx *c, unsigned long long out[4])
{
	if(GRP_HEAD(c)) return pwn_unit_order_state(GRP_M0(c), out);
	if(c == NULL || out == NULL) return PWN_EINVAL;
	out[0] = (unsigned long long)c->unit_order; out[1] = c->order_used; out[2] = c->order_sorts;
	out[3] = c->order[0].perm_valid ? c->order[0].perm_units : 0ull;
	return PWN_OK;
}

int pwn_i_launch_blur(pwn_ctx *c, const pwn_blur_launch *L)
{
	const pwn_vps_launch *vps = L->vps.n > 0 ? &L->vps : NULL;
	// (views of their own sizes in planes of the caller's, pwn_trace_viewports_device: the planes' size and the layout's skip-ahead table)
	const int fw = vps != NULL && vps->fw > 0 ? vps->fw : c->w, fh = vps != NULL && vps->fh > 0 ? vps->fh : c->h;
	if((fw & 3) != 0) return PWN_EINVAL; // screen.h:88,117: aligned 16-B store per group
	pwn_blur_params B;
	B.views = L->views; B.plane = (unsigned long long)c->w * (unsigned long long)c->h;
	B.vps = vps != NULL ? vps->d_recs : NULL; B.nvp = vps != NULL ? vps->n : 0; B.vp_tiles = 0;
	B.w = fw; B.h = fh; B.y0 = L->y0; B.y1 = L->y1;
	B.groups = fw / 4;
	B.pre = L->d_pre; B.zbuf = L->d_z; B.out = L->d_out; B.skip = vps != NULL && vps->d_skip != NULL ? vps->d_skip : c->d_skip;
	B.avail_y0 = L->avail_y0; B.avail_y1 = L->avail_y1; B.miss = L->d_miss;
	B.cost_acc = L->d_cost_acc; B.cost_out = L->d_cost_out;
	B.cost_mul = L->cost_mul ? L->cost_mul : 1u; B.cost_div = L->cost_div ? L->cost_div : 1u;
	// The workgroup's tile of output pixels (post_kernels.hip), chosen by what the frame rate on two streams said
	// (profiles/r3_blur_sweep.txt): 32 x 32 for wide frames and their strips (256-thread workgroups with 17 KB of LDS find room
	// beside the trace grid's workgroups that a 1024-thread one with 42 KB does not: 4K +1.9 %, 8K +5.3 %, the strips of an
	// 8-way 4K tiling -3.5 % kernel time against the 128 x 32 of rounds 1-2), 128 x 16 for narrow ones (720p +4.8 %, 1080p
	// +3.4 %; 32 x 32 loses 6 % at 720p).  Any shape gives the same pixels.
	{
		// With room beside the trace grid (PWN_OPT_TRACE_ROOM, what level.txt-like scenes settle on) 32 x 32 wins on narrow frames
		// too: 720p 16.4-17.5 -> 19.4 Gpixels/s (profiles/r3_blur_sweep.txt, last block).
		B.tile_w = 32; B.tile_h = 32; B.batch = 1;
		// (views of their own sizes: the widest view decides, as it would on a context of its size)
		int wide = c->w;
		if(vps != NULL) { wide = 0; for(int i = 0; i < vps->n; i++) if(vps->h_recs[i].w > wide) wide = vps->h_recs[i].w; }
		if(wide < 2560 && pwn_room_for_launch(c) == 0) { B.tile_w = 128; B.tile_h = 16; }
		if(c->dbg_blur_th > 0) B.tile_h = c->dbg_blur_th;          // (a shape without an instantiation: the launch fails with hipErrorInvalidValue)
		if(c->dbg_blur_tw > 0) B.tile_w = c->dbg_blur_tw;
		if(c->dbg_blur_batch >= 0) B.batch = c->dbg_blur_batch;
		// ... and the grid is that of the view with the most tiles of this shape
		if(vps != NULL && B.tile_w > 0 && B.tile_h > 0)
			for(int i = 0; i < vps->n; i++)
			{
				const int t = ((vps->h_recs[i].w + B.tile_w - 1) / B.tile_w) * ((vps->h_recs[i].h + B.tile_h - 1) / B.tile_h);
				if(t > B.vp_tiles) B.vp_tiles = t;
			}
	}
	HIPCHK(c, pwn_launch_blur(&B, L->stream));
	return PWN_OK;
}

extern "C" int pwn_trace_rows_device(pwn_ctx *c, const float cam[16], float sec, int y0, int y1,
	void *d_sbuf, void *d_zbuf, void *stream)
{
	GRP_REFUSE(c, "pwn_trace_rows_device");
	if(c == NULL || cam == NULL || d_sbuf == NULL || d_zbuf == NULL || y0 < 0 || y1 > c->h || y0 > y1) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	pwn_trace_launch L = { .cam = cam, .sec = sec, .y0 = y0, .y1 = y1, .d_sbuf = (uint32_t *)d_sbuf, .d_zbuf = (float *)d_zbuf, .stream = (hipStream_t)stream };
	return pwn_i_launch_trace(c, &L);
}

extern "C" int pwn_blur_rows_device(pwn_ctx *c, int y0, int y1, const void *d_pre, const void *d_zbuf, void *d_out, void *stream)
{
	GRP_REFUSE(c, "pwn_blur_rows_device");
	if(c == NULL || d_pre == NULL || d_zbuf == NULL || d_out == NULL || y0 < 0 || y1 > c->h || y0 > y1 || d_pre == d_out) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	const pwn_blur_launch B = { .y0 = y0, .y1 = y1, .d_pre = (const uint32_t *)d_pre, .d_z = (const float *)d_zbuf, .d_out = (uint32_t *)d_out, .stream = (hipStream_t)stream };
	int rc = pwn_i_launch_blur(c, &B);
	// PWN_OPT_UNIT_ORDER: a strip's trace and blur on one stream of the caller's -- the order of that stream's next trace of the same rows
	if(rc == PWN_OK) rc = pwn_i_launch_order(c, (hipStream_t)stream);
	return rc;
}

extern "C" int pwn_blur_rows_device_bounded(pwn_ctx *c, int y0, int y1, const void *d_pre, const void *d_zbuf, void *d_out,
	int avail_y0, int avail_y1, void *d_miss, void *stream)
{
	GRP_REFUSE(c, "pwn_blur_rows_device_bounded");
	if(c == NULL || d_pre == NULL || d_zbuf == NULL || d_out == NULL || d_miss == NULL || y0 < 0 || y1 > c->h || y0 > y1 ||
	   d_pre == d_out || avail_y0 > avail_y1) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	const pwn_blur_launch B = { .y0 = y0, .y1 = y1, .d_pre = (const uint32_t *)d_pre, .d_z = (const float *)d_zbuf, .d_out = (uint32_t *)d_out, .stream = (hipStream_t)stream,
		.avail_y0 = avail_y0, .avail_y1 = avail_y1, .d_miss = (uint32_t *)d_miss };
	int rc = pwn_i_launch_blur(c, &B);
	if(rc == PWN_OK) rc = pwn_i_launch_order(c, (hipStream_t)stream);
	return rc;
}

// The blur passes behind a trace into *cur: each pass is B (its rows, depth, stream and views as given) from the plane that holds
// the frame into the other of the two, which take turns (the memcpy of screen.h:75 becomes a pointer swap per pass); the last pass
// into `last` where one is given.  *cur is left at the plane that holds the result.
int pwn_i_blur_passes_run(pwn_ctx *c, pwn_blur_launch B, uint32_t **cur, uint32_t *other, uint32_t *last)
{
	for(int p = 0; p < c->blur_passes; p++)
	{
		B.d_pre = *cur; B.d_out = (last != NULL && p == c->blur_passes - 1) ? last : other;
		const int rc = pwn_i_launch_blur(c, &B);
		if(rc != PWN_OK) return rc;
		other = *cur; *cur = B.d_out;
	}
	return PWN_OK;
}
