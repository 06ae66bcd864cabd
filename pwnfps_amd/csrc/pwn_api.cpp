// pwn_api.cpp -- the C ABI of libpwnhip.so (include/pwnhip.h) over the HIP runtime: the context and its options, the room
// control, stats, the sink, the probes.  The tables are pwn_tables.cpp's, the launchers pwn_launch.cpp's, the blocking and batch
// calls pwn_calls.cpp's, the frames in flight pwn_frames.cpp's (pwn_internal.h has the map).
// Host code only, as all of these; compiled with -ffp-contract=off because the camera set-up
// of screen.h:43-57 is part of the bit-exact path.
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <new>
#include "pwn_internal.h"
#include "level_host.h"

extern "C" const char *pwn_strerror(int code)
{
	switch(code)
	{
		case PWN_OK: return "ok";
		case PWN_EINVAL: return "invalid argument";
		case PWN_ENODEV: return "no usable HIP device";
		case PWN_ENOMEM: return "out of memory";
		case PWN_EIO: return "level file could not be read";
		case PWN_EHIP: return "HIP runtime error";
		case PWN_ENOLEVEL: return "no level uploaded";
		case PWN_ETOOBIG: return "sphere tables exceed PWN_TABLES_MAX";
		case PWN_EBUSY: return "frame slot still in flight";
		case PWN_ENOTSUP: return "not available (RCCL missing, or not configured)";
		case PWN_ETIMEDOUT: return "the row tiling's deadline passed waiting for a peer";
	}
	return "unknown error";
}

extern "C" const char *pwn_last_error(pwn_ctx *ctx) { return ctx ? ctx->err : "null context"; }

static int ensure_scratch(pwn_ctx *c, size_t bytes)
{
	if(bytes <= c->scratch_cap) return PWN_OK;
	if(c->d_scratch) { (void)hipFree(c->d_scratch); c->d_scratch = NULL; c->scratch_cap = 0; }
	HIPCHK(c, hipMalloc((void **)&c->d_scratch, bytes));
	c->scratch_cap = bytes;
	return PWN_OK;
}

extern "C" int pwn_init(pwn_ctx **out, int device, int width, int height)
{
	if(out == NULL || width <= 0 || height <= 0 || width > 32768 || height > 32768) return PWN_EINVAL;
	*out = NULL;
	int ndev = 0;
	if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PWN_ENODEV;
	pwn_ctx *c = new(std::nothrow) pwn_ctx();
	if(c == NULL) return PWN_ENOMEM;
	c->device = device; c->w = width; c->h = height;
	c->blur_passes = 1; c->counters_on = 0; c->scheduler = PWN_SCHED_DEFAULT; c->refill_limit = PWN_REFILL_LIMIT_DEFAULT; c->have_level = false; c->cell_base_ok = false;
	// experiments and the test suite pick the trace scheduler for every context of a process
	if(const char *e = getenv("PWN_SCHEDULER")) c->scheduler = (strcmp(e, "refill") == 0 || strcmp(e, "1") == 0) ? PWN_SCHED_REFILL : PWN_SCHED_UNITS;
	if(const char *e = getenv("PWN_REFILL_LIMIT")) { int v = atoi(e); if(v >= 1 && v <= 64000) c->refill_limit = v; }
	// test / experiment hooks, read once: every camera through the general 4-lane variant (tests/test_gpu_fuzz.py);
	// workgroups per CU of the persistent grid
	c->dbg_force_hasw = getenv("PWN_DBG_FORCE_HASW") != NULL;
	c->dbg_blocks_per_cu = 0;
	c->dbg_blur_th = 0;
	if(const char *e = getenv("PWN_DBG_BLUR_TH")) c->dbg_blur_th = atoi(e);
	c->dbg_sphere_lists = 0; c->off_recsph = 0;
	c->dbg_sphere_lists = pwn_i_forced_lists();
	c->nbounds = 0;
	{ const char *e = getenv("PWN_SPHERE_BOUNDS"); c->dbg_sphere_bounds = (e != NULL && strcmp(e, "0") == 0) ? 0 : 1; }
	c->lists_form = PWN_LF_INDEXED; c->big_which = c->big_sph = 0; c->big_high = 0;
	for(int i = 0; i < PWN_NBLOB; i++) { c->d_big[i] = NULL; c->d_big_cap[i] = 0; }
	for(int i = 0; i < PWN_NSTAGE; i++) { c->h_big[i] = NULL; c->h_big_cap[i] = 0; }
	c->dbg_blur_tw = 0; c->dbg_blur_batch = -1;          // (sweeps with a -DPWN_BLUR_SWEEP build: tools/r3/run_w.sh)
	if(const char *e = getenv("PWN_DBG_BLUR_TW")) c->dbg_blur_tw = atoi(e);
	if(const char *e = getenv("PWN_DBG_BLUR_BATCH")) if(*e) c->dbg_blur_batch = atoi(e);
	if(const char *e = getenv("PWN_DBG_BLOCKS_PER_CU")) { int v = atoi(e); if(v > 0) c->dbg_blocks_per_cu = v; }
	// tile pairs (trace_kernel.hip): 0 never, 1 (default) in the launches that would draw their tickets two at a time, 2 always
	c->tile_pairs = 1;
	if(const char *e = getenv("PWN_TILE_PAIRS")) if(*e) { const int v = atoi(e); if(v >= 0 && v <= 2) c->tile_pairs = v; }
	c->blob_cur = 0; c->blob_dirty = true; c->off_sph = 0; c->stage_next = 0; c->up_stream = NULL;
	for(int i = 0; i < PWN_NBLOB; i++)
	{
		c->d_blob[i] = NULL; c->blob_has_static[i] = false;
		c->ev_tables[i] = NULL; c->tables_in_use[i] = false; c->tables_wait[i] = NULL;
		c->ev_upload[i] = NULL; c->upload_pending[i] = false;
	}
	for(int i = 0; i < PWN_NSTAGE; i++) { c->h_stage[i] = NULL; c->ev_stage[i] = NULL; c->stage_used[i] = false; }
	c->d_pre = c->d_out = NULL; c->d_z = NULL; c->d_skip = NULL; c->d_counters = NULL; c->d_tickets = NULL; c->ticket_set = 0; c->launch_rot = 2; c->launch_waits = 0;
	c->grid_reserve = 0;
	c->d_vpre = c->d_vout = NULL; c->d_vz = NULL; c->views_cap = 0; c->h_vrec = c->d_vrec = NULL; c->d_vrec_dev = NULL;
	c->d_ppre = c->d_pout = NULL; c->d_pz = NULL; c->h_prec = c->d_prec = NULL; c->d_prec_dev = NULL;
	c->h_rays = c->d_rays = NULL; c->rays_cap = 0;
	c->h_hits = c->d_hits = NULL; c->hits_cap = 0;
	c->h_players = c->d_players = NULL; c->players_cap = 0; c->dbg_players_stage = -1;
	if(const char *e = getenv("PWN_PLAYERS_STAGE")) if(*e) c->dbg_players_stage = atoi(e) != 0;      // (A/B of the step's LDS staging: tools/players_bench.py)
	for(int i = 0; i < PWN_NBLOB; i++) { c->d_walk[i] = NULL; c->walk_of[i] = i; c->ev_walk[i] = NULL; c->walk_in_use[i] = false; c->walk_stream[i] = NULL; }
	for(int i = 0; i < PWN_NSTAGE; i++) c->h_walk[i] = NULL;
	c->walk_dirty = false;
	memset(&c->sd, 0, sizeof(c->sd));
	memset(&c->ld, 0, sizeof(c->ld));
	memset(&c->room, 0, sizeof(c->room)); c->room.mode = -1;
	if(const char *e = getenv("PWN_TRACE_ROOM")) if(*e) c->room.mode = atoi(e) < 0 ? -1 : atoi(e);      // (the option's default for every context of a process)
	c->d_scratch = NULL; c->scratch_cap = 0;
	for(int i = 0; i < 12; i++) { c->occ_lds[i] = 0; c->occ_blocks[i] = 0; }
	c->stream = NULL; c->copy_stream = NULL; c->copy_stream2 = NULL; c->stream2 = NULL; c->d_pre2 = NULL;
	c->frame_overlap = 1; c->last_frame_done = NULL; c->last_frame_stream = NULL;
	if(const char *e = getenv("PWN_FRAME_OVERLAP")) c->frame_overlap = atoi(e) != 0;
	c->unit_order = 0;             // (measured: a loss except on short launches that run alone, profiles/r4/unit_order_ab.txt)
	if(const char *e = getenv("PWN_UNIT_ORDER")) c->unit_order = atoi(e) != 0;
	c->tiled_comms = PWN_TILED_COMMS_ONE;
	if(const char *e = getenv("PWN_TILED_COMMS")) c->tiled_comms = (strcmp(e, "perstream") == 0 || strcmp(e, "2") == 0) ? PWN_TILED_COMMS_PER_STREAM : PWN_TILED_COMMS_ONE;
	c->tiled_streams = PWN_TILED_STREAMS_DEFAULT;
	if(const char *e = getenv("PWN_TILED_STREAMS")) { const int v = atoi(e); if(v == 2 || v == 3) c->tiled_streams = v; }
	c->tiled_choreo = PWN_TILED_CHOREO_INSTREAM;
	if(const char *e = getenv("PWN_TILED_CHOREO")) c->tiled_choreo = (strcmp(e, "split") == 0 || strcmp(e, "1") == 0) ? PWN_TILED_CHOREO_SPLIT : PWN_TILED_CHOREO_INSTREAM;
	memset(c->ev, 0, sizeof(c->ev));
	memset(&c->stats, 0, sizeof(c->stats));
	c->strip_reach = 0;
	c->call_strips = -1; c->strip_ev_n = 0; c->d_strip_miss = NULL; c->h_strip_miss = NULL; c->strip_backoff = 0;
	c->strip_calls = c->strip_redone = 0; c->strips_last = 1; c->host_regs_n = 0;
	memset(c->strip_ev, 0, sizeof(c->strip_ev));
	c->strip_copy_streams = 0; c->strip_calib_n = 0;
	if(const char *e = getenv("PWN_CALL_COPY_STREAMS")) if(atoi(e) == 1 || atoi(e) == 2) c->strip_copy_streams = atoi(e);
	if(const char *e = getenv("PWN_CALL_STRIPS")) if(*e) { const int v = atoi(e); if(v >= -1 && v <= PWN_CALL_STRIPS_MAX && v != 1) c->call_strips = v; }
	c->frame_timing = 1; c->wave_log_on = 0; c->d_wave_log = NULL; c->wave_log_cap = 0;
	c->nslots = 0; c->frame_flags = 0; c->frame_scale = 1; c->frame_pitch = 0; c->frame_seq = 0;
	memset(c->slot, 0, sizeof(c->slot));
	c->tiled = NULL; c->grp = NULL; c->grp_head = false; c->hub = NULL;
	c->err[0] = 0;
	pwn_level_clear(c->cells, c->pmap, c->spawn);
	c->bin_off.assign(4097, 0);
	pwn_i_expand_tables(c->tabs, c->tabs + 2048);

	int rc = PWN_OK;
	do
	{
		hipDeviceProp_t prop;
		if(hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) { rc = PWN_ENODEV; break; }
		if(strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		{
			snprintf(c->err, sizeof(c->err), "device %d is %s; libpwnhip is built for gfx950 only", device, prop.gcnArchName);
			rc = PWN_ENODEV; break;
		}
		c->num_cus = prop.multiProcessorCount;
		size_t n = (size_t)width * (size_t)height;
		if(hipMalloc((void **)&c->d_pre, n * 4) != hipSuccess ||
		   hipMalloc((void **)&c->d_out, n * 4) != hipSuccess ||
		   hipMalloc((void **)&c->d_z, n * 4) != hipSuccess ||
		   hipMalloc((void **)&c->d_counters, PWN_NCOUNTERS * sizeof(unsigned long long)) != hipSuccess ||
		   hipMalloc((void **)&c->d_tickets, PWN_TICKET_SETS * PWN_QUEUES * PWN_QUEUE_STRIDE * sizeof(uint32_t)) != hipSuccess ||
		   hipMemset(c->d_tickets, 0, PWN_TICKET_SETS * PWN_QUEUES * PWN_QUEUE_STRIDE * sizeof(uint32_t)) != hipSuccess ||
		   hipMalloc((void **)&c->d_skip, sizeof(uint2) * (size_t)(width / 4 + 1)) != hipSuccess) { rc = PWN_ENOMEM; break; }
		for(int i = 0; i < PWN_NBLOB && rc == PWN_OK; i++)
			if(hipMalloc((void **)&c->d_blob[i], PWN_BLOB_MAX) != hipSuccess) rc = PWN_ENOMEM;
		for(int i = 0; i < PWN_NSTAGE && rc == PWN_OK; i++)
			if(hipHostMalloc((void **)&c->h_stage[i], PWN_BLOB_MAX, hipHostMallocDefault) != hipSuccess) rc = PWN_ENOMEM;
		// the walk tables of the players' step beside them (pwn_internal.h d_walk)
		for(int i = 0; i < PWN_NBLOB && rc == PWN_OK; i++)
			if(hipMalloc((void **)&c->d_walk[i], sizeof(pwn_walk_table)) != hipSuccess) rc = PWN_ENOMEM;
		for(int i = 0; i < PWN_NSTAGE && rc == PWN_OK; i++)
			if(hipHostMalloc((void **)&c->h_walk[i], sizeof(pwn_walk_table), hipHostMallocDefault) != hipSuccess) rc = PWN_ENOMEM;
		if(rc != PWN_OK) break;
		if(hipMemset(c->d_z, 0, n * 4) != hipSuccess || hipMemset(c->d_pre, 0, n * 4) != hipSuccess ||
		   hipMemset(c->d_out, 0, n * 4) != hipSuccess) { rc = PWN_EHIP; break; }
		if(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
		   hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
		   hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess) { rc = PWN_EHIP; break; }
		// The second compute stream has to sit on another HARDWARE queue than the first, or the two only take turns.
		// The runtime hands its hardware queues (four per priority level by default, GPU_MAX_HW_QUEUES) to streams as
		// they are first used, and with PyTorch's streams, the copy and the upload stream in the same process the two
		// compute streams of a context landed on the same one: frames "on two streams" measured exactly like frames
		// on one (0.0823 / 0.0823 ms at 3840 x 272; 0.0823 / 0.0655 with GPU_MAX_HW_QUEUES=8).  Queues are pooled per
		// priority, so a stream of another priority level is certain to have a queue of its own.
		{
			int least = 0, greatest = 0;
			(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
			int prio = greatest < 0 ? greatest : -1;          // (numerically lower = more urgent; 0 is the default level)
			if(const char *e = getenv("PWN_DBG_STREAM2_PRIORITY")) if(*e) prio = atoi(e);
			if(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio) != hipSuccess)
			{
				// (a runtime without stream priorities: an ordinary stream -- the frames then overlap only if it happens
				// to get a hardware queue of its own)
				(void)hipGetLastError();
				if(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) { rc = PWN_EHIP; break; }
			}
		}
		for(int i = 0; i < 4; i++) if(hipEventCreate(&c->ev[i]) != hipSuccess) { rc = PWN_EHIP; break; }
		for(int i = 0; i < PWN_NBLOB && rc == PWN_OK; i++)
			if(hipEventCreateWithFlags(&c->ev_tables[i], hipEventDisableTiming) != hipSuccess ||
			   hipEventCreateWithFlags(&c->ev_upload[i], hipEventDisableTiming) != hipSuccess ||
			   hipEventCreateWithFlags(&c->ev_walk[i], hipEventDisableTiming) != hipSuccess) rc = PWN_EHIP;
		for(int i = 0; i < PWN_NSTAGE && rc == PWN_OK; i++)
			if(hipEventCreateWithFlags(&c->ev_stage[i], hipEventDisableTiming) != hipSuccess) rc = PWN_EHIP;
		if(rc != PWN_OK) break;

		// blur LCG skip-ahead: entry g maps the row seed to the seed in front
		// of group g, i.e. 32*g draws later (screen.h:82,95-109; util.h:1-6)
		std::vector<uint2> skip((size_t)(width / 4 + 1));
		uint32_t A = 1, C = 0;
		for(size_t g = 0; g < skip.size(); g++)
		{
			skip[g].x = A; skip[g].y = C;
			for(int k = 0; k < 32; k++) { A = (A * 25739u) & 0x7FFFFFFFu; C = (C * 25739u + 4u) & 0x7FFFFFFFu; }
		}
		if(hipMemcpy(c->d_skip, skip.data(), skip.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess) { rc = PWN_EHIP; break; }
		// (the memsets above ran on the null stream; the context's streams are non-blocking and do not wait for it)
		if(hipDeviceSynchronize() != hipSuccess) { rc = PWN_EHIP; break; }
	} while(0);

	if(rc != PWN_OK) { pwn_destroy(c); return rc; }
	*out = c;
	return PWN_OK;
}

extern "C" void pwn_destroy(pwn_ctx *c)
{
	if(GRP_HEAD(c)) { pwn_group_destroy(c); return; }
	if(c == NULL) return;
	(void)hipSetDevice(c->device);
	if(c->tiled) pwn_tiled_destroy(c);
	if(c->stream) (void)hipStreamSynchronize(c->stream);
	if(c->stream2) (void)hipStreamSynchronize(c->stream2);
	if(c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
	if(c->up_stream) (void)hipStreamSynchronize(c->up_stream);
	(void)hipDeviceSynchronize();        // strip forms run on the caller's streams
	pwn_i_frames_release(c);
	for(int i = 0; i < 4; i++) if(c->ev[i]) (void)hipEventDestroy(c->ev[i]);
	for(int i = 0; i < c->strip_ev_n; i++) if(c->strip_ev[i]) (void)hipEventDestroy(c->strip_ev[i]);
	(void)hipFree(c->d_strip_miss);
	if(c->h_strip_miss) (void)hipHostFree(c->h_strip_miss);
	for(int i = 0; i < c->host_regs_n; i++) (void)hipHostUnregister(c->host_regs[i].base);
	for(int i = 0; i < PWN_NBLOB; i++)
	{
		if(c->ev_tables[i]) (void)hipEventDestroy(c->ev_tables[i]);
		if(c->ev_upload[i]) (void)hipEventDestroy(c->ev_upload[i]);
		if(c->ev_walk[i]) (void)hipEventDestroy(c->ev_walk[i]);
		(void)hipFree(c->d_walk[i]);
		(void)hipFree(c->d_blob[i]);
		(void)hipFree(c->d_big[i]);
	}
	pwn_i_spheres_device_release(c);
	pwn_i_level_device_release(c);
	pwn_i_viewports_device_release(c);
	for(int i = 0; i < PWN_NSTAGE; i++)
	{
		if(c->ev_stage[i]) (void)hipEventDestroy(c->ev_stage[i]);
		if(c->h_stage[i]) (void)hipHostFree(c->h_stage[i]);
		if(c->h_big[i]) (void)hipHostFree(c->h_big[i]);
		if(c->h_walk[i]) (void)hipHostFree(c->h_walk[i]);
	}
	if(c->stream) (void)hipStreamDestroy(c->stream);
	if(c->stream2) (void)hipStreamDestroy(c->stream2);
	if(c->copy_stream2) { (void)hipStreamSynchronize(c->copy_stream2); (void)hipStreamDestroy(c->copy_stream2); }
	if(c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
	if(c->up_stream) (void)hipStreamDestroy(c->up_stream);
	(void)hipFree(c->d_pre); (void)hipFree(c->d_out); (void)hipFree(c->d_z); (void)hipFree(c->d_pre2);
	(void)hipFree(c->d_wave_log);
	(void)hipFree(c->d_vpre); (void)hipFree(c->d_vout); (void)hipFree(c->d_vz); (void)hipFree(c->d_vrec); (void)hipFree(c->d_vrec_dev);
	if(c->h_vrec) (void)hipHostFree(c->h_vrec);
	(void)hipFree(c->d_ppre); (void)hipFree(c->d_pout); (void)hipFree(c->d_pz); (void)hipFree(c->d_prec);
	if(c->h_prec) (void)hipHostFree(c->h_prec);
	(void)hipFree(c->d_rays);
	if(c->h_rays) (void)hipHostFree(c->h_rays);
	(void)hipFree(c->d_hits);
	if(c->h_hits) (void)hipHostFree(c->h_hits);
	(void)hipFree(c->d_players);
	if(c->h_players) (void)hipHostFree(c->h_players);
	for(int i = 0; i < 4; i++) { (void)hipFree(c->order[i].d_cost); (void)hipFree(c->order[i].d_perm); }
	(void)hipFree(c->d_skip); (void)hipFree(c->d_counters); (void)hipFree(c->d_tickets); (void)hipFree(c->d_scratch);
	delete c;
}

// ---- PWN_OPT_TRACE_ROOM (pwn_internal.h) ----
#define ROOM_WINDOW 24        // delivered frames timed per setting
#define ROOM_SKIP 6           // ... after this many that are not (frames in flight were launched with the old setting)
#define ROOM_HOLD 480         // frames the better setting is kept before the next look
int pwn_room_for_launch(pwn_ctx *c)
{
	if(c->room.mode >= 0) return c->room.mode;
	return c->room.arm ? c->num_cus : 0;
}

void pwn_room_frame_done(pwn_ctx *c)
{
	pwn_room_ctl &r = c->room;
	if(r.mode >= 0) return;
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	const double now = (double)ts.tv_sec + (double)ts.tv_nsec * 1e-9, dt = now - r.t_prev;
	const bool first = r.t_prev == 0.0;
	r.t_prev = now;
	if(first) { r.skip = ROOM_SKIP; return; }
	if(r.hold > 0) { if(r.hold > 1) r.hold--; else if(now - r.t_hold > 0.5) { r.hold = 0; r.arm = 1 - r.best; r.skip = ROOM_SKIP; r.sum[0] = r.sum[1] = 0.0; r.cnt[0] = r.cnt[1] = 0; r.switches++; } return; }
	if(r.skip > 0) { r.skip--; return; }
	// (a host that stops between frames -- a debugger, a vsync -- is not the GPU's time: intervals far above the window's mean are left out)
	if(r.cnt[r.arm] >= 4 && dt > 4.0 * r.sum[r.arm] / r.cnt[r.arm]) return;
	r.sum[r.arm] += dt; r.cnt[r.arm]++;
	if(r.cnt[r.arm] < ROOM_WINDOW) return;
	if(r.cnt[1 - r.arm] < ROOM_WINDOW) { r.arm = 1 - r.arm; r.skip = ROOM_SKIP; r.switches++; return; }
	// both windows are in: the better one (the one in use stays on a tie within 0.5 %)
	const double m0 = r.sum[0] / r.cnt[0], m1 = r.sum[1] / r.cnt[1];
	int best = m1 < m0 ? 1 : 0;
	if(r.looks > 0 && best != r.best && (best ? m1 > 0.995 * m0 : m0 > 0.995 * m1)) best = r.best;
	if(best != r.arm) { r.skip = ROOM_SKIP; r.switches++; }
	r.best = best; r.arm = best; r.hold = ROOM_HOLD; r.t_hold = now; r.looks++;       // (kept for ROOM_HOLD frames and at least half a second)
}

extern "C" int pwn_trace_room_state(pwn_ctx *c, int out[4])
{
	if(GRP_HEAD(c)) return pwn_trace_room_state(GRP_M0(c), out);
	if(c == NULL || out == NULL) return PWN_EINVAL;
	out[0] = c->room.mode; out[1] = pwn_room_for_launch(c); out[2] = (int)c->room.looks; out[3] = (int)c->room.switches;
	return PWN_OK;
}

extern "C" int pwn_set_option(pwn_ctx *c, int option, int value)
{
	if(GRP_HEAD(c)) return pwn_group_set_option(c, option, value);
	if(c == NULL) return PWN_EINVAL;
	switch(option)
	{
		case PWN_OPT_BLUR_PASSES:
			if(value < 0 || value > 16) return PWN_EINVAL;
			// the row tiling fixed its halo, planes and choreography on this at pwn_tiled_init; frames in flight were
			// enqueued with it
			if(c->tiled != NULL) return PWN_EBUSY;
			for(int i = 0; i < c->nslots; i++) if(c->slot[i].in_flight) return PWN_EBUSY;
			c->blur_passes = value; return PWN_OK;
		case PWN_OPT_COUNTERS: c->counters_on = value ? 1 : 0; return PWN_OK;
		case PWN_OPT_SCHEDULER:
			if(value < 0 || value > PWN_SCHED_REFILL) return PWN_EINVAL;
			// (the form of the per-cell sphere lists goes with the scheduler: pwn_i_pack_blob -- but tables built on the device stay in
			// force and in their form, which runs the units kernel under any scheduler: nothing is repacked from the host's spheres)
			if(value != c->scheduler && !c->sd.in_force) c->blob_dirty = true;
			c->scheduler = value; return PWN_OK;
		case PWN_OPT_WAVE_LOG: c->wave_log_on = value ? 1 : 0; return PWN_OK;
		case PWN_OPT_FRAME_TIMING: if(value < 0) return PWN_EINVAL; c->frame_timing = value; return PWN_OK;
		case PWN_OPT_REFILL_LIMIT: if(value < 1 || value > 64000) return PWN_EINVAL; c->refill_limit = value; return PWN_OK;
		case PWN_OPT_UNIT_ORDER: if(value != 0 && value != 1) return PWN_EINVAL; c->unit_order = value; for(int i = 0; i < 4; i++) c->order[i].perm_valid = false; return PWN_OK;
		case PWN_OPT_TILED_CHOREO:
			if(value != PWN_TILED_CHOREO_INSTREAM && value != PWN_TILED_CHOREO_SPLIT) return PWN_EINVAL;
			if(c->tiled != NULL) return PWN_EBUSY;
			c->tiled_choreo = value; return PWN_OK;
		case PWN_OPT_TILED_COMMS:
			if(value != PWN_TILED_COMMS_ONE && value != PWN_TILED_COMMS_PER_STREAM) return PWN_EINVAL;
			if(c->tiled != NULL) return PWN_EBUSY;
			c->tiled_comms = value; return PWN_OK;
		case PWN_OPT_TILED_STREAMS:
			if(value != 2 && value != 3) return PWN_EINVAL;
			if(c->tiled != NULL) return PWN_EBUSY;
			c->tiled_streams = value; return PWN_OK;
		case PWN_OPT_TRACE_ROOM: if(value < -1 || value > 4096) return PWN_EINVAL; memset(&c->room, 0, sizeof(c->room)); c->room.mode = value; return PWN_OK;
		case PWN_OPT_CALL_STRIPS:
			if(value < -1 || value == 1 || value > PWN_CALL_STRIPS_MAX) return PWN_EINVAL;
			c->call_strips = value; c->strip_backoff = 0; c->strip_reach = 0; return PWN_OK;
		case PWN_OPT_FRAME_OVERLAP:
			for(int i = 0; i < c->nslots; i++) if(c->slot[i].in_flight) return PWN_EBUSY;
			c->frame_overlap = value ? 1 : 0; return PWN_OK;
	}
	return PWN_EINVAL;
}

extern "C" int pwn_read_plane(pwn_ctx *c, const void *d_src, void *dst, size_t bytes)
{
	if(GRP_HEAD(c)) return pwn_group_on_member0(c, [d_src, dst, bytes](pwn_ctx *m0) { return pwn_read_plane(m0, d_src, dst, bytes); });       // (a frame that stayed on the devices was gathered on member 0's)
	if(c == NULL || d_src == NULL || dst == NULL) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	HIPCHK(c, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
	return PWN_OK;
}

extern "C" int pwn_get_stats(pwn_ctx *c, pwn_stats *out)
{
	if(GRP_HEAD(c)) return out == NULL ? PWN_EINVAL : pwn_group_get_stats(c, out);
	if(c == NULL || out == NULL) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	if(c->counters_on)
	{
		unsigned long long v[PWN_NCOUNTERS];
		HIPCHK(c, hipMemcpy(v, c->d_counters, sizeof(v), hipMemcpyDeviceToHost));
		for(int i = 0; i < 32; i++) c->stats.regions[i] = v[16 + i];
		c->stats.rays = v[0]; c->stats.steps = v[1]; c->stats.portals = v[2];
		c->stats.sphere_tests = v[3]; c->stats.exhausted = v[4]; c->stats.wave_steps = v[5];
		for(int i = 0; i < 8; i++) c->stats.wave_paths[i] = v[6 + i];
		c->stats.phase_passes = v[14]; c->stats.phase_lanes = v[15];
	}
	if(c->wave_log_on && c->d_wave_log != NULL)
	{
		std::vector<unsigned long long> log(c->wave_log_cap * 2);
		HIPCHK(c, hipMemcpy(log.data(), c->d_wave_log, log.size() * 8, hipMemcpyDeviceToHost));
		unsigned long long sum = 0, first = ~0ull, last = 0, n = 0;
		for(size_t i = 2; i + 1 < log.size(); i += 2)
		{
			if(log[i + 1] == 0) continue;
			sum += log[i + 1] - log[i]; n++;
			if(log[i] < first) first = log[i];
			if(log[i + 1] > last) last = log[i + 1];
		}
		c->stats.wave_time = sum; c->stats.waves = n; c->stats.kernel_span = n ? last - first : 0;
		if(const char *path = getenv("PWN_DBG_WAVE_LOG"))        // tools/wave_log.py: the raw log
			if(FILE *fp = fopen(path, "wb")) { fwrite(log.data(), 8, log.size(), fp); fclose(fp); }
		if(const char *path = getenv("PWN_DBG_UNIT_COST"))       // tools/unit_order_sim.py: u16 per unit (arithmetic numbering), 40 ns each
			if(c->order[0].d_cost != NULL && c->order[0].units > 0)
			{
				std::vector<uint16_t> uc(c->order[0].units);
				HIPCHK(c, hipMemcpy(uc.data(), c->order[0].d_cost, uc.size() * 2, hipMemcpyDeviceToHost));
				if(FILE *fp = fopen(path, "wb")) { fwrite(uc.data(), 2, uc.size(), fp); fclose(fp); }
			}
	}
	*out = c->stats;
	return PWN_OK;
}

// ---- sink -------------------------------------------------------------------

extern "C" int pwn_upscale_device(pwn_ctx *c, const void *d_src, int scale, int pitch_bytes, void *d_dst, void *stream)
{
	GRP_REFUSE(c, "pwn_upscale_device");
	if(c == NULL || d_src == NULL || d_dst == NULL || scale <= 0 || (pitch_bytes & 3) != 0 ||
	   (long long)pitch_bytes < (long long)c->w * scale * 4) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	HIPCHK(c, pwn_launch_upscale((const uint32_t *)d_src, (uint32_t *)d_dst, c->w, c->h, scale, pitch_bytes / 4, (hipStream_t)stream));
	return PWN_OK;
}

extern "C" int pwn_screen_upscale(pwn_ctx *c, const uint32_t *sbuf, int scale, int pitch_bytes, uint32_t *pixels)
{
	if(GRP_HEAD(c)) return pwn_group_screen_upscale(c, sbuf, scale, pitch_bytes, pixels);
	if(c == NULL || pixels == NULL || scale <= 0 || (pitch_bytes & 3) != 0 ||
	   (long long)pitch_bytes < (long long)c->w * scale * 4) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	size_t n = (size_t)c->w * (size_t)c->h;
	size_t dst_bytes = (size_t)pitch_bytes * (size_t)c->h * (size_t)scale;
	int rc = ensure_scratch(c, dst_bytes + n * 4);
	if(rc != PWN_OK) return rc;
	uint32_t *d_dst = c->d_scratch;
	const uint32_t *d_src = c->d_out;
	if(sbuf != NULL)
	{
		uint32_t *d_in = (uint32_t *)((uint8_t *)c->d_scratch + dst_bytes);
		HIPCHK(c, hipMemcpyAsync(d_in, sbuf, n * 4, hipMemcpyHostToDevice, c->stream));
		d_src = d_in;
	}
	// With pitch == w*scale*4 every byte of the surface is written.  Otherwise
	// the reference leaves gaps untouched (and packs rows, see the kernel):
	// start from the caller's surface so that untouched bytes survive.
	bool padded = (long long)pitch_bytes != (long long)c->w * scale * 4;
	if(padded) HIPCHK(c, hipMemcpyAsync(d_dst, pixels, dst_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, pwn_launch_upscale(d_src, d_dst, c->w, c->h, scale, pitch_bytes / 4, c->stream));
	HIPCHK(c, hipMemcpyAsync(pixels, d_dst, dst_bytes, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return PWN_OK;
}

// ---- probes -----------------------------------------------------------------

extern "C" int pwn_probe(pwn_ctx *c, int op, const uint32_t *in, uint32_t *out, int n)
{
	if(GRP_HEAD(c)) return pwn_group_on_member0(c, [op, in, out, n](pwn_ctx *m0) { return pwn_probe(m0, op, in, out, n); });
	if(c == NULL || in == NULL || out == NULL || n < 0 || op < 0 || op > PWN_PROBE_COS_OF_PAIR) return PWN_EINVAL;
	if(n == 0) return PWN_OK;
	(void)hipSetDevice(c->device);
	size_t per = (op == PWN_PROBE_DIV) ? 2 : (op == PWN_PROBE_FTOINT ? 4 : 1);
	size_t in_bytes = (size_t)n * per * 4, out_bytes = (size_t)n * 4;
	int rc = ensure_scratch(c, in_bytes + out_bytes + 8192);
	if(rc != PWN_OK) return rc;
	uint8_t *base = (uint8_t *)c->d_scratch;
	uint16_t *d_tabs = (uint16_t *)base;
	uint32_t *d_in = (uint32_t *)(base + 8192), *d_out = (uint32_t *)(base + 8192 + in_bytes);
	HIPCHK(c, hipMemcpy(d_tabs, c->tabs, 8192, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, pwn_launch_probe(op, d_in, d_out, n, d_tabs, c->stream));
	HIPCHK(c, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return PWN_OK;
}
