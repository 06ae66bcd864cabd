// pwn_internal.h -- the context behind include/pwnhip.h, shared by the translation
// units of libpwnhip.so:
//   pwn_api.cpp     context, options, the room control, stats, sink, probes
//   pwn_tables.cpp  level, objects, the sphere tables: their size rules, packing and upload
//   pwn_launch.cpp  the trace and blur launchers (the launch geometry itself: launch_plan.h), the unit order, the *_rows_device calls
//   pwn_calls.cpp   the blocking call and its strips, host registration, the batches of views, viewports, rays and hits
//   pwn_players.cpp the players' step: a batch of cameras walked through the level (host and device form)
//   pwn_reach.cpp   rays that stop after a given distance (pwn_trace_reach and its device forms)
//   pwn_pixel_rays.cpp  pixel rays from cameras on the device (pwn_pixel_rays_device)
//   pwn_spheres_device.cpp  the sphere tables built on the device (pwn_upload_spheres_device)
//   pwn_level_device.cpp  the level's tables baked on the device (pwn_upload_level_device)
//   pwn_viewports_device.cpp  views of their own sizes from device cameras (pwn_viewports_layout, pwn_trace_viewports_device)
//   pwn_frames.cpp  frames in flight
//   pwn_tiled.cpp   row tiling over RCCL
//   pwn_group.cpp   several contexts behind one handle
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include <atomic>

#include "pwnhip.h"
#include "tables.h"

// A batch of views (pwn_trace_views) as what a trace launch traces: n views, their records (tables.h pwn_view_rec) already on
// the device, into planes `plane` pixels apart; has_w: some view's camera has w components.  n = 0: none.
// d_label (pwn_trace_view_hits / pwn_trace_view_hits_device): not NULL = the launch writes the views' first-hit planes instead, from the
// primary segments alone: the label plane there, the cell plane to the launch's d_sbuf and the distance plane to its d_zbuf (each
// unless NULL); the records' times are then not read.
// hide (pwn_trace_views_hide_device / pwn_trace_view_hits_hide_device): the records' `hide` words count -- the launch runs the HIDE kernels.
struct pwn_views_launch
{
	const pwn_view_rec *d_recs;
	int n;
	bool has_w;
	unsigned long long plane;
	uint32_t *d_label;
	bool hide;
};

// Views of their own sizes in rectangles of one frame (pwn_trace_viewports) as what a launch traces or blurs: n records (tables.h
// pwn_viewport_rec) on the device, in the order the trace kernel expects, and the same records on the host (the blur launcher
// counts the tiles of the shape it picks); units = the launch's 16 x 4 units over all views.  n = 0: none.
// fw x fh: the size of the planes the rectangles lie in (fw is their pitch), 0 = the context's (pwn_trace_viewports); d_skip: the
// blur's skip-ahead table where the context's may be too short for the widest view (pwn_trace_viewports_device), NULL = the context's.
// d_label (pwn_trace_viewport_hits / pwn_trace_viewport_hits_device): not NULL = the launch writes the views' first-hit planes instead,
// from the primary segments alone: the label plane there, the cell plane to the launch's d_sbuf and the distance plane to its d_zbuf
// (each unless NULL), one plane of fw x fh words each; the records' times are then not read.
// hide (pwn_trace_viewports_hide_device / pwn_trace_viewport_hits_hide_device): the records' `hide` words count -- the launch runs the HIDE kernels.
struct pwn_vps_launch
{
	const pwn_viewport_rec *d_recs, *h_recs;
	int n;
	bool has_w;
	uint32_t units;
	int fw, fh;
	const uint2 *d_skip;
	uint32_t *d_label;
	bool hide;
};

// A batch of caller-supplied rays (pwn_trace_rays / pwn_trace_rays_device; tables.h pwn_trace_params.rays): n rays into
// d_sbuf (colour) / d_zbuf (depth) of the launch; has_w: their w lanes count (PWN_RAYS_HAS_W).  n = 0: none.
// d_hits (pwn_trace_hits / pwn_trace_hits_device): not NULL = the launch writes n first-hit records (pwn_hit) there instead,
// from the primary segments alone; d_seeds, d_sbuf, d_zbuf and sec are then not read.
// d_hide (pwn_trace_hits_hide_device with d_hits, pwn_trace_rays_hide_device without): not NULL = n int32, ray i's hidden sphere -- the
// launch runs the HIDE kernels.
// d_reach (pwn_trace_reach / pwn_trace_reach_device / pwn_trace_reach_hide_device, with d_hits): not NULL = n floats, ray i's reach -- the
// launch runs the REACH kernels, with d_hide those that hide as well.
struct pwn_rays_launch
{
	const float *d_rays;
	const uint32_t *d_seeds;
	uint32_t n;
	bool has_w;
	void *d_hits;
	const int32_t *d_hide;
	const float *d_reach;
};

// One trace launch (pwn_i_launch_trace).  All zero but what is traced and where to: a plain launch, nothing cleared or
// added up, no room, the launcher's own tables event.
struct pwn_trace_launch
{
	const float *cam; float sec; int y0, y1;     // rows [y0, y1) of camera cam[16]'s frame (y0 == y1: nothing is launched) ...
	pwn_views_launch views;                      // ... or of every view of a batch (cam and sec not read) ...
	pwn_rays_launch rays;                        // ... or a batch of rays (cam and the rows not read)
	pwn_vps_launch vps;                          // ... or views of their own sizes into one frame (cam, sec and the rows not read)
	uint32_t *d_sbuf; float *d_zbuf; hipStream_t stream;
	uint32_t *clear_word, *cost_word;            // pwn_trace_params.clear_word, .cost_word
	// An event the caller records itself right behind this launch anyway (its frame's "kernels done").  The launcher
	// then records none of its own -- every event between two kernels costs the queue a few microseconds.  The caller
	// must have waited on the host for the frame of the event's previous record (a slot is handed in again only when it
	// is free): the launcher drops the guards that still point at the event before the caller records it again.
	hipEvent_t tables_event;
	int room;                                    // PWN_OPT_TRACE_ROOM: workgroups this launch leaves free (a number set by the host goes first)
	// out: resident grid / grid launched, what the launch's cost word is to be scaled by (1 / 1 where nothing was launched)
	uint32_t cost_mul, cost_div;
};

// One blur launch (pwn_i_launch_blur).  All zero but the rows, the planes and the stream: every row of `d_pre` valid, no
// cost word, one frame.
struct pwn_blur_launch
{
	int y0, y1;
	const uint32_t *d_pre; const float *d_z; uint32_t *d_out; hipStream_t stream;
	int avail_y0, avail_y1; uint32_t *d_miss;    // pwn_blur_params.avail_y0, .avail_y1, .miss
	uint32_t *d_cost_acc, *d_cost_out;           // pwn_blur_params.cost_acc, .cost_out ...
	uint32_t cost_mul, cost_div;                 // ... scaled by what the frame's trace launch gave out (0 = 1)
	int views;                                   // a batch of views (pwn_trace_views): that many, planes w * h apart (0 = one frame)
	pwn_vps_launch vps;                          // views of their own sizes in one frame (pwn_trace_viewports): each rectangle a frame of its own (rows not read)
};

// the units kernel: mode (PWN_KM_*, with its HIDE and REACH bits; launch_plan.h pwn_launch_mode), lists (PWN_LF_*) and order pick the
// variant, whichever unit compiles it; hipErrorInvalidValue where trace_variants.h has none
extern "C" hipError_t pwn_launch_trace(int mode, int lists, bool order, const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream);
extern "C" hipError_t pwn_launch_trace_refill(const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream);
extern "C" unsigned pwn_trace_refill_lds_extra(bool has_w);
extern "C" int pwn_trace_refill_blocks_per_cu(size_t lds_bytes, bool count, bool has_w);
extern "C" int pwn_trace_blocks_per_cu(size_t lds_bytes, bool count, bool has_w);
extern "C" int pwn_trace_global_blocks_per_cu(size_t lds_bytes, bool count, bool has_w);
extern "C" int pwn_trace_tile_h(void);
extern "C" int pwn_trace_tile_w(void);
extern "C" unsigned pwn_trace_lds_extra(void);
extern "C" hipError_t pwn_launch_blur(const pwn_blur_params *P, hipStream_t stream);
extern "C" hipError_t pwn_launch_order(const uint16_t *cost, uint32_t units, uint32_t cap, uint32_t *perm, hipStream_t stream);
extern "C" hipError_t pwn_launch_upscale(const uint32_t *src, uint32_t *dst, int w, int h, int scale, int pitch, hipStream_t stream);
extern "C" hipError_t pwn_launch_upload(const void *h_pinned_src, void *d_dst, size_t bytes, hipStream_t stream);
// the camera set-up of n views from device memory (view_setup.hip): d_cams n x 16 floats and d_out 16-byte aligned; d_secs NULL: every time 0
extern "C" hipError_t pwn_launch_view_setup(const float *d_cams, const float *d_secs, pwn_view_rec *d_out, int n, int w, int h, hipStream_t stream);
// ... with every view's hidden sphere: d_hide n int32 (or NULL: the call above), record i's `hide` word = d_hide[i] + 1 where that is 1 .. PWN_OBJ_MAX, else 0
extern "C" hipError_t pwn_launch_view_setup_hide(const float *d_cams, const float *d_secs, const int32_t *d_hide, pwn_view_rec *d_out, int n, int w, int h, hipStream_t stream);
// the records of pwn_trace_viewports_device (viewport_setup.hip): record j's geometry words from the layout's master copy d_master, its
// head from camera d_perm[j] and time d_secs[d_perm[j]] with the view's own scalars d_scal[j] = (-yrat, xsrat, ysrat, 0); all but
// d_secs and d_perm 16-byte aligned, every d_perm[j] < n; d_secs NULL: every time 0 (pwn_trace_viewport_hits_device)
extern "C" hipError_t pwn_launch_viewport_setup(const pwn_viewport_rec *d_master, const float *d_scal, const uint32_t *d_perm,
	const float *d_cams, const float *d_secs, pwn_viewport_rec *d_out, int n, hipStream_t stream);
// ... with every rectangle's hidden sphere: d_hide n int32 in the caller's order (or NULL: the call above), record j's `hide` word =
// d_hide[d_perm[j]] + 1 where that is 1 .. PWN_OBJ_MAX, else 0
extern "C" hipError_t pwn_launch_viewport_setup_hide(const pwn_viewport_rec *d_master, const float *d_scal, const uint32_t *d_perm,
	const float *d_cams, const float *d_secs, const int32_t *d_hide, pwn_viewport_rec *d_out, int n, hipStream_t stream);
// d_hide of the *_hide_device calls (include/pwnhip.h): n int32 in device memory, 4-byte aligned, apart from every range the call
// writes -- wr[k] .. + wr_bytes (NULL: not given)
bool pwn_i_hide_array_ok(const void *d_hide, size_t n, const void *const *wr, int nwr, size_t wr_bytes);
// ticks of host/player.c's pwn_player_step for n players (player_step.hip): d_cams n x 16 floats and d_gravity n x 4 floats, 16-byte aligned,
// d_traversals n int32 or NULL, d_keys n bytes; stage != 0: every workgroup copies the walk table into LDS first
extern "C" hipError_t pwn_launch_players_step(float *d_cams, float *d_gravity, int32_t *d_traversals, const uint8_t *d_keys, int n,
	float tdiff, int ticks, const pwn_walk_table *d_walk, int stage, hipStream_t stream);
// the ray records and seeds of pwn_pixel_rays_device (pixel_rays.hip) from the view records d_recs: total = n x m rays, ray i * m + j camera
// i's pixel j; d_xy m pairs (shared != 0) or total pairs, or NULL = the whole frame (m == width x height); d_seeds or NULL; the magic
// numbers of the divisions by m and by width (launch_plan.h pwn_unit_div_magic)
extern "C" hipError_t pwn_launch_pixel_rays(const pwn_view_rec *d_recs, const int32_t *d_xy, float *d_rays, uint32_t *d_seeds, uint32_t total,
	uint32_t m, uint32_t m_magic, int m_shift, int shared, int width, uint32_t w_magic, int w_shift, hipStream_t stream);
// the sphere tables in the lists' device-memory form built from n sphere records in device memory (sphere_bins.hip): four launches on
// `stream`.  d_scratch: PWN_SD_SCRATCH_BYTES; d_base: the level's part of the blob, PWN_T_BINIDX bytes; d_blob: the copy's LDS part;
// d_big: its device-memory part, laid out for max_pairs records and n spheres, sections at which_off / sph_off
extern "C" hipError_t pwn_launch_sphere_bins(const void *d_spheres, uint32_t n, uint32_t max_pairs, void *d_scratch, const void *d_base,
	void *d_blob, void *d_big, uint64_t which_off, uint64_t sph_off, hipStream_t stream);
// ... its scratch: a box word per sphere, 4096 counts, 4096 list starts, the status words of the last build
#define PWN_SD_BOX_WORDS 10240u
#define PWN_SD_STATUS_WORD (PWN_SD_BOX_WORDS + 8192u)
#define PWN_SD_SCRATCH_BYTES ((PWN_SD_STATUS_WORD + 8u) * 4u)
enum { PWN_SD_ST_PAIRS = 0, PWN_SD_ST_NCELL = 1, PWN_SD_ST_LONGEST = 2, PWN_SD_ST_REASON = 3, PWN_SD_ST_N = 4, PWN_SD_ST_MAX_PAIRS = 5 };
// the level's part of the tables from a grid (and a portal table, or NULL: derived) in device memory (level_bake.hip): one launch on
// `stream`.  On verdict 0 the cell words and endpoint records of d_base and the walk table d_walk are written; else d_base is left
// alone and d_walk_prev (another buffer) is copied into d_walk.  d_status: PWN_LD_STATUS_WORDS words -- verdict, offending letter,
// records, paired letters, derived, 0, 0, and word 7: a device-built level is in force, carried over from the build before where
// prev_dev != 0 (else that word is not read).
extern "C" hipError_t pwn_launch_level_bake(const void *d_data, const void *d_pmap, void *d_base, pwn_walk_table *d_walk,
	const pwn_walk_table *d_walk_prev, uint32_t *d_status, int prev_dev, hipStream_t stream);
#define PWN_LD_STATUS_WORDS 8u
enum { PWN_LD_ST_VERDICT = 0, PWN_LD_ST_LETTER = 1, PWN_LD_ST_RECS = 2, PWN_LD_ST_PAIRED = 3, PWN_LD_ST_DERIVED = 4, PWN_LD_ST_DEV = 7 };
extern "C" hipError_t pwn_launch_words(const uint32_t *d_all, const uint32_t *d_own, uint32_t *h_pinned_dst, int world, hipStream_t stream);
extern "C" hipError_t pwn_launch_probe(int op, const uint32_t *in, uint32_t *out, int n, const uint16_t *tabs, hipStream_t stream);

// The camera-independent scalars of the camera set-up (screen.h:43-57) of a w x h frame, in the reference build's operation
// order: frame_setup (below) and the device's set-up (view_setup.hip) both take them from here, computed on the host.
struct pwn_setup_scalars { float yrat, xsrat, ysrat; };
static inline pwn_setup_scalars pwn_frame_setup_scalars(int w, int h)
{
	float dimx = (float)w, dimy = (float)h;
	pwn_setup_scalars s;
	s.yrat = (-dimy) / dimx;
	s.xsrat = -2.0f / dimx;
	s.ysrat = (s.yrat + s.yrat) / dimy;
	return s;
}
// screen.h:43-57 in the reference build's operation order:
// rayb = (cam.x + cam.z) + (-yrat)*cam.y
// (into a launch's parameters, or into the head that a view's record shares with them: pwn_view_rec, pwn_viewport_rec)
template<class T> static inline void frame_setup(int w, int h, const float cam[16], T *P)
{
	const pwn_setup_scalars S = pwn_frame_setup_scalars(w, h);
	const float yrat = S.yrat, xsrat = S.xsrat, ysrat = S.ysrat;
	for(int i = 0; i < 4; i++)
	{
		P->rayb[i] = (cam[0 + i] + cam[8 + i]) + (-yrat) * cam[4 + i];
		P->rdx[i] = xsrat * cam[0 + i];
		P->rdy[i] = ysrat * cam[4 + i];
		P->from[i] = cam[12 + i];
	}
}
// ordinary cameras (rows x,y,z with w = 0, position w = 1: mat4_iden + rotations,
// main.c:61-64) never put anything but 0 / 1 into the w lanes; the kernel has a
// 3-lane specialisation for them that is arithmetically identical
static inline bool camera_has_w(const float cam[16]) { return !(cam[3] == 0.0f && cam[7] == 0.0f && cam[11] == 0.0f && cam[15] == 1.0f); }

// LDS budget for the table blob: leave room so that at least two workgroups
// fit per CU (160 KiB LDS per CU on gfx950)
#define PWN_BLOB_MAX (72u * 1024u)
// ... and for the device-memory part of tables whose lists do not fit there (tables.h PWN_LF_GLOBAL).  10000 spheres with boxes
// of 3 x 3 cells need about 2 MB; the limit exists because a sphere's box may cover all 4096 cells.
#define PWN_TABLES_MAX (16u << 20)
#ifndef PWN_NBLOB
#define PWN_NBLOB 4       // device copies of the blob: an upload never touches one that launches in flight read.  With two, the upload
                          // of frame f+1's tables had to wait for the end of frame f-1 and so ran right where trace f starts;
                          // with three or four it runs at once, somewhere beside the trace grid: 0.3823 -> 0.3790 ms per 4K frame
#endif
#define PWN_NCOUNTERS 48     // device counters of the counting kernel variants: 16 (pwn_stats) + 31 regions + waves
#define PWN_TILED_STREAMS_DEFAULT 2
#define PWN_TICKET_SETS 6u  // launch n counts in set n mod 2R and clears set (n + R) mod 2R, R = pwn_ctx.launch_rot streams in rotation, 2 or 3 (pwn_i_launch_trace)
#define PWN_NSTAGE 4      // pinned staging buffers for those uploads
#define PWN_CALL_STRIPS_MAX 32   // row strips of one blocking call at most
#define PWN_HOST_REGS_MAX 16     // host buffers a context keeps registered (pwn_host_register)

// one frame in flight (pwn_submit_frame / pwn_wait_frame)
struct pwn_slot
{
	uint32_t *d_out; float *d_z; uint32_t *d_surface;      // device: final colour, depth, upscaled surface
	uint32_t *h_sbuf; float *h_zbuf; uint32_t *h_surface;  // pinned host copies handed to the caller
	hipEvent_t ev_k[4];                                    // compute stream: start, after trace, after blur, after sink
	hipEvent_t ev_done;                                    // copy stream: this frame's host buffers are complete
	bool in_flight, timed, beside;                         // (beside: launched while frames alternate between two streams)
	float sec;
	uint64_t seq;
};

// PWN_OPT_TRACE_ROOM: how many workgroups the persistent trace grid leaves free while frames alternate between two compute
// streams, so that the OTHER stream's kernels (the previous frame's blur, the next frame's grid) find room on every CU instead
// of waiting for this grid's end.  Worth +3.5 % at 4K and -11 % kernel time on the strips of an 8-way tiling on level.txt,
// and -3 % on synth256: so the default measures -- pwn_room_frame_done() is told of every delivered frame,
// times a window of frames with no room and one with a workgroup per CU, keeps the better for a while, and looks again.
struct pwn_room_ctl
{
	int mode;                 // -1: measure (default); >= 0: that many workgroups, always
	int arm, best;            // 0 = no room, 1 = one workgroup per CU
	int skip, hold;           // delivered frames not counted after a switch; frames left before the next look
	double sum[2]; int cnt[2];
	double t_prev, t_hold;
	unsigned long long looks, switches;
};
int pwn_room_for_launch(struct pwn_ctx *c);          // workgroups to leave free for a launch on one of two alternating streams
void pwn_room_frame_done(struct pwn_ctx *c);         // a frame of such a sequence was delivered to the host

struct pwn_tiled;        // pwn_tiled.cpp
struct pwn_group;        // pwn_group.cpp: several contexts of one process behind one handle (pwn_init_multi)

// What the members of a group share besides their handle (pwn_group.cpp makes it, pwn_tiled.cpp uses it): a meeting point for the
// members' threads with a deadline, a flag that ends every wait when a member has failed, the members themselves (every member
// reads the others' two words of a frame straight from their pinned memory: one process, no exchange needed for eight bytes),
// and the mailboxes of the in-process transport (PWN_TRANSPORT_LOCAL).
#define PWN_HUB_RING 64
// One box per ordered pair (from -> to).  A message is a rendezvous: the receiver posts where the bytes are to go and an event
// behind whatever of its own still uses that place; the sender, on ITS stream, waits for that event, copies, and says so with an
// event the receiver's stream then waits for.  So a send is complete, in the sender's stream order, when the bytes have left --
// the sender may overwrite its buffer behind it, as with ncclSend.
struct pwn_hub_post { void *dst; size_t bytes; hipEvent_t ev_free; int device; };
struct pwn_hub_box
{
	std::atomic<unsigned long long> posted, copied, consumed;      // by the receiver; by the sender (<= posted); by the receiver (<= copied)
	pwn_hub_post post[PWN_HUB_RING];
	hipEvent_t done[PWN_HUB_RING];
};
struct pwn_hub
{
	int world;
	std::atomic<int> failed;                     // a member gave up (an error, a deadline): nobody waits for it any more
	std::atomic<unsigned> bar_count, bar_gen;
	struct pwn_ctx *member[PWN_TILED_MAX_WORLD];
	pwn_hub_box *boxes;                          // world x world, [from * world + to]
};
int pwn_hub_meet(pwn_hub *h, int wait_ms);       // every member's thread arrives, or PWN_ETIMEDOUT / PWN_EHIP (failed)

struct pwn_ctx
{
	int device, w, h;
	int num_cus;
	int blur_passes, counters_on, scheduler, refill_limit;
	bool have_level;

	uint8_t cells[4096];
	uint32_t cell_base[65 * 65];      // the level's part of every cell word (class bits + the baked low byte, cell_bake.h; row / column 64 = the
	bool cell_base_ok;               // clamp copies): built by pwn_i_pack_blob when the level OR its portal table changed, patched per upload with the cells' sphere lists
	uint32_t ep_recs[PWN_EP_MAX];    // ... and the portals' endpoint records that go with it
	pwn_portal pmap[26];
	int32_t spawn[2];
	std::vector<pwn_sphere> spheres;          // the live spheres the current lists index
	std::vector<int32_t> bin_off, bin_idx;
	std::vector<pwn_sphere> objs;             // lv->objs (defs.h:98): every slot ever handed out
	std::vector<uint8_t> obj_typ;             // P_INVAL / P_FREE / P_SPHERE (defs.h:55-60)

	std::vector<uint8_t> blob;       // host image of the LDS blob
	// The device copy exists twice: an upload goes into the buffer the launches in flight do not
	// read, on its own stream and from a pinned staging ring, so the host never waits for the GPU
	// between frames (level_prepare_render runs every frame, main.c:95).
	uint8_t *d_blob[PWN_NBLOB]; int blob_cur;
	bool blob_has_static[PWN_NBLOB];                                   // the rcp / rsqrt tables are in place
	hipEvent_t ev_tables[PWN_NBLOB]; bool tables_in_use[PWN_NBLOB];    // behind the last trace launch reading that copy
	hipEvent_t tables_wait[PWN_NBLOB];                                 // ... the event to wait for: ev_tables[i], or the caller's (pwn_trace_launch.tables_event)
	hipEvent_t ev_upload[PWN_NBLOB]; bool upload_pending[PWN_NBLOB];   // behind the last upload into that copy
	uint8_t *h_stage[PWN_NSTAGE]; hipEvent_t ev_stage[PWN_NSTAGE]; bool stage_used[PWN_NSTAGE]; unsigned stage_next;
	hipStream_t up_stream;
	uint16_t tabs[4096];             // expanded rcp + rsqrt tables (never change)
	uint32_t off_sph;
	uint32_t off_recsph; int dbg_sphere_lists;      // inline sphere records in the per-cell lists (tables.h): where their "which sphere" array is, 0 = indexed lists; PWN_SPHERE_LISTS
	// The lists' global form (tables.h PWN_LF_GLOBAL): `blob` is then the LDS part alone and `big` the host image of the device-memory
	// part, big_which / big_sph its sections.  Copy i of the tables has d_big[i] beside d_blob[i], under the same events; staging
	// buffer i of the ring has h_big[i] beside h_stage[i].  All of them are allocated with the first tables that need them and
	// grown to the largest so far (big_high); pwn_i_pack_blob says what growing waits for.
	int lists_form;                  // PWN_LF_* of the tables in force
	pwn_sphere_bound bounds[PWN_BOUNDS_MAX]; int nbounds;      // the balls of their longest lists (sphere_bound.h), made with them by pwn_i_pack_blob
	int dbg_sphere_bounds;           // PWN_SPHERE_BOUNDS of the environment: 0 = launches are sent no balls (tests, A/B in one process)
	std::vector<uint8_t> big; uint64_t big_which, big_sph;
	uint8_t *d_big[PWN_NBLOB]; size_t d_big_cap[PWN_NBLOB];
	uint8_t *h_big[PWN_NSTAGE]; size_t h_big_cap[PWN_NSTAGE];
	size_t big_high;
	bool blob_dirty;
	// The walk tables of the players' step (tables.h pwn_walk_table): as many buffers as copies of the tables.  Copy i of the tables
	// reads buffer walk_of[i].  A level upload fills a buffer no other copy refers to, from pinned h_walk[staging slot], on the upload
	// stream under the copy's ev_upload; an upload of spheres alone hands the current copy's buffer on to the copy it makes current
	// and sends nothing.  A step that reads copy i records ev_walk[i] behind itself, and the next upload into copy i waits for it.
	// An event holds one record: a step on another stream than the last one that read copy i (walk_stream[i]) first puts the upload
	// stream behind the record that is there, so that no upload gets ahead of a step on any stream.
	pwn_walk_table *d_walk[PWN_NBLOB], *h_walk[PWN_NSTAGE];
	int walk_of[PWN_NBLOB];
	bool walk_dirty;                 // the level changed and no walk table of it has been sent yet
	hipEvent_t ev_walk[PWN_NBLOB]; bool walk_in_use[PWN_NBLOB]; hipStream_t walk_stream[PWN_NBLOB];
	size_t occ_lds[12]; int occ_blocks[12];    // cached occupancy query per kernel variant
	// pwn_upload_spheres_device (pwn_spheres_device.cpp): tables built on the device from spheres in device memory, into the next copy
	// of the ring above, in the lists' device-memory form laid out for a declared capacity.  in_force: the tables in force are such
	// tables -- pwn_i_pack_blob clears it, and while it is set nothing repacks from the host's spheres (pwn_set_option).  d_base: the
	// level's part of the blob on the device (static head, cell words without sphere bits, eprec), made from pinned h_base by the
	// first build after a level change (base_ok; pwn_i_pack_blob clears that with cell_base_ok), under ev_base.  Builds share
	// d_scratch and d_base, so each is put behind the one before it (ev_build, build_stream) where the stream differs.
	struct spheres_device_state
	{
		bool in_force, base_ok, base_used, built;
		int n, max_pairs;                         // of the last build
		unsigned long long uploads;
		uint8_t *d_base, *h_base, *d_scratch;
		hipEvent_t ev_base, ev_build; hipStream_t build_stream;
	} sd;
	// pwn_upload_level_device (pwn_level_device.cpp): the level's part of the tables baked on the device, into sd.d_base, and a walk
	// table with it; then sphere-less tables built from that base copy as pwn_upload_spheres_device builds them.  in_force: such a
	// call has been made since the host's level last went up, so the base copy and the walk table of the tables in force MAY hold a
	// device-built level (whether they do is the builds' verdicts, which only the device knows: d_status word PWN_LD_ST_DEV).
	// pwn_i_pack_blob clears it, and with it sd.base_ok: the base copy is no longer the host's level.  ev_order: recorded on the
	// upload stream and waited for on the call's stream, which puts the bake behind everything the upload stream is behind.
	struct level_device_state
	{
		bool in_force, built;
		unsigned long long uploads;
		uint32_t *d_status;
		hipEvent_t ev_order;
	} ld;

	uint32_t *d_pre, *d_out;         // pre-blur ("tsbuf") and final ("sbuf") frames
	float *d_z;
	uint2 *d_skip;                   // blur LCG skip-ahead, w/4 entries
	unsigned long long *d_counters;
	unsigned long long *d_wave_log; int wave_log_on; size_t wave_log_cap;   // PWN_OPT_WAVE_LOG; entries (16 B) allocated
	// PWN_OPT_UNIT_ORDER: per stream that trace launches go out on ([0] `stream`, [1] `stream2`, [2..3] a strip-form caller's own)
	// what every unit of the last trace launch cost its wave (pwn_trace_params.unit_cost, indexed by the unit's number in
	// arithmetic order) and, sorted from that behind the frame's blur (pwn_i_launch_order), the order the NEXT launch of the same
	// rows on that stream hands its units out in.  Everything that touches one entry is ordered by ITS stream: the launch that
	// writes the costs, the sort that reads them and writes the order, the next launch that reads the order.
	struct unit_order_state
	{
		hipStream_t key; bool used; unsigned long long stamp;                 // the stream this entry belongs to
		uint16_t *d_cost; uint32_t *d_perm; size_t cost_cap, perm_cap;        // allocated: u16 entries, u32 entries
		uint32_t units, qcap; int y0, y1;                                     // what d_cost holds: of a launch over rows [y0, y1)
		bool cost_fresh;                                                      // written by a launch, not sorted yet
		uint32_t perm_units; int perm_y0, perm_y1; bool perm_valid;           // what d_perm orders
	} order[4];
	unsigned long long order_stamp;
	int tiled_choreo;                // PWN_OPT_TILED_CHOREO, read by pwn_tiled_init
	int tiled_streams;               // PWN_OPT_TILED_STREAMS, read by pwn_tiled_init
	int tiled_comms;                 // PWN_OPT_TILED_COMMS, read by pwn_tiled_init
	int unit_order;                  // the option: 1 = units handed out by last launch's cost, 0 = arithmetic order
	unsigned long long order_used, order_sorts;      // trace launches that ran in a sorted order; sorts launched (pwn_unit_order_state)
	bool dbg_force_hasw; int dbg_blocks_per_cu;      // PWN_DBG_* hooks, read at pwn_init
	int tile_pairs;                                  // PWN_TILE_PAIRS, read at pwn_init: 0 never, 1 where tickets would go out in pairs, 2 always (pwn_i_launch_trace)
	int dbg_blur_th, dbg_blur_tw, dbg_blur_batch;                 // PWN_DBG_BLUR_TH: tile height of every blur launch (8 / 16 / 32), 0 = the launcher's choice
	int grid_reserve;                // workgroups the persistent trace grid leaves free (row tiling over RCCL), else 0
	// pwn_trace_views: per view slot a pre-blur, a colour and a depth plane (views_cap of each, view-major; the depth planes persist
	// by slot and are kept when the count grows), the records of the call in pinned staging and on the device
	uint32_t *d_vpre, *d_vout; float *d_vz; int views_cap;
	pwn_view_rec *h_vrec, *d_vrec;
	// pwn_trace_views_device: PWN_VIEWS_MAX records per ticket set, written by the set-up kernel of the call whose trace launch
	// counts in that set (so reuse is ordered as the sets' is); allocated by the first call
	pwn_view_rec *d_vrec_dev;
	// pwn_trace_viewports: one pre-blur, one colour and one depth plane of w x h (the depth plane persists by pixel), the records
	// of the call in pinned staging and on the device (PWN_VIEWS_MAX of them)
	uint32_t *d_ppre, *d_pout; float *d_pz;
	pwn_viewport_rec *h_prec, *d_prec;
	// pwn_trace_viewports_device (pwn_viewports_device.cpp): PWN_VIEWS_MAX records per ticket set, as d_vrec_dev, allocated by the first
	// call; the layouts alive (pwn_viewports_layout), which pwn_destroy frees
	pwn_viewport_rec *d_prec_dev;
	std::vector<struct pwn_vp_layout *> vp_layouts;
	// pwn_trace_rays: room for rays_cap rays in pinned staging and on the device, 44 B each (record, seed, depth, colour; pwn_calls.cpp pwn_i_staging_reserve)
	unsigned char *h_rays, *d_rays; size_t rays_cap;
	// pwn_trace_hits: the same for hits_cap rays, 32 B in (record) and 48 B out (pwn_hit) each; pwn_trace_view_hits stages its planes
	// here too, 12 B a pixel (a call's label plane, behind it its cell plane, then its distance plane): no call uses both at once
	unsigned char *h_hits, *d_hits; size_t hits_cap;
	// pwn_players_step: room for players_cap players in pinned staging and on the device, 85 B each (camera, gravity, traversals, key byte)
	unsigned char *h_players, *d_players; size_t players_cap; int dbg_players_stage;      // (PWN_PLAYERS_STAGE=0 of the environment: the walk table read from device memory, not staged in LDS)
	uint32_t *d_tickets; unsigned ticket_set;  // PWN_TICKET_SETS sets of work-queue counters of the trace kernel, used in turn
	uint32_t *d_scratch; size_t scratch_cap;   // upscale / probe staging

	hipStream_t stream;              // compute
	hipStream_t stream2;             // frames in flight alternate between `stream` and this one (PWN_OPT_FRAME_OVERLAP)
	uint32_t *d_pre2;                // the pre-blur plane of the frames on stream2 (allocated with the first of them)
	pwn_room_ctl room;               // PWN_OPT_TRACE_ROOM
	int frame_overlap;               // PWN_OPT_FRAME_OVERLAP
	hipEvent_t last_frame_done; hipStream_t last_frame_stream;   // "kernels done" of the frame submitted last, and its stream
	hipStream_t copy_stream;         // frames in flight: D2H of finished frames
	hipEvent_t ev[4];
	// The blocking call in row strips (PWN_OPT_CALL_STRIPS; pwn_calls.cpp, call_in_strips): trace strip k, blur strip k - 1 from the
	// rows traced so far, strip k - 2 on its way to the caller's buffer -- the copy over PCIe is twice a 4K frame's kernels
	int call_strips;                 // the option: -1 = by frame size (default), 0 = one launch per pass, n >= 2 = that many strips
	hipStream_t copy_stream2;        // the blocking call in strips: chunks go out on one copy stream or on the two in turn
	int strip_copy_streams;          // ... 1 or 2 as found out by the context's first sixteen calls in strips (0: still finding out); PWN_CALL_COPY_STREAMS
	int strip_calib_n; double strip_calib_ms[16];
	hipEvent_t strip_ev[2 * PWN_CALL_STRIPS_MAX]; int strip_ev_n;      // behind strip k's trace [2k] and blur [2k + 1]; made on first use
	uint32_t *d_strip_miss, *h_strip_miss;     // taps of a strip's blur that left the rows traced so far: the device word, its pinned copy
	int strips_last;                 // strips of the last blocking call (1 = one launch per pass)
	int strip_reach;                 // 0: chunks are blurred where taps of depth <= 8 are traced, 1: <= 24 (after a frame whose taps went further)
	int strip_backoff;               // blocking calls left before strips are tried again after such a frame
	unsigned long long strip_calls, strip_redone;      // blocking calls that ran in strips; ... whose blur was repeated over the whole frame
	struct host_reg { void *base; size_t bytes; } host_regs[PWN_HOST_REGS_MAX]; int host_regs_n;     // pwn_host_register
	pwn_stats stats;

	// frames in flight
	int nslots, frame_flags, frame_scale, frame_pitch, frame_timing;
	pwn_slot slot[PWN_MAX_SLOTS];
	uint64_t frame_seq;

	pwn_group *grp; bool grp_head;   // pwn_init_multi: the group this context is the handle of (grp_head) or a member of; NULL otherwise
	pwn_hub *hub;                    // ... and what its members share (NULL outside a group)
	pwn_tiled *tiled;                // row tiling over RCCL, NULL until pwn_tiled_init
	int tiled_init_ms, tiled_wait_ms;   // pwn_tiled_set_timeouts (0 = the default: environment, else 120 s / 60 s)

	// The kernel's work queues are used in turn, 2R sets of them, R = launch_rot: launch n counts in set n mod 2R and clears set
	// (n + R) mod 2R, the one of the launch R launches on = the set launch n - R drew from, so it has to come after launch n - R.
	// Launches of a context are stream-ordered (include/pwnhip.h) -- on ONE stream, or rotating over the R = 2 compute streams of
	// the frames in flight (pwn_submit_frame) or the R = 2 or 3 of a row tiling, where launch n + R is behind launch n on its
	// stream and the launches between may run beside it with sets of their own.  So the order holds by itself on one stream and in
	// the rotation, NOT when a launch leaves that pattern (a blocking call or a counted frame between alternating ones): the last
	// launches' streams and an event behind each are kept here, and pwn_i_launch_trace then waits for the one R back.
	hipStream_t launch_stream[3]; hipEvent_t launch_event[3];     // [0] the last launch, [1] the one before, [2] the one before that
	unsigned long long launch_waits; // launches that left the rotation and were put behind the launch R before them (pwn_launch_order_waits)
	int launch_rot;                  // streams that successive trace launches rotate over: 2 (one stream, or two alternating), 3 (pwn_i_set_launch_rotation)

	char err[256];
};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { \
	snprintf((ctx)->err, sizeof((ctx)->err), "%s: %s", #call, hipGetErrorString(e_)); return PWN_EHIP; } } while(0)

// pwn_init_multi's handle (pwn_group.cpp): the call goes to the group, or to its member 0 where it is about the one
// level and object table, or is refused
#define GRP_HEAD(c) ((c) != NULL && (c)->grp != NULL && (c)->grp_head)
#define GRP_M0(c) pwn_group_member((c), 0)
#define GRP_REFUSE(c, what) do { if(GRP_HEAD(c)) { snprintf((c)->err, sizeof((c)->err), "%s is not available on a group's handle", what); return PWN_ENOTSUP; } } while(0)

// pwn_launch.cpp: the launchers, used by the calls, the frames in flight and pwn_tiled.cpp
int pwn_i_launch_trace(pwn_ctx *c, pwn_trace_launch *L);
int pwn_i_launch_blur(pwn_ctx *c, const pwn_blur_launch *L);
int pwn_i_tables_uploaded(pwn_ctx *c, int cur, hipStream_t stream);      // a launch on `stream` that reads copy `cur` of the tables comes after their upload
// pwn_calls.cpp, shared with pwn_players.cpp: what refuses a batch call once its own arguments are in order; a blocking call on
// stream s put behind the frames in flight; the pinned staging and device buffer of a blocking batch call grown to n records
int pwn_i_batch_refuse(const pwn_ctx *c, int views = 0, bool blurs = true);
int pwn_i_wait_frames_in_flight(pwn_ctx *c, hipStream_t s);
int pwn_i_staging_reserve(pwn_ctx *c, size_t n, size_t per_ray, const char *who, unsigned char **h, unsigned char **d, size_t *cap_io, size_t cap_max = PWN_RAYS_MAX, const char *unit = "rays");
// what the blocking ray calls do between filling their staging and reading it (pwn_calls.cpp): N records into the staging's head, the 3-lane /
// 4-lane rule over them, the first `up` bytes to the device, the launch T, bytes [lo, hi) back, the wait and the times
int pwn_i_rays_stage_and_launch(pwn_ctx *c, hipStream_t s, const float *rays, size_t N, unsigned char *h, unsigned char *d, size_t up,
	pwn_trace_launch *T, size_t lo, size_t hi);
void pwn_launch_history_clear(pwn_ctx *c);      // the launch-order events are about to be destroyed (streams idle)
int pwn_i_set_launch_rotation(pwn_ctx *c, int rot);
int pwn_i_launch_order(pwn_ctx *c, hipStream_t stream);      // behind a frame's last kernel on `stream`: sort that stream's unit costs (no-op when there are none)
// the blur passes behind a trace into *cur, the two planes taking turns, the last pass into `last` where one is given
int pwn_i_blur_passes_run(pwn_ctx *c, pwn_blur_launch B, uint32_t **cur, uint32_t *other, uint32_t *last = NULL);
// pwn_frames.cpp: every frame slot gone (no frame in flight); pwn_tables.cpp: the rcp / rsqrt tables as the kernels read them,
// and the tables in force packed and uploaded into the next copy
void pwn_i_frames_release(pwn_ctx *c);
void pwn_i_expand_tables(uint16_t *rcp, uint16_t *rsq);
int pwn_i_pack_blob(pwn_ctx *c);
void pwn_i_spheres_device_release(pwn_ctx *c);      // pwn_spheres_device.cpp: the device builder's buffers and events gone (pwn_destroy)
// ... shared with pwn_level_device.cpp: the builder's own buffers, once; room for `need` bytes of the device-memory part in copy nb; the
// base copy of the level in force made on stream s unless it is there
int pwn_i_sd_buffers(pwn_ctx *c);
int pwn_i_sd_big_reserve(pwn_ctx *c, int nb, size_t need);
int pwn_i_sd_base(pwn_ctx *c, hipStream_t s);
void pwn_i_level_device_release(pwn_ctx *c);        // pwn_level_device.cpp: its status words and event gone (pwn_destroy)
void pwn_i_viewports_device_release(pwn_ctx *c);    // pwn_viewports_device.cpp: every layout and the records gone (pwn_destroy, streams idle)
// pwn_calls.cpp, shared with pwn_viewports_device.cpp: the records of n rectangles in order of rising units, ties in the given order --
// recs[j] stands for rectangle ord[j]; its geometry words (rectangle, units, division constants, segment) are filled in, its head
// (rayb .. sec_current) is left alone.  Returns the units of all views.
uint32_t pwn_i_viewport_recs_bake(int n, const pwn_viewport *vp, pwn_viewport_rec *recs, int *ord);
void pwn_tiled_destroy(pwn_ctx *c);
bool pwn_tiled_busy(pwn_ctx *c);        // frames of the row tiling in flight
// pwn_tiled.cpp internals used by pwn_group.cpp: a member's frame with the host buffers its strip is delivered into (NULL: the
// frame stays on the devices and is gathered on member 0), and the switch that makes the tiling deliver to the host
int pwn_i_tiled_submit(pwn_ctx *c, const float cam[16], float sec, uint32_t *host_sbuf, float *host_zbuf, int zplane, uint32_t *host_surface);
int pwn_i_tiled_surface(pwn_ctx *c, int scale, int pitch_bytes);
int pwn_i_tiled_sink(pwn_ctx *c);
int pwn_i_tiled_ready(pwn_ctx *c, int ahead);
// pwn_tables.cpp: level_prepare_render's binning of a compact list of live spheres (no context: PWN_ETOOBIG where the lists would not
// fit on chip), and its upload into one context; the object table of pwn_upload_spheres by itself
struct pwn_binned { std::vector<pwn_sphere> s; std::vector<int32_t> off, idx; };
// The size rules of the sphere tables, in one place: which form the per-cell lists of these bins take under this scheduler
// (PWN_SCHED_*) and this PWN_SPHERE_LISTS setting (0 none, 1 indexed, 2 inline, 3 global), and what that costs.  PWN_ETOOBIG: no form holds them.
struct pwn_tables_plan
{
	int form;                        // PWN_LF_*
	uint32_t nsph, nrec, nbin, ncell, longest;      // spheres; (cell, sphere) pairs; entries of the indexed lists; non-empty cells; the longest list
	uint32_t blob_bytes;             // the blob = the LDS part, a multiple of 16
	uint64_t big_bytes;              // the device-memory part (0 unless form == PWN_LF_GLOBAL)
};
int pwn_i_tables_plan(const int32_t off[4097], uint32_t nsph, int scheduler, int forced, pwn_tables_plan *out);
int pwn_i_forced_lists(void);        // PWN_SPHERE_LISTS of the environment
int pwn_i_bin_spheres(const pwn_sphere *s, int n, pwn_binned *out);
int pwn_i_upload_binned(pwn_ctx *c, const pwn_binned &b);
void pwn_i_set_object_table(pwn_ctx *c, const pwn_sphere *s, int n);
// pwn_group.cpp: the entry points of include/pwnhip.h when the context is a group's handle
int pwn_group_set_option(pwn_ctx *h, int option, int value);
int pwn_group_level_mem(pwn_ctx *h, const char *text, int len);
int pwn_group_upload_level(pwn_ctx *h, const uint8_t *data, const pwn_portal *pmap);
int pwn_group_upload_spheres(pwn_ctx *h, const pwn_sphere *s, int n);
int pwn_group_prepare_render(pwn_ctx *h);
int pwn_group_trace_screen_centred(pwn_ctx *h, const float cam[16], float sec, uint32_t *sbuf, float *zbuf);
int pwn_group_frames_config(pwn_ctx *h, int nslots, int flags, int scale, int pitch_bytes);
int pwn_group_submit_frame(pwn_ctx *h, const float cam[16], float sec, int slot);
int pwn_group_wait_frame(pwn_ctx *h, int slot, pwn_frame *out);
int pwn_group_frame_ready(pwn_ctx *h, int slot);
int pwn_group_get_stats(pwn_ctx *h, pwn_stats *out);
int pwn_group_screen_upscale(pwn_ctx *h, const uint32_t *sbuf, int scale, int pitch_bytes, uint32_t *pixels);
int pwn_group_host_register(pwn_ctx *h, void *base, size_t bytes);
int pwn_group_host_unregister(pwn_ctx *h, void *base);
int pwn_group_set_timeouts(pwn_ctx *h, int init_ms, int wait_ms);
pwn_ctx *pwn_group_member(pwn_ctx *h, int i);                 // member i (0 = the one that holds the level and the object table)
int pwn_group_sync(pwn_ctx *h);                               // everything posted to the members is through
#include <functional>
int pwn_group_on_member0(pwn_ctx *h, const std::function<int(pwn_ctx *)> &fn);      // ... on member 0's thread
void pwn_group_destroy(pwn_ctx *h);
