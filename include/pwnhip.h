/*
 * pwnhip.h -- C ABI of libpwnhip.so, the MI355X (gfx950) implementation of
 * pwnfps's per-pixel portal ray-march path.
 *
 * Plain C: opaque context, plain pointers and sizes, int return codes
 * (0 = ok, negative = PWN_E*).  Nothing here aborts or asserts.
 * Each entry cites the reference interface it replaces (paths relative to
 * the reference tree).  INTEGRATION.md shows the host-side change.
 *
 * Like the reference's render path (globals, one main thread: main.c:26-34) a
 * context is not re-entrant: one thread at a time per context.  Trace launches
 * of a context take turns on four sets of work-queue counters: launch n counts in
 * set n mod 4 and clears the set of launch n + 2.  So a caller of the strip forms
 * either keeps all its launches on ONE stream, or alternates strictly between
 * TWO (launch n on stream n mod 2, what the frames in flight and the row tiling
 * do themselves): launch n + 2 is then ordered behind launch n, and launch n + 1
 * may run beside it.  Any other pattern needs the caller's own ordering (events)
 * between launches two apart.  The blocking frame call is ordered behind the
 * frames in flight.  Different contexts (one per GPU, one process per GPU) are
 * independent.
 */
#ifndef PWNHIP_H
#define PWNHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWN_OK            0
#define PWN_EINVAL       -1  /* bad argument (NULL, size, row range, w%4 with blur) */
#define PWN_ENODEV       -2  /* no usable HIP device / not gfx950 */
#define PWN_ENOMEM       -3  /* host or device allocation failed */
#define PWN_EIO          -4  /* level file could not be read (level.h:110-115) */
#define PWN_EHIP         -5  /* a HIP runtime call failed; see pwn_last_error() */
#define PWN_ENOLEVEL     -6  /* render called before a level was uploaded */
#define PWN_ETOOBIG      -7  /* sphere tables exceed PWN_TABLES_MAX (or one cell's list PWN_LIST_MAX): the per-cell lists of these spheres, kept in device memory where they outgrow
                                the on-chip (LDS) budget, would take more than 16 MiB -- 10000 spheres that each touch 3 x 3 cells need
                                about 2 MB, a sphere whose box covers the whole grid alone makes 4096 entries (pwn_sphere_tables_plan) */
#define PWN_EBUSY        -8  /* the frame slot is still in flight (pwn_wait_frame it first) */
#define PWN_ENOTSUP      -9  /* not available here (RCCL could not be loaded; not configured) */
#define PWN_ETIMEDOUT    -10 /* the row tiling waited longer than its deadline for a peer (pwn_tiled_set_timeouts); the tiling is
                                dead from then on (its communicator was aborted): pwn_tiled_shutdown, or leave the process */

typedef struct pwn_ctx pwn_ctx;

/* reference `portal` (defs.h:87-94); double1/double2 are never read */
typedef struct pwn_portal { int32_t x1, z1, x2, z2, rot12, c1, c2; } pwn_portal;

/* the arguments of obj_set(...,"sphere",...) (script.h:20-32), i.e. the live
   fields of `part.sph` (defs.h:73-79): radius, reflectivity, centre, colour b,g,r */
typedef struct pwn_sphere { float r, refl, x, y, z, cb, cg, cr; } pwn_sphere;

/* work counters of the last counted frame + device timings of the last frame */
typedef struct pwn_stats
{
	uint64_t rays;          /* trace_ray invocations            (trace.h:186) */
	uint64_t steps;         /* iterations of the cell walk      (trace.h:250) */
	uint64_t portals;       /* portal crossings                 (trace.h:576) */
	uint64_t sphere_tests;  /* sphere candidates tested         (trace.h:253) */
	uint64_t exhausted;     /* rays that ran out of maxsteps    (trace.h:677) */
	uint64_t wave_steps;    /* walk-loop iterations summed over wave64s: steps / (64 *
	                           wave_steps) = active-lane fraction of the walk loop   */
	float trace_ms;         /* trace kernel, HIP events                        */
	float blur_ms;          /* blur kernel(s), HIP events                      */
	float total_ms;         /* whole pwn_trace_screen_centred call incl. D2H   */
	float reserved_;
	/* divergence profile of the walk loop: how many wave64 iterations entered each code
	   path with at least one lane.  0 sphere list of the cell, 1 room body, 2 fog,
	   3 two-level transition (" / # / &), 4 ramp, 5 portal, 6 solid, 7 sphere hit maths */
	uint64_t wave_paths[8];
	/* PWN_SCHED_REFILL: passes of a wave64 through the shade / new-pixel / set-up phase, and the
	   lanes that had a ray to shade in them (phase_lanes / (64 * phase_passes) = their lane use) */
	uint64_t phase_passes, phase_lanes;
	/* PWN_OPT_WAVE_LOG: residency of the trace kernel's wave64s in the last frame, in ticks of the GPU's
	   constant 100 MHz clock: sum of the waves' lifetimes, first start to last end, number of waves.
	   wave_time / (waves * kernel_span) = share of the kernel's duration the average wave was resident */
	uint64_t wave_time, kernel_span, waves;
	/* counted frames: how often a wave64 entered each region of the kernel outside the walk's paths above (the issue
	   model, tools/issue_model.py; the order is trace_common.h's RG_* enum): 0 ray segment set-up, 1 its slow path, 2 exhausted
	   rays, 3 wall shading, 4 sphere shading, 5 floor normal, 6 sphere mirror, 7 jitter + push, 8 / 9 composite of the last
	   bounce and its fog, 10 / 11 of the first, 12 help-another-queue, 13 units, 14 sphere tests (list loop trips), 15
	   nearer-sphere updates, 16 walk iterations with a lane in a non-room cell, 17 units in the right half of a 32-pixel tile,
	   18 / 19 height-change block: out of a 2-high cell, and its wall test, 20 portal letters that are walls, 21 portal
	   crossings, 22 / 23 those that turn by a quarter / by a half, 24 waves of the launch */
	uint64_t regions[32];
} pwn_stats;

/* options for pwn_set_option */
#define PWN_OPT_BLUR_PASSES 1  /* POSTPROC_BLUR (defs.h:9); default 1, 0 = off */
#define PWN_OPT_COUNTERS    2  /* 1: frames also fill pwn_stats counters (slower) */
#define PWN_OPT_SCHEDULER   3  /* how the trace kernel hands pixels to the lanes of a wave64: */
#define PWN_SCHED_UNITS     0  /*   a wave traces 16x4-pixel units, all 64 lanes in step (ray set-up, walk, shading) */
#define PWN_SCHED_REFILL    1  /*   lanes whose ray ended are refilled by ballot + prefix rank while the rest walk on */
#define PWN_SCHED_DEFAULT   PWN_SCHED_UNITS
                               /*   While the sphere tables are in their device-memory form (pwn_sphere_tables_state: form 2) every launch runs
                                    the units kernel whatever this option says -- the refill kernel reads on-chip lists only.  Same frames. */
#define PWN_OPT_REFILL_LIMIT 4 /* PWN_SCHED_REFILL: lane-steps (1..64000) the ended rays of a batch may wait, in sum, for
                                  the batch's other rays before they are shaded and replaced; rays still walking
                                  then walk on beside the next batches */
#define PWN_REFILL_LIMIT_DEFAULT 256
#define PWN_OPT_WAVE_LOG     6 /* 1: every wave64 of the trace kernel stamps its start and end (two clock reads and one
                                  store per wave); pwn_get_stats then fills wave_time / kernel_span / waves */
#define PWN_OPT_FRAME_OVERLAP 7 /* frames in flight: 1 (default) = the kernels of successive frames alternate between two compute
                                  streams, so that the next frame's trace grid fills the CUs the current one's tail leaves idle
                                  and its blur runs beside it; 0 = all frames on one stream, strictly one after the other.
                                  PWN_EBUSY while frames are in flight.  A slot's frame is complete when its pwn_wait_frame
                                  returns (every slot has its own event); frames two apart complete in order, neighbours may
                                  finish either way round.  Frames f and f + 1 share nothing they write: pre-blur planes by parity,
                                  colour / depth / surface planes by slot, counter sets by launch, and the tables a frame reads are
                                  the copy that was current at its submit (four copies; an upload never touches one in use).
                                  A frame counted (PWN_OPT_COUNTERS) or wave-logged runs on one stream: one set of counters.
                                  The second stream is created at another priority level than the first so that it gets a
                                  hardware queue of its own.  The row tiling reads the option at pwn_tiled_init. */
#define PWN_OPT_TRACE_ROOM 8   /* frames on two compute streams (PWN_OPT_FRAME_OVERLAP, and the row tiling): workgroups the persistent
                                  trace grid leaves free so that the other stream's kernels find room on every CU beside it
                                  instead of waiting for its end.  -1 (default): the library measures -- windows of delivered
                                  frames with no room and with one workgroup per CU, the better kept for ~500 frames (half a second
                                  at least), then again (the answer depends on the scene: +3.5 % at 4K on level.txt, -3 % on a hall of
                                  mirrors); >= 0: that many, always.  Results never depend on it. */
#define PWN_OPT_TILED_CHOREO 10 /* row tiling, read by pwn_tiled_init (PWN_EBUSY while a tiling exists; PWN_TILED_CHOREO=split in the environment
                                  for a process).  PWN_TILED_CHOREO_INSTREAM (default): pwn_tiled_submit(f) enqueues everything of frame f --
                                  trace, halo rows, blur, gather, words -- in order on the frame's own compute stream (frames alternate between
                                  two); frame f's exchange overlaps the other stream's trace f+1 and no event crosses a queue.
                                  PWN_TILED_CHOREO_SPLIT (rounds 2-3): the exchanges on a third stream tied to the kernels by four events per
                                  frame, blur f enqueued by submit f+1 and its gather by submit f+2.  Same frames either way.  Measured on one
                                  GPU (profiles/r4/host_bound.txt): split costs a rank 0.14-0.21 ms per frame whatever the frame's
                                  size -- a strip of an 8-way tiled 4K frame needs 0.05 ms of kernels. */
#define PWN_TILED_CHOREO_INSTREAM 0
#define PWN_TILED_CHOREO_SPLIT    1
#define PWN_OPT_TILED_COMMS 12   /* row tiling over RCCL, in-stream choreography, read by pwn_tiled_init (PWN_EBUSY while a tiling exists;
                                  PWN_TILED_COMMS=perstream in the environment).  PWN_TILED_COMMS_ONE (default): one communicator for all
                                  exchanges -- it runs its grouped launches in the order they were made, so frame f+1's halo rows start
                                  behind frame f's gather although the two are on different streams.  PWN_TILED_COMMS_PER_STREAM: one
                                  communicator per compute stream (each brought up like the first, under the deadline; its id travels from
                                  rank 0 over the first): the streams' exchanges are independent.  Blocking mode only.  Never run between
                                  GPUs (nor has anything else here); on one GPU, a rank's exchange with itself: DESIGN.md 6. */
#define PWN_TILED_COMMS_ONE        1
#define PWN_TILED_COMMS_PER_STREAM 2
#define PWN_OPT_TILED_STREAMS 11 /* row tiling, in-stream choreography, read by pwn_tiled_init (PWN_EBUSY while a tiling exists; PWN_TILED_STREAMS=n
                                  in the environment): 2 = frames alternate between the context's two compute streams, 3 = they rotate
                                  over those and a third that the tiling creates -- two frames' exchanges and blurs then overlap a third
                                  frame's trace.  Same frames.  Without PWN_OPT_FRAME_OVERLAP there is one stream whatever this says. */
#define PWN_OPT_UNIT_ORDER 9   /* 0 (default): the trace kernel hands its 16 x 4-pixel units out in arithmetic order, rows from the frame's
                                  middle row outwards.  1 (PWN_UNIT_ORDER=1 in the environment for a process): dearest first -- every unit's cost
                                  (the time its wave spent on it) is written by the launch, put in order per work queue behind the frame's last
                                  kernel (a counting sort, ~3 us), and used by the next launch of the same rows on that stream, so that the units
                                  handed out last are the cheap ones.  Measured (profiles/r4/unit_order_ab.txt): a launch of a few units per wave
                                  that runs alone gets shorter (720p -9 %, a middle strip of an 8-way 4K tiling -10 %), long launches and frames
                                  on two streams get slower (4K +2 ... +4 %): sorted by cost, units of one kind share a SIMD.  Hence off.  The
                                  first launch of a geometry uses the arithmetic order; with the strip forms the sort rides behind
                                  pwn_blur_rows_device[_bounded] on the caller's stream.  Any order gives the same pixels.  The reference's
                                  counterpart is OpenMP's static schedule over 32-row chunks (screen.h:63-64). */
#define PWN_OPT_CALL_STRIPS 13 /* the blocking call, pwn_trace_screen_centred (the one call an unchanged reference loop makes per frame,
                                  main.c:107): handing a 4K frame to the host over PCIe takes twice as long as its kernels, so the call
                                  works in row strips -- strip k is traced while strip k - 1 is blurred from the rows traced so far and
                                  strip k - 2 travels to sbuf / zbuf on the copy stream.  A tap of the blur that lands below the rows
                                  traced so far (taps reach 0.002*h*|depth-1| rows, screen.h:100-102; a strip is blurred where taps of
                                  depth <= 8 are covered) is counted; such a frame's blur is repeated over the whole frame before the call
                                  returns and the next calls cover depth 24; a frame that exceeds that too sends the next calls through in
                                  one piece for a while: the frame delivered is always the exact one.  -1 (default): strips for frames of 3 Mpixels
                                  and more into registered buffers (pwn_host_register), of 6 Mpixels and more into others, with
                                  POSTPROC_BLUR 0 or 1, not for counted or wave-logged frames; 0: one launch per pass,
                                  then the copies (what pwn_stats.trace_ms / blur_ms time as single launches); 2..32: that many
                                  strips whatever the size.  With strips pwn_stats.trace_ms runs from the first strip's trace to the
                                  end of the last one's (the blurs between them included), blur_ms is the tail behind it. */
#define PWN_OPT_FRAME_TIMING 5 /* frames in flight: record HIP events around the trace and blur kernels of every N-th
                                  frame (pwn_frame.timed, .trace_ms ...); 1 = every frame (default), 0 = never.  An event
                                  between two kernels costs a few microseconds of pipeline */

/*
 * Replaces the buffer/global set-up of main.c:26-34,395-400 (rwidth, rheight,
 * sbuf, tsbuf, zbuf).  `device` is the HIP ordinal.  Device depth is
 * zero-initialised; like the reference's zbuf it keeps its previous value at
 * pixels whose primary ray exhausts maxsteps (trace.h:677).
 */
int pwn_init(pwn_ctx **out, int device, int width, int height);
void pwn_destroy(pwn_ctx *ctx);
/*
 * The same for several GPUs of ONE process.  The reference's host is one process with one loop (main.c:93-109) whose row
 * parallelism -- the OpenMP pragmas of screen.h:63-67,77 -- is invisible to it; so is this: the handle is used exactly
 * like pwn_init's (the level and object calls, pwn_trace_screen_centred, the frames in flight, pwn_screen_upscale,
 * pwn_get_stats, pwn_host_register), and every frame is row-tiled over the devices behind it -- the choreography of
 * pwn_tiled_* (strip per device, halo rows to the neighbours, bounded blur with exact repeat, moving cuts), driven by one
 * library-owned thread per device, the devices' tables filled from the one level and object table of the handle.  No
 * unique id, no second process, no replicated game state.
 *   devices[ndev]   HIP ordinals, 1..PWN_TILED_MAX_WORLD of them.  The same ordinal may appear more than once: so many
 *                   members share that device (tests on a box with one GPU; no use otherwise).  ndev = 1 is pwn_init.
 *   frames          pwn_trace_screen_centred: every device copies its finished strip (and its depth strip) straight into the
 *                   caller's sbuf / zbuf over its own PCIe link.  pwn_frames_config with PWN_FRAME_SBUF / _ZBUF: the same
 *                   into the group's pinned frames, up to PWN_MAX_SLOTS in flight; PWN_FRAME_SURFACE: every device upscales its own
 *                   strip (screen_upscale, screen.h:126-149) and copies those rows of the surface to the host as well; with flags 0
 *                   the finished strips are gathered on devices[0] (pwn_frame.d_sbuf) and nothing goes to the host.
 *   exchange        between devices: RCCL (ncclSend / ncclRecv groups over xGMI, one communicator rank per device, made
 *                   in-process under the bring-up deadline) when the ordinals are distinct and librccl loads, else -- and
 *                   with PWN_GROUP_TRANSPORT=local in the environment -- PWN_TRANSPORT_LOCAL: peer-to-peer copies behind
 *                   events.  pwn_group_info says which.
 *   errors          1. A refusal is not a failure.  A call that a pwn_init handle refuses with the same arguments in the same state
 *                   (PWN_EINVAL, PWN_EBUSY, PWN_ENOLEVEL, PWN_ENOTSUP, PWN_EIO, PWN_ETOOBIG) returns the same code here and leaves the
 *                   handle as it was: the next call of any kind returns what it would have returned without it, frames in flight are
 *                   delivered, the tiling in force stays in force (pwn_group_info's transport, note, cuts, halo_rows, host_sink,
 *                   frames are what they were).  pwn_last_error after a later successful call may be anything.  A group's own
 *                   refusals are of the same kind: PWN_OPT_BLUR_PASSES above 1 and pwn_screen_upscale(NULL, ...) before a blocking
 *                   call has delivered a frame (PWN_EINVAL), pwn_trace_screen_centred and the options a tiling fixes
 *                   (PWN_OPT_BLUR_PASSES, _FRAME_OVERLAP, _TILED_*) with frames in flight (PWN_EBUSY), pwn_tiled_* and the strip
 *                   forms (PWN_ENOTSUP).
 *                   2. A real failure breaks the group and is mended.  A member past its deadline (PWN_ETIMEDOUT after
 *                   pwn_tiled_set_timeouts' limits, which the handle takes too), a transport error, PWN_EHIP / PWN_ENOMEM, and
 *                   whatever leaves the members in different states (a sphere upload that one member could not allocate for, a
 *                   frame that failed on one member after others had enqueued it, a table call refused by one member only): the
 *                   first call that waits for the members reports it, pwn_last_error naming the member; the tiling goes down, and
 *                   the next frame call brings it up again (its depth planes start from zero, as after pwn_frames_config).  After
 *                   a failed table upload the host uploads again; from then on the frames are one device's.
 *                   3. A lost frame is reported per slot.  After a real failure with frames in flight, pwn_wait_frame returns that
 *                   failure's code once for every slot whose frame was lost (a frame that had reached the host's frames before
 *                   is delivered); *out is not written, and the slot is then free -- a further wait without a submit is
 *                   PWN_EINVAL, as for a slot never submitted.  pwn_frame_ready of a lost slot returns the code, never 1.  It is
 *                   never PWN_OK with NULL planes.
 *                   Not covered: a member's thread that never returns from a HIP or RCCL call holds the call that waits for it.
 * pwn_tiled_* (other than set_timeouts) and the strip forms are refused on such a handle (PWN_ENOTSUP): it runs its own tiling.
 */
typedef struct pwn_group_info
{
	int members, transport;                  /* PWN_TRANSPORT_RCCL or _LOCAL */
	int devices[64];                         /* the ordinals as given (PWN_TILED_MAX_WORLD) */
	int cuts[65];                            /* member m traces rows [cuts[m], cuts[m + 1]) of the next frame */
	int halo_rows, host_sink;                /* of the tiling in force (0, 0 before the first frame) */
	uint64_t frames, frames_redone, recuts;  /* delivered; repeated with whole strips; how often the cuts moved */
	char note[160];                          /* why the transport is not RCCL (members on one device; librccl did not load; its
	                                            bring-up between the members failed -- the group then goes on with copies, once, unless
	                                            PWN_GROUP_TRANSPORT named the transport), or empty */
} pwn_group_info;
int pwn_init_multi(pwn_ctx **out, const int *devices, int ndev, int width, int height);
int pwn_group_info_get(pwn_ctx *ctx, pwn_group_info *out);
int pwn_set_option(pwn_ctx *ctx, int option, int value);
/* (PWN_OPT_UNIT_ORDER is ignored while the sphere tables are in their device-memory form, pwn_sphere_tables_state: form 2 -- those
   kernels hand their units out in arithmetic order and write no costs.  Same frames.) */
/* PWN_OPT_UNIT_ORDER as it stands: out[0] the option, out[1] trace launches so far that handed their units out in a sorted order,
   out[2] sorts launched (one behind every frame whose trace wrote its units' costs), out[3] units the first compute stream's
   current order covers (0: none yet). */
int pwn_unit_order_state(pwn_ctx *ctx, unsigned long long out[4]);
/* the sort by itself (tests): `units` costs in (host memory), the order out -- perm_out holds 64 * cap entries, cap = ceil(units / 64);
   queue q's units, dearest first, are perm_out[q * cap .. q * cap + its length), the rest of its row is left 0xffffffff */
int pwn_unit_order_probe(pwn_ctx *ctx, const uint16_t *cost, uint32_t units, uint32_t *perm_out);
/* Trace launches of a context take their work-queue counters from sets used in turn, and launch n resets the set of launch n - R
   (R = 2; 3 for a tiling on three compute streams): launches R apart have to be ordered.  On one stream, and with frames rotating over
   R streams, they are by themselves; a launch that leaves the rotation (pwn_trace_screen_centred behind frames in flight, a counted
   frame) is put behind the launch R before it with an event.  *out = how often that happened (tests). */
int pwn_launch_order_waits(pwn_ctx *ctx, unsigned long long *out);
/* PWN_OPT_TRACE_ROOM as it stands: out[0] the option's value (-1 = measuring), out[1] the workgroups the next two-stream trace launch
   leaves free, out[2] how often the two settings were compared, out[3] how often the setting changed */
int pwn_trace_room_state(pwn_ctx *ctx, int out[4]);
const char *pwn_strerror(int code);
const char *pwn_last_error(pwn_ctx *ctx);

/* level_load (level.h:107-228): parse the ASCII grid (CR/LF rules, '*' spawn,
   lower-case portal quirk), build pmap, upload.  */
int pwn_level_load(pwn_ctx *ctx, const char *path);
int pwn_level_load_mem(pwn_ctx *ctx, const char *text, int len);
/* the same tables handed over ready-made: lv->data / lv->pmap (defs.h:103-105), also as level_load leaves them (x == -1 for
   an endpoint never seen, with whatever z).  PWN_EINVAL for a coordinate outside -1 .. 63, and for a hand-made table on which
   a ray in a cell OUTSIDE the grid, at coordinate -1, would stand on an endpoint and see or do something there: a paired
   letter with an endpoint at (-1, z) or (x, -1) that stands in the column-0 / row-0 cell read for that cell, or a '#', '&', '"'
   far side (c1 / c2) behind such an endpoint (level_host.c: pwn_check_portals) */
int pwn_upload_level(pwn_ctx *ctx, const uint8_t data[4096], const pwn_portal pmap[26]);
int pwn_get_level(pwn_ctx *ctx, uint8_t data[4096], pwn_portal pmap[26], int32_t spawn[2]);

/* level_prepare_render (level.h:64-81) + level_part_add_bbox (level.h:1-19):
   bins the live spheres per cell in object order and uploads the lists.
   Any table up to PWN_OBJ_MAX spheres loads, as in the reference.  Lists that fit the on-chip budget are copied into LDS by every
   workgroup, in the form and with the kernels they always had; lists that do not (more than 2047 spheres, more than 32767 list
   entries, more than 72 KiB in all) stay in device memory and are read from there by kernels of their own, for every call of this
   file -- frames, frames in flight, strips, views, rays, hits, the row tiling, groups -- with the same pixels, depths, records and
   counters.  Only tables whose device-memory part would exceed PWN_TABLES_MAX, or with more than PWN_LIST_MAX spheres binned to one
   cell, are refused (PWN_ETOOBIG); a refused or failed
   upload leaves the previous tables in force.  The device-memory part and its pinned staging are allocated with the first tables
   that need them and grown to the largest so far; an upload that has to grow a device buffer synchronises the device once (a
   launch in flight may still read the buffer it replaces), one that fits waits for nothing, as before. */
int pwn_upload_spheres(pwn_ctx *ctx, const pwn_sphere *spheres, int n);
int pwn_get_bins(pwn_ctx *ctx, uint16_t counts[4096], int32_t *idx, int cap);
#define PWN_TABLES_MAX (16u << 20)   /* bytes of the sphere tables' device-memory part at most */
#define PWN_LIST_MAX 4096            /* ... and spheres binned to ONE cell at most, for tables in device memory: every step of every ray through a
                                        cell tests the cell's whole list (trace.h:252-296), up to 1000 steps a segment, so a list bounds how long a
                                        launch can run.  Thousands of spheres piled into one cell stay PWN_ETOOBIG, as they always were; the reference's
                                        scenes and 10000 spheres spread over a level are nowhere near (pwn_sphere_tables_plan: out[5]) */
/* What an upload of these n spheres would do, under the default scheduler (and PWN_SPHERE_LISTS=indexed|inline|global of the
   environment, which every context of the process follows: tests, experiments).  Host only: no context, no device.
     out[0]  form of the per-cell lists: 0 indexed, 1 inline records (both in LDS), 2 in device memory
     out[1]  LDS bytes per workgroup of the units kernel (the tables' on-chip part and the kernel's own 16 bytes)
     out[2]  bytes in device memory beside that (0 for forms 0 and 1): 16 per (cell, sphere) pair and 16 more, 4 per pair, 32 per
             sphere, each section rounded up to 16
     out[3]  (cell, sphere) pairs    out[4]  non-empty cells    out[5]  the longest cell list
   PWN_OK; PWN_ETOOBIG (out is filled in all the same); PWN_EINVAL for NULL spheres or out, n < 0, n > PWN_OBJ_MAX. */
int pwn_sphere_tables_plan(const pwn_sphere *spheres, int n, unsigned long long out[6]);
/* The bounding balls the next upload of these n spheres would make, under the default scheduler (and PWN_SPHERE_LISTS, as above): the
   trace kernels skip a cell's whole sphere list for a wave none of whose rays can meet the list's ball.  At most PWN_BOUNDS_MAX
   lists get one -- those with the most records, of equally long ones the lower cell first, none shorter than four records; a list
   with a member that is not finite, further out than 1024 on an axis, or more than 1.5 from the members' mean including its
   radius gets none.  Host only.  Returns how many balls there are (out[i] for the rest is zero), or PWN_EINVAL / PWN_ETOOBIG /
   PWN_ENOMEM as pwn_sphere_tables_plan.  PWN_SPHERE_BOUNDS=0 in the environment makes every context of the process launch without
   them (tests, A/B); this function reports them all the same.
     out[i][0]  the list's cell, z * 64 + x    out[i][1]  its records    out[i][2]  the list's id in the cell word (bits 16..30)
     out[i][3..5]  centre x, y, z (fp32 values)    out[i][6]  effective radius    out[i][7]  its square as the kernel compares it */
#define PWN_BOUNDS_MAX 4
int pwn_sphere_bounds_plan(const pwn_sphere *spheres, int n, double out[PWN_BOUNDS_MAX][8]);
/* The same six values for the tables in force in this context, under its scheduler (a pwn_init_multi handle: member 0's). */
int pwn_sphere_tables_state(pwn_ctx *ctx, unsigned long long out[6]);

/*
 * The sphere tables built on the device: pwn_upload_spheres for spheres that are already in device memory, on the caller's
 * stream, with no host round trip -- the other players of an arena drawn as spheres, a projectile, anything a policy moves.
 *   what                 d_spheres holds n records of pwn_sphere (8 floats, 32 B: r, refl, x, y, z, cb, cg, cr), 16-byte aligned, in
 *                        device memory.  The call bins them as level_prepare_render does (level.h:64-81: object order inside a
 *                        cell, cells outside the grid skipped), builds a full copy of the tables in the lists' device-memory form
 *                        (pwn_sphere_tables_state: form 2) and makes that copy the tables in force.  pwn_hit.object and the label
 *                        planes' object field index d_spheres' order.  d_spheres is read by the call's own launches only: in stream
 *                        order the caller may overwrite it afterwards.
 *   capacity             the host cannot know the lists' sizes, so the caller declares them: max_pairs is the most (cell, sphere)
 *                        pairs the tables may hold.  The on-chip part is then laid out for min(4096, max_pairs) non-empty cells and
 *                        the device-memory part for max_pairs records and n spheres (16 B a pair and 16 more, 4 B a pair, 32 B a
 *                        sphere, each section rounded up to 16).  Tables with max_pairs >= 4096 take 42 KB of LDS per workgroup
 *                        (three workgroups per CU), whatever the spheres are.
 *   overflow             the device cannot refuse.  Spheres that make more than max_pairs pairs, or one cell's list longer than
 *                        PWN_LIST_MAX, put tables WITHOUT ANY sphere into force -- exactly the tables of n = 0 -- and
 *                        pwn_spheres_device_state says why.  Nothing is truncated, nothing is read or written out of range.
 *   exactness            with these tables every call family -- frames, frames in flight, strips, views, viewports, rays, hits, view
 *                        hits, their device forms, the five counters -- returns bit for bit what it returns after pwn_upload_spheres of
 *                        the same n spheres.  Such tables carry no bounding balls (pwn_sphere_bounds_plan); results and counters never
 *                        depend on those.  This holds for every bit pattern in the records: NaN, infinities, coordinates and radii
 *                        beyond int, negative and denormal radii, r * r below FLT_MIN stored as 0.  The box is (int)(x - r) etc. as
 *                        the x86 build computes it (INT_MIN for NaN and anything outside int), then clamped; positions, refl and
 *                        colours are moved, not computed with.  Every address comes from counted values and the clamped box: no
 *                        input bit pattern reaches one.
 *   ordering             at most FIVE launches on `stream` (a hipStream_t, NULL = the default stream): four of the build, and in the
 *                        first call after a level change one more that brings the level's part of the tables (static head, baked
 *                        cell words, portal records) into a device-resident base copy from one pinned slot.  No host wait, no
 *                        synchronisation and, from the second call of a level on, no copy from host memory.  Trace launches and
 *                        players' steps made after the call returns read the new tables, on any stream: they are put behind the
 *                        build as they are put behind an upload.  Launches made before it keep the copy they were given.  The build
 *                        takes the next of the four copies of the tables and waits ON `stream` for the launches and steps that
 *                        still read that copy.  The walk table of the players' step is handed on as an upload of spheres alone
 *                        hands it on.  Builds of one context on different streams are put behind each other.  No work-queue
 *                        counters are used and the launch rotation is not entered.
 *   memory               the context's: the copies' device-memory parts grow to the largest need so far.  A call that needs more
 *                        than any before allocates and may synchronise the device once, as pwn_upload_spheres does; a call that
 *                        fits allocates nothing.  The first call of a context allocates the builder's scratch (74 KB) and the base
 *                        copy (25 KB on the device and pinned).  pwn_destroy frees them.
 *   in force until       the next call that builds tables from the host's object table: pwn_upload_spheres, pwn_prepare_render,
 *                        pwn_level_load, pwn_level_load_mem, pwn_upload_level, which behave exactly as they always did.
 *                        pwn_set_option never replaces them: under PWN_SCHED_REFILL they run the units kernel, as form 2 always
 *                        does, and a change of scheduler repacks nothing.  pwn_get_objects, pwn_get_object_ids and pwn_get_bins go
 *                        on describing the host's table.  pwn_sphere_tables_state reports out[0] = 2, out[1] and out[2] as laid out
 *                        above, out[3..5] the capacity's bounds: max_pairs, min(4096, max_pairs), min(PWN_LIST_MAX, max_pairs).
 *   left alone           everything pwn_players_step leaves alone, pwn_stats and pwn_launch_order_waits included.
 *   cost                 measured on an MI355X (profiles/spheres_device/bench.txt): the call 35 us for up to 64
 *                        spheres, 43 us for 1024, 99 us for 10000, against 53 to 325 us for copying the records down,
 *                        pwn_upload_spheres and the wait for its upload.  The trace pays for the device-memory form (one 16-byte
 *                        global load per sphere test where the on-chip forms make an LDS read) and for its LDS: the blocking
 *                        call's trace time at 3840x2160 was +2.4 % on level.txt's 14 spheres and -0.1 % on synth64's 64 with
 *                        max_pairs = 4096, differences the measurement does not resolve below a few per cent.
 *   errors               PWN_EINVAL for a NULL ctx, n < 0, n > PWN_OBJ_MAX, max_pairs < 0, a NULL or misaligned d_spheres with
 *                        n > 0; PWN_ETOOBIG when the device-memory part as laid out above exceeds PWN_TABLES_MAX; PWN_ENOLEVEL before
 *                        a level; PWN_ENOTSUP on a pwn_init_multi handle; PWN_EBUSY while the context runs a row tiling; PWN_ENOMEM
 *                        when a buffer cannot grow.  n == 0 is PWN_OK and puts empty tables into force (it still takes the next
 *                        copy).  A refused call launches nothing and leaves the tables in force as they were.
 *   pwn_spheres_device_state   BLOCKS: waits for the last build.  For tests and for hosts that size max_pairs.
 *                        out[0]  1 if device-built tables are in force, else 0
 *                        out[1]  n of the last build            out[2]  max_pairs of the last build
 *                        out[3]  the pairs the spheres made (the full count also when over capacity)
 *                        out[4]  non-empty cells                out[5]  the longest list
 *                        out[6]  0 = built, 1 = more pairs than max_pairs, 2 = a list longer than PWN_LIST_MAX
 *                        out[7]  device uploads so far
 *                        All eight are 0 before any device upload.  PWN_EINVAL for a NULL ctx or out, PWN_ENOTSUP on a
 *                        pwn_init_multi handle, PWN_EBUSY under a row tiling.
 */
int pwn_upload_spheres_device(pwn_ctx *ctx, int n, const void *d_spheres, int max_pairs, void *stream);
int pwn_spheres_device_state(pwn_ctx *ctx, unsigned long long out[8]);

/*
 * The level's tables baked on the device: pwn_upload_level for a grid that is already in device memory, on the caller's stream, with
 * no host round trip -- an arena generated at every episode reset, a door a policy opens, a wall a projectile removes.  (The
 * reference's script interface names the operation and leaves it a stub: level_set, script.h:65-69.)
 *   what                 d_data holds 4096 cell bytes, z * 64 + x, the layout of pwn_upload_level's data; d_pmap 26 records of
 *                        pwn_portal (7 int32 each) or NULL.  Both in device memory, 16-byte aligned, read by the call's own launches
 *                        only: in stream order the caller may overwrite them afterwards.  No byte of the grid is special: '*', CR,
 *                        LF and lower-case letters are cells like any other (their text meaning belongs to the parser).
 *   d_pmap given         the level in force becomes bit for bit what pwn_upload_level(data, pmap) followed by pwn_upload_spheres(NULL, 0)
 *                        puts into force, for every call family of this header and pwn_players_step[_device]: results, records,
 *                        depth, the five counters.  c1 / c2 are taken by their low byte and rot12 by & 3, as the host does.
 *   d_pmap NULL          the portal table is derived on the device from the cells as stored, the way pwn_level_load derives it: the
 *                        first two cells holding a letter, in scan order (z major, then x), are its endpoints 1 and 2, a third sighting
 *                        is ignored; for a letter with both, rot12 = (d2 - d1 + 2) & 3 with the directions' order +x, +z, -x, -z and
 *                        the fall-back to +x, and c1 / c2 are the cell in that direction, read through the FLAT 4096-byte array (x = 64
 *                        aliases the next row, a read outside the array is '.'); a letter with fewer than two sightings keeps
 *                        coordinates -1, rot12 0, c1 = c2 = ';' for what it lacks.  For a grid holding none of CR, LF, '*',
 *                        'a'..'y' the result is bit for bit what pwn_level_load_mem(those 4096 bytes, 4096) puts into force, and
 *                        pwn_get_level_device returns the same 26 x 7 int32 as pwn_get_level (full rows need no line end).
 *   the device cannot refuse   a given table that pwn_upload_level would refuse -- a coordinate outside -1 .. 63, or a cell outside
 *                        the grid at coordinate -1 that would stand on an endpoint and see or do something there -- leaves the LEVEL
 *                        that was in force in force, and pwn_level_device_state says why.  The checks run first, on the 26 x 4
 *                        coordinates as integers and on the 130 cells outside the grid; no bit pattern of d_pmap or d_data reaches
 *                        an address, a loop bound or a shift count before it has passed them.  Endpoints are compared with cell
 *                        coordinates, never used as indices; a derived table's coordinates are the kernel's own and always pass.
 *   spheres              either way the call puts tables WITHOUT any sphere into force, exactly what
 *                        pwn_upload_spheres_device(n = 0, max_pairs = 0) makes.  Follow it with pwn_upload_spheres_device on the same
 *                        stream.
 *   ordering             FIVE launches on `stream` (a hipStream_t, NULL = the default stream): one that derives, checks, bakes and
 *                        commits, and the four of a sphere-less build; in a context's first device build one more, which brings the
 *                        static head of the tables into the device-resident base copy.  No host wait, no synchronisation and, after
 *                        that first build, no copy from host memory.  The bake waits ON `stream` for the device builds that still
 *                        read the base copy, for the launches and steps that still read the copy of the tables it takes, and for
 *                        the upload stream as it stands (its walk table goes into a buffer no other copy refers to, whose readers
 *                        the upload stream is behind).  Trace launches and players' steps made after the call returns read the new
 *                        level, on any stream; launches made before it keep the copy they were given; later host uploads stay
 *                        ordered behind the call.  No work-queue counters are used and the launch rotation is not entered.
 *   in force until       the next call that builds tables from the host's level or object table: pwn_level_load, pwn_level_load_mem,
 *                        pwn_upload_level, pwn_upload_spheres, pwn_prepare_render, which behave exactly as they always did and put
 *                        the HOST's level back.  pwn_upload_spheres_device keeps the device level.  pwn_get_level, pwn_level_get,
 *                        the spawn, pwn_get_objects and pwn_get_bins go on describing the host's state.  pwn_set_option never
 *                        repacks while device tables are in force.
 *   left alone           everything pwn_upload_spheres_device leaves alone.
 *   memory               the builder's buffers of pwn_upload_spheres_device, and 32 bytes of status words.
 *   cost                 measured on an MI355X (profiles/level_device/bench.txt): the call 52 us alone and 54 to 56 us
 *                        back to back on the three shipped levels, given or derived table alike, against 67 to 71 us for copying
 *                        the grid and the table down, pwn_upload_level and the wait for its upload.
 *   errors               PWN_EINVAL for a NULL ctx, a NULL or misaligned d_data, a misaligned d_pmap; PWN_ENOLEVEL before a first
 *                        level (a context gets its static tables with its first host level); PWN_ENOTSUP on a pwn_init_multi
 *                        handle; PWN_EBUSY under a row tiling; PWN_ENOMEM.  A refused call launches nothing and changes nothing.
 *   pwn_level_device_state   BLOCKS until the last device level build is done.  All eight words are 0 before any such build.
 *                        out[0]  1 if a device-built level is in force
 *                        out[1]  device level uploads so far
 *                        out[2]  the last build's verdict: 0 taken, 1 a coordinate outside -1 .. 63, 2 the rule for cells outside the grid
 *                        out[3]  the lowest letter that offends against that rule, 0 .. 25, else 26
 *                        out[4]  endpoint records baked           out[5]  letters with both endpoints
 *                        out[6]  1 if the table was derived       out[7]  0
 *                        PWN_EINVAL for a NULL ctx or out, PWN_ENOTSUP on a pwn_init_multi handle, PWN_EBUSY under a row tiling.
 *   pwn_get_level_device   BLOCKS.  The cells and the portal table (as given, or as derived) of the device-built level in force,
 *                        read from its walk table; either pointer may be NULL.  PWN_EINVAL when none is in force.
 */
int pwn_upload_level_device(pwn_ctx *ctx, const void *d_data, const void *d_pmap, void *stream);
int pwn_level_device_state(pwn_ctx *ctx, unsigned long long out[8]);
int pwn_get_level_device(pwn_ctx *ctx, uint8_t data[4096], pwn_portal pmap[26]);

/*
 * The object table behind those lists, driven the way game.lua drives the
 * reference (script.h:1-64): lv->objs[OBJ_MAX] (defs.h:4,98-99).
 *   pwn_obj_new        level_obj_new (level.h:41-62): first freed slot, else
 *                      append; returns the object's index, PWN_ENOMEM when all
 *                      PWN_OBJ_MAX slots are taken (the reference returns NULL)
 *   pwn_obj_set_sphere obj_set(o, "sphere", r, refl, x, y, z, b, g, r)
 *                      (script.h:10-40); Lua numbers are doubles and are
 *                      narrowed to float on store, as there
 *   pwn_obj_free       obj_free (script.h:42-51): the slot becomes reusable.  As with
 *                      the reference's part pointers the handle stays usable:
 *                      obj_set on a freed slot makes it a sphere again (script.h:24
 *                      sets pt->typ whatever it was), obj_free on it changes nothing
 *   pwn_level_get      level_get(cx, cz) (script.h:53-64): the cell character
 *                      under get_cell's clamp (util.h:151-158)
 *   pwn_prepare_render level_prepare_render (level.h:64-81): bin every object
 *                      that is not free, in table order, and upload (all PWN_OBJ_MAX
 *                      of them if need be: see pwn_upload_spheres); an object
 *                      that was created but never set is PWN_EINVAL (the
 *                      reference aborts, level.h:34-37)
 *   pwn_get_objects    the live spheres in table order (at most cap); returns
 *                      their number
 * pwn_upload_spheres replaces the whole table by n set spheres.
 */
#define PWN_OBJ_MAX 10000
int pwn_obj_new(pwn_ctx *ctx);
int pwn_obj_set_sphere(pwn_ctx *ctx, int obj, double r, double refl, double x, double y, double z,
	double cb, double cg, double cr);
int pwn_obj_free(pwn_ctx *ctx, int obj);
int pwn_level_get(pwn_ctx *ctx, int cx, int cz);
int pwn_prepare_render(pwn_ctx *ctx);
int pwn_get_objects(pwn_ctx *ctx, pwn_sphere *out, int cap);

/*
 * trace_screen_centred(lv, 0, 0, rwidth, rheight, &cam) (screen.h:31-124,
 * called at main.c:107) with sec_current (defs.h:23) passed explicitly.
 * cam = mat4 rows x,y,z,w (defs.h:46-52).  Blocking.  Fills the caller's
 * host sbuf (BGRA8, pitch = width) and, if not NULL, zbuf -- the layouts of
 * main.c:31,33.
 */
int pwn_trace_screen_centred(pwn_ctx *ctx, const float cam[16], float sec_current,
	uint32_t *sbuf, float *zbuf);
/*
 * The host's frame buffers are malloc'ed once and live as long as the process (main.c:395-400).  Made known to the
 * device once (hipHostRegister), the copies of the blocking call into them are plain DMA that runs beside the kernels
 * of the frame's later strips and never holds the calling thread; into memory that is not registered every strip's
 * copy is staged by the runtime and blocks the caller while it runs (the call then keeps two strips of kernels
 * enqueued ahead of the copy it waits in).  Same pixels either way.
 *   pwn_host_register    [base, base + bytes): once, right after the malloc; PWN_EBUSY when PWN_HOST_REGS_MAX (16)
 *                        ranges are registered, PWN_EHIP when the runtime refuses (the range stays usable, unregistered)
 *   pwn_host_unregister  before the memory is freed -- a registered range that is freed and handed out again by
 *                        malloc is still the OLD pages to the device; pwn_destroy unregisters what is left
 * *_state: out[0] the option, out[1] strips of the last blocking call (1 = it ran in one piece), out[2] blocking calls
 * that ran in strips, out[3] how many of those had their blur repeated over the whole frame, out[4] the copy streams the
 * chunks go out on (1 or 2; 0 = the context is still finding out: its first 8 calls in strips use one, the next 8 two, the
 * faster stays -- which it is depends on the queues the runtime handed out; PWN_CALL_COPY_STREAMS=1|2 in the environment
 * fixes it), out[5] the depth whose taps a chunk's blur waits for (8, or 24 after a frame whose taps went further).
 */
int pwn_host_register(pwn_ctx *ctx, void *base, size_t bytes);
int pwn_host_unregister(pwn_ctx *ctx, void *base);
int pwn_call_strips_state(pwn_ctx *ctx, unsigned long long out[6]);

/*
 * trace_screen_centred (screen.h:31-124) once per view, for n views of the one level and object table: split-screen,
 * camera or portal previews, stereo pairs, many poses.  Blocking; one trace launch and one blur launch per pass for the
 * whole batch.  cams = n x 16 floats (view i's mat4 rows x,y,z,w as for pwn_trace_screen_centred), secs = n sec_current;
 * sbuf = n x h x w BGRA8 and zbuf (or NULL) = n x h x w depth, view-major.  View i is bit-identical, colour and depth, to
 * pwn_trace_screen_centred(cams[i], secs[i]) on a context of the same size, level and objects whose earlier frames were
 * view slot i's earlier cameras.
 *   depth per view slot  view slot i has a device depth plane of its own, zero when first allocated; where the primary ray
 *                        runs out of steps it keeps its previous value (trace.h:677).  Planes persist by index across calls;
 *                        a larger n keeps the existing ones; pwn_destroy frees them.  Cost: 12 B x n x w x h on the device
 *                        (pre-blur, colour, depth), allocated by the first call with that many views.
 *   blur                 PWN_OPT_BLUR_PASSES as the blocking call; PWN_EINVAL for w % 4 != 0 with blur on.
 *   counters             with PWN_OPT_COUNTERS on, pwn_get_stats returns the counters summed over the views; trace_ms,
 *                        blur_ms and total_ms time the batch call.
 *   ordering             behind the frames in flight, as the blocking call.
 *   left alone           the blocking call's own planes (its depth persistence, and pwn_screen_upscale(NULL, ...), still
 *                        refer to the last blocking frame), the unit-order state, the trace-room measurement.
 *   not followed         always the units scheduler, whatever PWN_OPT_SCHEDULER says; never in row strips
 *                        (PWN_OPT_CALL_STRIPS); PWN_OPT_UNIT_ORDER and PWN_OPT_WAVE_LOG are ignored.
 *   errors               PWN_EINVAL for NULL ctx / cams / secs / sbuf, n < 1, n > PWN_VIEWS_MAX, n x w x h > 2^28;
 *                        PWN_ENOLEVEL before a level; PWN_ENOTSUP on a pwn_init_multi handle; PWN_EBUSY while the context
 *                        runs a row tiling (pwn_tiled_init).
 */
#define PWN_VIEWS_MAX 1024
int pwn_trace_views(pwn_ctx *ctx, int n, const float *cams, const float *secs, uint32_t *sbuf, float *zbuf);
/*
 * The device form: the same n views from cameras in device memory into planes in device memory, stream-ordered on `stream` (a
 * hipStream_t, NULL = default stream) like pwn_trace_rays_device -- no synchronisation, no host copy.  Observations of many agents
 * as tensors, previews composited on the device.
 *   d_cams, d_secs       n x 16 floats (rows x,y,z,w as above) and n floats.
 *   d_sbuf               n x h x w BGRA8, view-major: the finished views.
 *   d_zbuf               n x h x w floats, required, in / out: the CALLER's depth planes stand where the host form has its view
 *                        slots.  A primary ray that runs out of steps keeps what the plane holds (trace.h:677), as a ray of
 *                        pwn_trace_rays keeps its depth.
 *   d_work               n x h x w words of scratch: required when PWN_OPT_BLUR_PASSES > 0, may be NULL when it is 0.  The trace
 *                        writes whichever of d_work / d_sbuf makes the last blur pass land in d_sbuf (d_work for an odd number of
 *                        passes); what d_work holds afterwards is unspecified.
 *                        All five pointers are 16-byte aligned.
 *   launches             one camera set-up launch, one trace launch, one blur launch per pass, all on `stream`.  The trace launch
 *                        falls under the rule for trace launches at the top of this file.
 *   exactness            view i is bit-identical, colour and depth, to view i of pwn_trace_views with the same cameras, times and
 *                        PWN_OPT_BLUR_PASSES, provided d_zbuf on entry holds what that call's view slots held (zero for a fresh
 *                        context) -- and so to pwn_trace_screen_centred.  The camera set-up runs on the device with the host's
 *                        arithmetic, operation for operation, denormals kept.
 *   w lanes              cameras with w components need PWN_VIEWS_HAS_W; without it the w lanes are taken as 0, 0, 0, 1 whatever
 *                        the cameras hold (as PWN_RAYS_HAS_W).  PWN_DBG_FORCE_HASW forces the 4-lane variants and changes nothing.
 *   records              the view records are the library's: PWN_VIEWS_MAX per set of work-queue counters (480 KB in all), allocated
 *                        by the first call, freed by pwn_destroy.  A launch uses the records of the counter set it counts in, so a
 *                        launch that may run beside it on the other stream never shares them.
 *   counters             as pwn_trace_rays_device: with PWN_OPT_COUNTERS on the counting variant runs, summed over the views.  The
 *                        call sets no timings.
 *   not followed         as pwn_trace_views.
 *   left alone           what pwn_trace_views leaves alone, and its view slots, the planes of pwn_trace_viewports and the
 *                        call-strips calibration window.
 *   errors               PWN_EINVAL for NULL ctx / d_cams / d_secs / d_sbuf / d_zbuf, NULL d_work with blur on, n < 1,
 *                        n > PWN_VIEWS_MAX, n x w x h > 2^28, flags other than PWN_VIEWS_HAS_W, a pointer that is not 16-byte
 *                        aligned, w % 4 != 0 with blur on, any two of the plane ranges d_work / d_sbuf / d_zbuf overlapping;
 *                        PWN_ENOLEVEL, PWN_ENOTSUP and PWN_EBUSY as pwn_trace_views.  A refused call launches nothing.
 */
#define PWN_VIEWS_HAS_W 1           /* flags of pwn_trace_views_device: honour the w lanes of the cameras */
int pwn_trace_views_device(pwn_ctx *ctx, int n, const void *d_cams, const void *d_secs, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream);

/*
 * trace_screen_centred(lv, x1, y1, x2, y2, cam) (screen.h:31-40) for n views of their OWN sizes, composited on the device into
 * one frame of the context's W x H: split-screen (two half-height views), picture-in-picture (a small preview beside the main
 * view), dynamic resolution (the same rectangle rendered smaller this frame).  Blocking; one trace launch and one blur launch
 * per pass for all the rectangles, one copy to the host.  vp = n rectangles of the frame, cams = n x 16 floats, secs = n
 * sec_current as for pwn_trace_views; sbuf and zbuf (or NULL) are ONE W x H frame each, pitch W.
 *   exactness            the w_i x h_i pixels of rectangle i are bit-identical, colour and depth, to what
 *                        pwn_trace_screen_centred(cams[i], secs[i]) returns on a context of size w_i x h_i with the same level,
 *                        objects and PWN_OPT_BLUR_PASSES.  The view is a frame of its own: the camera set-up of a w_i x h_i frame,
 *                        the pixel seed of (x_local, y_local) in a frame w_i wide (screen.h:19-21 with rwidth = w_i), the 32-pixel
 *                        add chain (screen.h:12-18) from the view's local column 0, blur strength 0.002 * h_i, row seeds from the
 *                        local row, taps clamped to the view's own rectangle (screen.h:103-106 with dimx = w_i, dimy = h_i): a tap
 *                        never reads a neighbouring rectangle.
 *   depth                the call family owns one pre-blur plane, one colour plane (the two take turns under several blur passes)
 *                        and one depth plane of W x H,
 *                        apart from the blocking call's planes and from the view slots of pwn_trace_views.  The depth plane is zero
 *                        when first allocated and persists across calls BY DESTINATION PIXEL: a primary ray that runs out of steps
 *                        keeps what the plane holds at the pixel it is composited to (trace.h:677), whichever rectangle wrote it.
 *                        Cost: 12 B x W x H on the device, allocated by the first call; pwn_destroy frees them.
 *   outside the rectangles  colour reads 0; zbuf is the depth plane as it stands.
 *   blur                 PWN_OPT_BLUR_PASSES as the blocking call.  With blur on, PWN_EINVAL unless W % 4 == 0 and every x_i % 4 == 0
 *                        and w_i % 4 == 0 (the w % 4 rule of the blocking call, and 16-byte groups in a pitch-W plane); with blur
 *                        off any rectangle is accepted.
 *   counters, timings, ordering, not followed, left alone
 *                        as pwn_trace_views (counters summed over the views; behind the frames in flight; always the units
 *                        scheduler, never in row strips; the unit-order state, the trace-room measurement and the blocking call's
 *                        planes are left alone) -- and so are the view slots of pwn_trace_views.
 *   errors               PWN_EINVAL for NULL ctx / vp / cams / secs / sbuf, n < 1, n > PWN_VIEWS_MAX, a rectangle with w < 1 or
 *                        h < 1, a rectangle not inside W x H, two rectangles that overlap (touching edges is fine), the blur rules
 *                        above; PWN_ENOLEVEL before a level; PWN_ENOTSUP on a pwn_init_multi handle; PWN_EBUSY while the context runs
 *                        a row tiling (pwn_tiled_init).
 * pwn_viewports_plan applies the checks of that list that need no context -- host only, no context, no device (like
 * pwn_sphere_tables_plan); pwn_trace_viewports calls the same function, so the two cannot disagree.  PWN_OK or PWN_EINVAL, and
 * out is filled in both cases (PWN_EINVAL alone for a NULL out):
 *     out[0]  16 x 4-pixel units of the launch: the sum over the views of ceil(w / 16) * ceil(h / 4)
 *     out[1]  pixels covered            out[2]  the largest view's units
 *     out[3]  index of the first offending rectangle (of two that overlap: the later one), or n if there is none -- also when
 *             what is wrong is not a rectangle: n itself, a NULL vp, W or H outside pwn_init's 1..32768, W % 4 with blur on
 *   (out[0..2] count the rectangles that lie inside a valid frame; 0 where vp, n or the frame is refused)
 */
typedef struct pwn_viewport { int32_t x, y, w, h; } pwn_viewport;   /* a rectangle of the context's W x H frame */
int pwn_viewports_plan(int W, int H, int blur_passes, int n, const pwn_viewport *vp, unsigned long long out[4]);
int pwn_trace_viewports(pwn_ctx *ctx, int n, const pwn_viewport *vp, const float *cams, const float *secs,
	uint32_t *sbuf, float *zbuf);
/*
 * The device form: views of their own sizes from cameras in device memory into planes of the CALLER's in device memory, of a frame
 * size the caller chooses -- stream-ordered on `stream` (a hipStream_t, NULL = default stream) like pwn_trace_views_device, no
 * synchronisation, no host copy.  Observations of many agents at their own resolutions in one tensor (an atlas), a 4K spectator
 * frame or a split screen from the cameras pwn_players_step_device moves, on the context that holds the level and the tables of
 * pwn_upload_spheres_device -- whatever that context's own size is: it plays no part in any pixel.
 *
 * A LAYOUT is the part of a call the host knows beforehand and that does not change: the frame size W x H (1..32768 each, an
 * argument, not the context's) and n rectangles of it.  pwn_viewports_layout makes one -- it may block, allocate and copy, and needs
 * no level -- and any number of calls use it: the typical host has one per screen arrangement or atlas and moves only cameras.
 *   rules                pwn_viewports_plan's for blur 0, by calling that very function: n in 1..PWN_VIEWS_MAX, every rectangle
 *                        inside W x H, no two overlapping (touching is fine).  Whether the blur rules hold as well (W % 4 == 0,
 *                        every x_i % 4 == 0 and w_i % 4 == 0) is recorded: a call with blur on needs such a layout.
 *   pwn_viewports_layout_info   out[0..5] = W, H, n, the 16 x 4-pixel units of a launch, the pixels covered, 1 if usable with blur on.
 *   pwn_viewports_layout_free   waits on the host for the last launches that read the layout (an event recorded behind every use,
 *                        per stream it was used on), then frees it.  PWN_EINVAL for a layout of another context or one already
 *                        freed.  pwn_destroy frees what is left.
 *   cost                 on the device 148 B a rectangle and 8 B per 4 pixels of the widest view (the blur's skip-ahead table, which
 *                        the context has only for views up to its own width), 128 B a rectangle on the host.
 *   errors               PWN_EINVAL for what pwn_viewports_plan refuses with blur 0 and for a NULL ctx or out; PWN_ENOMEM;
 *                        PWN_ENOTSUP on a pwn_init_multi handle.  *out is NULL unless the call returns PWN_OK.
 *
 * pwn_trace_viewports_device:
 *   d_cams, d_secs       n x 16 floats (rows x,y,z,w), camera i for rectangle i of the layout -- the array pwn_players_step_device
 *                        steps -- and n floats.
 *   d_sbuf, d_zbuf, d_work   ONE plane of W x H words each, pitch W, all the caller's.  d_zbuf is required and in / out: a primary ray
 *                        that runs out of steps keeps what the plane holds at its destination pixel (trace.h:677).  d_work is
 *                        required when PWN_OPT_BLUR_PASSES > 0; the trace writes whichever of d_work / d_sbuf makes the last blur
 *                        pass land in d_sbuf (d_work for an odd number of passes), as pwn_trace_views_device.
 *                        All five pointers are 16-byte aligned.
 *   flags                0 or PWN_VIEWS_HAS_W, with pwn_trace_views_device's meaning.
 *   launches             one set-up launch (a thread per record: its geometry from the layout, its head from the view's camera), one
 *                        trace launch, one blur launch per pass, all on `stream`.  After the context's first such call, which
 *                        allocates the records below, a call makes no allocation, no copy from host memory, no event wait on the
 *                        host and no synchronisation.  The trace launch falls under the rule for trace launches at the top of this
 *                        file; a call that leaves the rotation is put behind launch n - R on `stream` before its set-up kernel writes.
 *   records              the library's, as pwn_trace_views_device's: PWN_VIEWS_MAX records of 128 B per set of work-queue counters
 *                        (768 KB in all), allocated by the first call, freed by pwn_destroy; a launch uses the records of the set it
 *                        counts in.
 *   exactness            rectangle i is bit-identical, colour and depth, to rectangle i of pwn_trace_viewports on a context of size
 *                        W x H with the same rectangles, cameras, times, level, objects and PWN_OPT_BLUR_PASSES, provided d_zbuf on
 *                        entry holds what that context's viewport depth plane held (zero for a fresh one) -- and so, through that
 *                        call's contract, to pwn_trace_screen_centred on a context of w_i x h_i.  The set-up runs on the device with
 *                        the host's arithmetic, operation for operation, denormals kept.
 *   outside the rectangles   nothing of d_sbuf or d_zbuf is written (the host form clears; this form leaves alone): several calls,
 *                        with other layouts of the same W x H or from other contexts, may fill one atlas.  What d_work holds
 *                        afterwards is unspecified.
 *   counters, not followed, left alone
 *                        as pwn_trace_views_device; the planes and the depth plane of pwn_trace_viewports are left alone too.  The
 *                        call sets no timings.
 *   errors               PWN_EINVAL for a NULL ctx / layout / d_cams / d_secs / d_sbuf / d_zbuf, a NULL d_work with blur on, a
 *                        layout of another context (or a freed one), flags other than PWN_VIEWS_HAS_W, a pointer that is not 16-byte
 *                        aligned, any two of the three plane ranges (W x H x 4 bytes each) overlapping, blur on with a layout that
 *                        is not usable with blur; PWN_ENOLEVEL, PWN_ENOTSUP and PWN_EBUSY as pwn_trace_views.  A refused call
 *                        launches nothing and changes nothing.
 */
typedef struct pwn_vp_layout pwn_vp_layout;
int pwn_viewports_layout(pwn_ctx *ctx, int W, int H, int n, const pwn_viewport *vp, pwn_vp_layout **out);
int pwn_viewports_layout_free(pwn_ctx *ctx, pwn_vp_layout *layout);
int pwn_viewports_layout_info(const pwn_vp_layout *layout, unsigned long long out[6]);
int pwn_trace_viewports_device(pwn_ctx *ctx, const pwn_vp_layout *layout, const void *d_cams, const void *d_secs, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream);

/*
 * Caller-supplied rays: trace_ray(0, &seed_i, lv, &depth_i, &origin_i, &dir_i, {1,1,1,1}) (trace.h:186, called as at
 * screen.h:22-24) for n rays of the caller's choosing, on the context's current level and object table with sec_current:
 * hitscan and line of sight ("how far along this direction is the first thing, through portals and past spheres"), picking
 * under the crosshair, projections other than the pinhole (panoramas, fisheyes, cube-map faces: the caller computes the rays).
 *   ray record     8 floats, 32 B: origin x y z w, then direction x y z w (the two vec4 of trace_ray).  n records, back to back.
 *   seed           seeds[i] is *seed as trace_ray is entered: pwn_pixel_rays below gives pixel (x, y)'s of a w-wide frame
 *                  (screen.h:19-21).  The device doubles it internally as the frame path does (lcg2_fs).
 *   colour         col[i] = col_ftoint of trace_ray's value, BGRA8 as a pixel of sbuf (before any blur: ray batches are not blurred).
 *   depth          in / out: on entry the value the ray keeps if its primary segment runs out of steps (trace.h:677), on return
 *                  the primary hit's distance (trace.h:102-105).
 *   w lanes        a batch whose records all have origin.w == 1 and direction.w == 0 runs the 3-lane kernel variants, any other
 *                  the 4-lane ones (the rule pwn_trace_screen_centred applies to cameras; PWN_DBG_FORCE_HASW forces 4 lanes and
 *                  changes no result).  The device form is told which by its flags: without PWN_RAYS_HAS_W the w lanes are
 *                  taken as 1 and 0, whatever the records hold.
 *   exactness      ray i is bit-identical, colour and depth, to pixel (x, y) of pwn_trace_screen_centred's pre-blur frame
 *                  (PWN_OPT_BLUR_PASSES 0) when its record and seed are pwn_pixel_rays' for that pixel and its depth on entry is
 *                  the frame's depth plane there; the same contract as the frames' with the reference.
 *   empty batch    n == 0 is PWN_OK once the arguments pass the checks below, and launches nothing.
 *   ordering       pwn_trace_rays (host memory, blocking) waits behind the frames in flight as pwn_trace_screen_centred does and
 *                  ends with its stream drained.  pwn_trace_rays_device is ONE trace launch on `stream` (device pointers,
 *                  stream-ordered, no synchronisation) under the rule for trace launches at the top of this file.
 *   counters       with PWN_OPT_COUNTERS on, the counting variant runs and pwn_get_stats returns its rays, steps, portals,
 *                  sphere tests and exhausted rays.  pwn_trace_rays also sets trace_ms (upload and trace) and total_ms; blur_ms 0.
 *   not followed   always the units scheduler, never refill (PWN_OPT_SCHEDULER); PWN_OPT_UNIT_ORDER, PWN_OPT_WAVE_LOG and
 *                  PWN_OPT_CALL_STRIPS do not apply; no blur.
 *   left alone     the blocking call's planes and their depth persistence, pwn_screen_upscale(NULL, ...), the view slots of
 *                  pwn_trace_views, the unit-order state, the trace-room measurement, the call-strips calibration window.
 *   cost           pwn_trace_rays keeps 44 B per ray of pinned host memory and as much device memory between calls, grown to
 *                  the largest batch so far (at least 4096 rays); pwn_destroy frees them.
 *   errors         PWN_EINVAL: NULL ctx, NULL rays with n > 0, n < 0, n > PWN_RAYS_MAX, col and depth both NULL (host form),
 *                  d_col or d_depth NULL with n > 0 (device form), flags other than PWN_RAYS_HAS_W, d_rays not 16-byte aligned or d_seeds /
 *                  d_col / d_depth not 4-byte aligned; PWN_ENOLEVEL before a level; PWN_ENOTSUP on a pwn_init_multi handle;
 *                  PWN_EBUSY while the context runs a row tiling (pwn_tiled_init); PWN_ENOMEM when the host form's buffers
 *                  cannot grow.
 */
#define PWN_RAYS_HAS_W 1            /* flags of pwn_trace_rays_device: honour the w lanes of the records */
#define PWN_RAYS_MAX (1 << 28)
/* Host only, no context and no GPU: the ray record (rays: n x 8 floats) and, unless seeds is NULL, the seed of pixels
   (xy[2i], xy[2i+1]) of a width x height frame of camera cam, computed exactly as the frame kernel does (frame_setup, then the
   add chain of screen.h:12-18 in the reference build's order, under FTZ|DAZ as the device and the reference executable).
   Tracing them reproduces that frame's pre-blur colour and depth at those pixels.  PWN_EINVAL: cam NULL, xy or rays NULL with
   n > 0, n < 0, n > PWN_RAYS_MAX, a pixel outside the frame, width or height outside pwn_init's 1..32768. */
int pwn_pixel_rays(int width, int height, const float cam[16], int n, const int32_t *xy, float *rays, uint32_t *seeds);
/*
 * pwn_pixel_rays on the device: the ray records and seeds of m pixels of each of n cameras that are already in device memory, written
 * to device memory on the caller's stream -- so that step -> aim -> pwn_trace_hits_device (which object does every player's
 * crosshair rest on), picking under a cursor, or a sparse or foveated subset of a view's pixels need no host round trip.
 *   what            for camera i and its pixel j the record and the seed that pwn_pixel_rays(width, height, cam_i, ...) writes for that pixel.
 *   rays            ray i * m + j is camera i's pixel j.  A record is 8 floats, origin then direction, as pwn_trace_rays takes them.
 *   width, height   1..32768: the frame the pixels belong to, which need not be the context's.
 *   d_cams          n x 16 floats, rows x, y, z, w: the array pwn_players_step_device steps and pwn_trace_views_device reads.
 *   d_xy            int32 pairs (x, y): m of them with PWN_PIXELS_SHARED, which every camera then uses; otherwise n x m, camera-major.
 *                   May be NULL with PWN_PIXELS_SHARED and m == width * height: the pixels are then the whole frame, row-major
 *                   (x = j % width, y = j / width).
 *   d_work          n x PWN_PIXEL_WORK_BYTES of the caller's scratch (as pwn_trace_views_device's d_work: the call owns no buffer,
 *                   allocates nothing and never synchronises).  What it holds afterwards is unspecified.
 *   d_rays          n x m records of 32 B.
 *   d_seeds         n x m uint32, or NULL: none is written.
 *   alignment       d_cams, d_work and d_rays 16 bytes, d_xy 8 bytes, d_seeds 4 bytes.
 *   exactness       record and seed are bit-identical to pwn_pixel_rays' for every finite camera, cameras with denormal entries and
 *                   with w components included: the camera set-up runs with denormals kept and the add chain flushed, as on the host.
 *                   The origin is the camera's row w bit for bit (a copy, not arithmetic).  All four lanes of the direction are
 *                   written (there is no HAS_W flag here: the caller tells the trace call about w lanes).  Through pwn_pixel_rays'
 *                   own contract the rays reproduce a frame's pre-blur colour and depth.
 *   outside the frame   the device cannot refuse a pixel.  The record is the formula's value for that (x, y) -- the ray through that
 *                   point of the image plane -- and the seed the uint32 formula's, defined for -32768 <= x, y < 65536; beyond
 *                   that the values are unspecified.  Whatever d_xy holds, the call reads and writes nothing outside its ranges,
 *                   and the add chain is (x & 31) + 1 long, never more.
 *   ordering        at most two launches on `stream` (a hipStream_t, NULL = default stream): no synchronisation, no events, no wait
 *                   for table uploads.  It uses no work-queue counters and does not enter the launch rotation: the rule for trace
 *                   launches at the top of this file does not apply to it.
 *   no level        it reads no tables: PWN_OK before a level is loaded.
 *   left alone      everything pwn_players_step leaves alone, pwn_stats and pwn_launch_order_waits included.
 *   errors          PWN_EINVAL for a NULL ctx, width or height out of range, n < 0, n > PWN_PLAYERS_MAX, m < 0, n x m > PWN_RAYS_MAX
 *                   (in 64 bits), flags other than PWN_PIXELS_SHARED, a NULL d_cams, d_work or d_rays with n x m > 0, a NULL d_xy
 *                   outside the whole-frame case, a misaligned pointer, any two of the five ranges overlapping; PWN_ENOTSUP on a
 *                   pwn_init_multi handle; PWN_EBUSY while the context runs a row tiling (pwn_tiled_init).
 *                   n x m == 0 is PWN_OK once the checks pass.  A refused or empty call launches nothing.
 */
#define PWN_PIXELS_SHARED   1    /* flags: d_xy holds m pixels that every camera uses; without it n x m, camera-major */
#define PWN_PIXEL_WORK_BYTES 80  /* bytes of d_work per camera (= a view record) */
int pwn_pixel_rays_device(pwn_ctx *ctx, int width, int height, int n, const void *d_cams,
	int m, const void *d_xy, int flags, void *d_work, void *d_rays, void *d_seeds, void *stream);
/* Blocking, host memory.  seeds NULL: every seed 0.  col or depth may be NULL (not both); depth NULL: every ray starts at 0. */
int pwn_trace_rays(pwn_ctx *ctx, int n, const float *rays, const uint32_t *seeds, float sec_current,
	uint32_t *col, float *depth);
/* Device pointers, stream-ordered on `stream` (a hipStream_t, NULL = default stream) like pwn_trace_rows_device: d_rays 16-byte
   aligned, d_seeds NULL (every seed 0) or n uint32, d_col n uint32 and d_depth n floats (in / out), both required for n > 0. */
int pwn_trace_rays_device(pwn_ctx *ctx, int n, const void *d_rays, const void *d_seeds, float sec_current, int flags,
	void *d_col, void *d_depth, void *stream);

/*
 * First hits of caller-supplied rays: what the PRIMARY segment of trace_ray (trace.h:186) ended on, for the rays pwn_trace_rays
 * takes.  Where pwn_trace_rays answers "what colour, how far", this answers a game loop's questions -- which object, which wall
 * cell, where, on which side of how many portals -- and stops there: one set-up and one walk per ray, no shading, no bounce, no
 * second or third segment, no random number (there is no seed) and no floor ripple (there is no sec_current).
 * Ray records, PWN_RAYS_HAS_W, PWN_RAYS_MAX, the 3-lane / 4-lane rule, the empty batch, the ordering of the two forms, "not
 * followed", "left alone" and the error rules are pwn_trace_rays' / pwn_trace_rays_device's above, with hits in the place of col and
 * depth (required for n > 0) and d_hits 16-byte aligned in the place of d_col / d_depth.
 * A record holds trace.h's variables at the moment trace_ray's primary walk returns:
 *   kind      PWN_HIT_NONE: the segment ran out of steps (trace.h:677).  Then face = object = -1 and every other field is 0.
 *   face      ldir, 0..5 = FXP, FZP, FXN, FZN, FYP, FYN (defs.h:25-33); a room cell's floor or ceiling as the frame shades it.  A sphere: -1.
 *   object    a sphere: its index in the live table -- its place in pwn_upload_spheres' array, in pwn_get_objects' output and in
 *             pwn_get_object_ids', which names the pwn_obj_new handle.  Otherwise -1.
 *   portals   portals this segment crossed (trace.h:576).
 *   dist      what a frame writes to zbuf for this ray: aux_dist for a sphere, cdist otherwise.
 *   x, y, z   aux_pos for a sphere (the reference's own point, pos + sdist * ray of trace.h:256-294: where it shades the sphere, not
 *             the geometric intersection), otherwise pos before the 0.001 step off the surface -- in the coordinates of the far
 *             side of the portals crossed.
 *   dx,dy,dz  the walked ray as the segment returns it: normalised, clamped to EPSILON, turned by the portals crossed; in a ramp
 *             cell with the ramp's y skew, as the reference's shading sees it.
 *   cell_x,z  cx, cz at the return.  A sphere, a floor or a ceiling: the cell the last step began in (a ramp or portal step that the
 *             reference leaves through trace.h:668 included).  A side wall: the solid cell, which out of a 2-high cell ('#', '&') is
 *             the cell stepped into.  A ray that starts further than 16383 cells out is pinned there.
 * Counters: with PWN_OPT_COUNTERS on, pwn_get_stats returns rays (= n), steps, portals, sphere_tests and exhausted of the primary
 * segments.  pwn_trace_hits keeps 80 B per ray of pinned host memory (32 in, 48 out) and as much device memory between calls,
 * grown to the largest batch so far (at least 4096 rays); pwn_destroy frees them.  It sets trace_ms and total_ms as pwn_trace_rays does.
 */
#define PWN_HIT_NONE   0   /* the primary segment ran out of steps (trace.h:677) */
#define PWN_HIT_WALL   1   /* wall, floor, ceiling, portal frame */
#define PWN_HIT_SPHERE 2
typedef struct pwn_hit {            /* 48 bytes */
	int32_t kind, face, object, portals;
	float   dist, x, y, z;
	float   dx, dy, dz;
	int16_t cell_x, cell_z;
} pwn_hit;
/* Blocking, host memory. */
int pwn_trace_hits(pwn_ctx *ctx, int n, const float *rays, pwn_hit *hits);
/* Device pointers, ONE trace launch, stream-ordered on `stream` (NULL = default stream): d_rays and d_hits (n records of 48 B) 16-byte aligned. */
int pwn_trace_hits_device(pwn_ctx *ctx, int n, const void *d_rays, int flags, void *d_hits, void *stream);
/* Per live sphere, in the order of the table the kernels read (pwn_hit.object indexes it), the pwn_obj_new handle it came from: after
   pwn_upload_spheres 0..n-1.  Writes at most cap entries; returns the count, or PWN_EINVAL (an object created but never set, as
   pwn_get_objects; NULL ctx, cap < 0, NULL ids with cap > 0). */
int pwn_get_object_ids(pwn_ctx *ctx, int *ids, int cap);

/*
 * First-hit planes of a batch of views: what is under every pixel of n views of the context's w x h -- which object, which kind of
 * surface, behind how many portals, in which cell, how far.  A label plane and a depth plane beside pwn_trace_views' colour for a
 * network's observations, an object-id map for picking by look-up, the set of cells and spheres a camera sees.  Per pixel: the
 * PRIMARY segment of trace_ray (trace.h:186) along the pixel's ray (screen.h:12-24) -- one set-up and one walk, as pwn_trace_hits,
 * with the rays made on the device by the add chain of the frame kernel (screen.h:12-18) and 12 B a pixel stored.
 *   cams                 n x 16 floats as for pwn_trace_views.  No secs: the primary segment reads no time and draws no random number.
 *   planes               label, cell, dist: n x h x w 32-bit words each, view-major.  label is required; cell and dist may be NULL and
 *                        are then not written.  EVERY pixel of every plane given is written: nothing is in / out, nothing persists
 *                        between calls, and the call family owns no depth plane.
 *   exactness            pixel (x, y) of view i holds the pwn_hit that pwn_trace_hits returns for pwn_pixel_rays(w, h, cams[i], (x, y)),
 *                        every field that has a place bit for bit:
 *                          label   kind | (face + 1) << 2 | (object + 1) << 5 | portals << 19   (PWN_LABEL_* take it apart)
 *                          cell    cell_x in the low 16 bits, cell_z in the high 16, both int16 (the record's last word)
 *                          dist    pwn_hit.dist
 *                        PWN_HIT_NONE gives 0 in all three.  And so, through pwn_trace_hits' contract, to the reference's variables when
 *                        trace_ray's primary walk returns; dist is what pwn_trace_views writes to that pixel of zbuf where the ray ends
 *                        on something.  x y z and dx dy dz have no plane: pwn_trace_hits on pwn_pixel_rays serves the pixels that need them.
 *   w lanes              as pwn_trace_views (the host form looks at the cameras) and pwn_trace_views_device (PWN_VIEWS_HAS_W).
 *   ordering             the host form behind the frames in flight, as pwn_trace_views, and ends with its stream drained.
 *   counters             with PWN_OPT_COUNTERS on: rays = n x w x h, and steps, portals, sphere_tests and exhausted of the primary
 *                        segments, as pwn_trace_hits counts them.  The host form sets trace_ms (upload and trace) and total_ms, blur_ms 0.
 *   not followed         as pwn_trace_views: always the units scheduler, never row strips, no unit order, no wave log; and no blur:
 *                        PWN_OPT_BLUR_PASSES is ignored (w % 4 != 0 is no error).
 *   left alone           the blocking call's planes, the view slots of pwn_trace_views, the planes of pwn_trace_viewports, the
 *                        unit-order state, the trace-room measurement, the call-strips calibration window.
 *   cost                 the host form keeps 12 B per pixel of pinned host memory and as much device memory between calls, grown to
 *                        the largest call so far; pwn_destroy frees them.  They are pwn_trace_hits' buffers: the larger need counts.
 *   errors               PWN_EINVAL for NULL ctx / cams / label, n < 1, n > PWN_VIEWS_MAX, n x w x h > 2^28; PWN_ENOLEVEL,
 *                        PWN_ENOTSUP and PWN_EBUSY as pwn_trace_views; PWN_ENOMEM when the host form's buffers cannot grow.
 */
/* one word per pixel; 0 = the primary segment ran out of steps (PWN_HIT_NONE) */
#define PWN_LABEL_KIND(l)     ((l) & 3u)                          /* PWN_HIT_* */
#define PWN_LABEL_FACE(l)     ((int)(((l) >> 2) & 7u) - 1)        /* pwn_hit.face, -1 for a sphere / nothing */
#define PWN_LABEL_OBJECT(l)   ((int)(((l) >> 5) & 0x3fffu) - 1)   /* pwn_hit.object, -1 = none */
#define PWN_LABEL_PORTALS(l)  ((l) >> 19)                         /* pwn_hit.portals */
/* Blocking, host memory. */
int pwn_trace_view_hits(pwn_ctx *ctx, int n, const float *cams, uint32_t *label, uint32_t *cell, float *dist);
/* The device form: cameras and planes in device memory, stream-ordered on `stream` (a hipStream_t, NULL = default stream) like
   pwn_trace_views_device -- no synchronisation, no host copy.  d_cams n x 16 floats; d_label required, d_cell and d_dist or NULL;
   all pointers 16-byte aligned.  flags: 0 or PWN_VIEWS_HAS_W, with pwn_trace_views_device's meaning.  One camera set-up launch and
   one trace launch, both on `stream`; the trace launch falls under the rule for trace launches at the top of this file and uses
   the view records of the counter set it counts in, as pwn_trace_views_device.  Sets no timings.  Beyond the host form's errors,
   PWN_EINVAL for flags other than PWN_VIEWS_HAS_W, a pointer that is not 16-byte aligned, any two of the given plane ranges
   overlapping.  A refused call launches nothing. */
int pwn_trace_view_hits_device(pwn_ctx *ctx, int n, const void *d_cams, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream);

/*
 * First-hit planes of views of their OWN sizes: pwn_trace_view_hits' three planes for the rectangles of pwn_trace_viewports -- label and
 * depth observations of agents at their own resolutions in one atlas beside a 4K spectator frame, from the ONE context that holds the
 * level and the tables of pwn_upload_spheres_device; picking by look-up under a split screen or a picture-in-picture frame at 12 B a
 * pixel.  n views, view i a frame of its own of w_i x h_i in rectangle vp[i] of a frame of W x H.
 *   cams                 n x 16 floats, camera i for rectangle i.  No secs, no seed, no blur: the primary segment reads no time and
 *                        draws no random number.
 *   planes               label, cell, dist: ONE plane of W x H 32-bit words each, pitch W (the host form: the context's w x h).  label is
 *                        required; cell and dist may be NULL and are then not written.  EVERY pixel of every rectangle is written in
 *                        every plane given: nothing is in / out, nothing persists between calls.
 *   exactness            pixel (x, y) of rectangle i, local to the rectangle, holds what pwn_trace_view_hits writes for pixel (x, y) of a
 *                        one-view batch of cams[i] on a context of size w_i x h_i with the same level and objects -- and so, through
 *                        that call's contract, the pwn_hit that pwn_trace_hits returns for pwn_pixel_rays(w_i, h_i, cams[i], (x, y)),
 *                        bit for bit: label with the PWN_LABEL_* packing, cell = the record's last word, dist = pwn_hit.dist;
 *                        PWN_HIT_NONE gives 0 in all three.  The view is a frame of its own: the camera set-up of a w_i x h_i frame
 *                        and the 32-pixel add chain from the view's local column 0.
 *   outside the rectangles   the host form gives 0 in every plane given (it owns its staging, as pwn_trace_viewports clears its
 *                        planes); the device form writes nothing there: several calls and several layouts may fill one atlas, as
 *                        with pwn_trace_viewports_device.
 *   rectangles           pwn_viewports_plan(W, H, 0, ...)'s rules, by calling that function: any rectangle inside W x H that overlaps
 *                        no other.  No % 4 rule: PWN_OPT_BLUR_PASSES is ignored.
 *   w lanes              the host form looks at the cameras; the device form takes PWN_VIEWS_HAS_W, as pwn_trace_views_device.
 *   ordering             the host form behind the frames in flight, and ends with its stream drained, as pwn_trace_view_hits.
 *   counters             with PWN_OPT_COUNTERS on: rays = the pixels covered, and steps, portals, sphere_tests and exhausted of the
 *                        primary segments, as pwn_trace_hits counts them, summed over the views.  The host form sets trace_ms (upload
 *                        and trace) and total_ms, blur_ms 0; the device form sets no timings.
 *   not followed         as pwn_trace_view_hits[_device]: always the units scheduler, never row strips, no unit order, no wave log, no blur.
 *   left alone           what pwn_trace_view_hits[_device] leaves alone, and the planes and the depth plane of pwn_trace_viewports, the
 *                        view slots, the blocking call's planes, the unit-order state, the trace-room measurement, the call-strips window.
 *   cost                 the host form keeps 12 B per pixel of W x H in pinned host memory and as much device memory between calls:
 *                        they are pwn_trace_hits' buffers, and the larger need counts.  Its records are pwn_trace_viewports' (128 B a
 *                        view for PWN_VIEWS_MAX views, pinned and on the device, with the first call of either).  The device form's
 *                        records are pwn_trace_viewports_device's.  pwn_destroy frees them.
 *   errors               PWN_EINVAL for a NULL ctx / vp / cams / label and for what pwn_viewports_plan refuses; PWN_ENOLEVEL,
 *                        PWN_ENOTSUP on a pwn_init_multi handle and PWN_EBUSY under a row tiling, as pwn_trace_viewports;
 *                        PWN_ENOMEM when the staging cannot grow.
 */
/* Blocking, host memory: planes of the context's W x H, pitch W. */
int pwn_trace_viewport_hits(pwn_ctx *ctx, int n, const pwn_viewport *vp, const float *cams,
	uint32_t *label, uint32_t *cell, float *dist);
/* Device form: a layout (pwn_viewports_layout), cameras and planes of the CALLER's in device memory, stream-ordered.  Any layout of
   this context: whether it is usable with blur plays no part.  d_cams n x 16 floats, camera i for rectangle i (the array
   pwn_players_step_device steps); the planes W x H words of the layout's frame size, pitch W; all pointers 16-byte aligned.  flags: 0
   or PWN_VIEWS_HAS_W.  One set-up launch and one trace launch on `stream`, nothing else; after the context's first such call (or
   first pwn_trace_viewports_device, whose records these are) no allocation, no copy from host memory, no host wait and no
   synchronisation.  The trace launch falls under the rule for trace launches at the top of this file and uses the viewport records
   of the counter set it counts in; a call that leaves the rotation is put behind launch n - R on `stream` before its set-up kernel
   writes.  A use of the layout records the event pwn_viewports_layout_free waits for.  PWN_EINVAL for a NULL ctx / layout / d_cams /
   d_label, a layout of another context (or a freed one), flags other than PWN_VIEWS_HAS_W, a pointer that is not 16-byte aligned,
   any two of the given plane ranges (W x H x 4 bytes each) overlapping; PWN_ENOLEVEL, PWN_ENOTSUP and PWN_EBUSY as the host form.
   A refused call launches nothing and changes nothing. */
int pwn_trace_viewport_hits_device(pwn_ctx *ctx, const pwn_vp_layout *layout, const void *d_cams, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream);

/*
 * One hidden sphere per view or ray: pwn_trace_views_device, pwn_trace_view_hits_device and pwn_trace_hits_device -- and
 * pwn_trace_viewports_device, pwn_trace_viewport_hits_device and pwn_trace_rays_device -- for viewers that do
 * not see one object of the table -- their own body (player i's sphere sits where camera i is, and a camera inside or next to a
 * sphere sees it in every ray that points at its centre, a crosshair ray reports it as its first hit), a carried item, the object a
 * preview camera is mounted on.  One sphere table and one launch for all agents, where the alternative is a table and a launch each.
 *   d_hide               n int32 in device memory, 4-byte aligned, required for n > 0; for the viewports pair n is the layout's count,
 *                        and entry i belongs to rectangle i and camera i of the layout, in the caller's order.  Entry i is an index into the sphere table in
 *                        force in pwn_hit.object's numbering: the order of pwn_upload_spheres' array, of pwn_get_objects, of d_spheres
 *                        for tables built by pwn_upload_spheres_device.  View i (ray i) does not see that sphere.  Any value that is
 *                        not the index of a live sphere hides nothing: PWN_HIDE_NONE, any negative value, any value >= the live
 *                        count, INT_MAX.  The device cannot refuse a value and does not need to:
 *   safety               a d_hide value is only ever COMPARED -- with the number of a sphere that the walk found through the tables.
 *                        No bit pattern of it reaches an address or a loop bound.
 *   exactness            view i / ray i is bit-identical to view i / ray i of the call without `_hide` on a context whose table is the
 *                        same spheres with entry d_hide[i] taken out and the order otherwise kept: colour, depth, label, cell, dist
 *                        and every field of pwn_hit -- except that object numbers are still those of the FULL table (an object
 *                        j > d_hide[i] reports as j, not j - 1).  The sphere is hidden on EVERY segment of the ray: the primary one and
 *                        the bounces off walls, floors and other spheres -- it is not in that view's mirrors either; that is what
 *                        "taken out of the table" means.  With every entry PWN_HIDE_NONE each call is bit-identical to the call
 *                        it shadows (pwn_trace_views_device / pwn_trace_view_hits_device / pwn_trace_hits_device /
 *                        pwn_trace_viewports_device / pwn_trace_viewport_hits_device / pwn_trace_rays_device), counters included.
 *                        For the viewports pair "view i" is rectangle i of the layout; nothing is written outside the rectangles.
 *   counters             with PWN_OPT_COUNTERS on: rays, steps, portals and exhausted are those of the table without the sphere,
 *                        summed as the calls without `_hide` sum them.  sphere_tests goes on counting the records of the lists walked,
 *                        the hidden sphere's included (it is tested and then passed over): not part of the exactness above.
 *   everything else      is the rule of the call each one shadows: launches (the camera set-up launch -- the viewport set-up launch
 *                        of the viewports pair -- takes d_hide along; one trace launch, of kernels of their own; pwn_trace_rays_hide_device
 *                        is one trace launch), ordering, the layout-use event, the view records per counter set, d_zbuf in / out
 *                        (the viewports': by destination pixel; the rays': d_depth in / out per ray), blur and
 *                        d_work, PWN_VIEWS_HAS_W / PWN_RAYS_HAS_W, the empty batch of rays (d_hide may then be NULL), "not followed",
 *                        "left alone", errors -- a pwn_init_multi handle and a row tiling refuse them like their siblings.
 *   errors, added        PWN_EINVAL for a NULL d_hide or one that is not 4-byte aligned with n > 0, and for the n x 4 bytes of d_hide
 *                        overlapping any range the call writes (d_work / d_sbuf / d_zbuf; d_label / d_cell / d_dist; d_hits;
 *                        d_col / d_depth).  A refused call launches nothing and changes nothing.
 */
#define PWN_HIDE_NONE (-1)
int pwn_trace_views_hide_device(pwn_ctx *ctx, int n, const void *d_cams, const void *d_secs, const void *d_hide, int flags,
	void *d_work, void *d_sbuf, void *d_zbuf, void *stream);
int pwn_trace_view_hits_hide_device(pwn_ctx *ctx, int n, const void *d_cams, const void *d_hide, int flags,
	void *d_label, void *d_cell, void *d_dist, void *stream);
int pwn_trace_hits_hide_device(pwn_ctx *ctx, int n, const void *d_rays, const void *d_hide, int flags, void *d_hits, void *stream);
int pwn_trace_viewports_hide_device(pwn_ctx *ctx, const pwn_vp_layout *layout, const void *d_cams, const void *d_secs,
	const void *d_hide, int flags, void *d_work, void *d_sbuf, void *d_zbuf, void *stream);
int pwn_trace_viewport_hits_hide_device(pwn_ctx *ctx, const pwn_vp_layout *layout, const void *d_cams, const void *d_hide,
	int flags, void *d_label, void *d_cell, void *d_dist, void *stream);
int pwn_trace_rays_hide_device(pwn_ctx *ctx, int n, const void *d_rays, const void *d_seeds, const void *d_hide,
	float sec_current, int flags, void *d_col, void *d_depth, void *stream);

/*
 * Rays that stop after a given distance: pwn_trace_hits with a reach per ray -- for whatever flies (a projectile moves `reach` a
 * tick and is the next tick's ray from where it got to) and for weapons with a range (the walk ends where the answer is decided,
 * not at the far wall).  The point a distance along a ray cannot be computed outside the walk once a portal, a two-high room or a
 * ramp lies in between: position and direction are re-expressed at every crossing, and a portal cell is crossed without adding to
 * the distance (trace.h:186 the set-up, trace.h:250 the walk's loop).
 * Ray records, PWN_RAYS_HAS_W, the 3-lane / 4-lane rule, PWN_RAYS_MAX and the empty batch are pwn_trace_hits' / pwn_trace_hits_device's /
 * pwn_trace_hits_hide_device's; so are the ordering of the forms, "not followed", "left alone", the buffers the host form keeps, the
 * timings it sets and every refusal (a pwn_init_multi handle, a row tiling, no level, alignment, overlaps).
 *   reach                n floats (device forms: in device memory), 4-byte aligned, required for n > 0; d_reach must not overlap d_hits.
 *   unit                 reach is measured as pwn_hit.dist is: in the walk's own distance, after the set-up's approximate normalise.
 *   the definition       a process, not geometry.  Ray i runs the primary walk of pwn_trace_hits.  Step k begins, at the top of the
 *                        walk's loop (trace.h:250), with pos_k, ray_k, cdist_k, the cell c_k and p_k portals crossed so far; cdist_{k+1}
 *                        is cdist when the step is over.  The walk stops behind the first step that leaves cdist > reach, or where the
 *                        unlimited walk returns, whichever comes first.  D is what the record's dist would be at that moment: aux_dist
 *                        for a sphere, cdist for a wall.
 *                          - the walk returned and D <= reach: pwn_trace_hits' record for that ray, bit for bit.
 *                          - the walk ran out of steps first: PWN_HIT_NONE, as there.
 *                          - otherwise PWN_HIT_FREE, read off the step the walk stopped behind, the reach step k with
 *                            cdist_k <= reach < cdist_{k+1}:
 *                              face = object = -1, portals = p_k, dist = reach, cell_x,z = c_k;
 *                              dx,dy,dz = ray_k: normalised, clamped, turned by the portals crossed, and WITHOUT a ramp's skew, so that
 *                              a caller can fly on along it tick after tick without drifting;
 *                              x,y,z = pos_k + (reach - cdist_k) * a, per lane one subtraction, one multiply and one add, never fused, in
 *                              the walk's float mode (denormals flushed); a is the ray with which step k itself advances pos: ray_k in
 *                              a room cell, ray_k with the ramp's skew applied in a ramp cell (trace.h:443-505).
 *                        A portal step adds nothing to cdist and is therefore never the reach step: the point is always in the
 *                        coordinates of the far side of the portals crossed, as pwn_hit.x,y,z are.  A wall met at cdist > reach and a
 *                        sphere with aux_dist > reach are both FREE.  A step that leaves cdist > reach and is the walk's last of
 *                        WALK_STEPS is FREE too (the stop is asked first).
 *   hostile values       reach is only ever compared, subtracted from and multiplied.  No bit pattern of it reaches an address or a loop
 *                        bound.  +inf gives pwn_trace_hits bit for bit, counters included.  NaN is never exceeded and behaves as +inf.
 *                        A negative reach is exceeded by the first step whatever that step does (a ray that starts in a portal's cell
 *                        included: the record is then read off that step's top, p_0 = 0, in front of the crossing) and gives FREE with
 *                        the point behind the origin -- unless that step returns a sphere whose aux_dist is below the reach too.
 *                        reach = 0 gives FREE at the set-up's pos_0, or what the first step returns at distance 0.
 *   hide                 d_hide has pwn_trace_hits_hide_device's meaning, safety and exactness: the table with that sphere taken out,
 *                        objects numbered by the full table -- a projectile a tick old is still inside its shooter's body and must not
 *                        hit it.  With every entry PWN_HIDE_NONE the call is bit-identical to pwn_trace_reach_device.  d_hide must
 *                        not overlap d_hits (d_reach may be anywhere else).
 *   counters             with PWN_OPT_COUNTERS on: rays = n; steps, portals, sphere_tests and exhausted count the steps actually taken,
 *                        up to and including the reach step.
 *   launches             the device forms: ONE trace launch on `stream`, of kernels of their own, under the rule for trace launches at
 *                        the top of this file.  pwn_trace_reach stages 84 B a ray (32 record, 4 reach, 48 out) through pwn_trace_hits'
 *                        buffers: the larger need counts.
 *   errors, added        PWN_EINVAL for a NULL reach / d_reach with n > 0, for a d_reach that is not 4-byte aligned and for its n x 4
 *                        bytes overlapping the n x 48 bytes of d_hits.  A refused call launches nothing and changes nothing.
 *   cost                 2^20 crosshair-like rays, MI355X, device time against pwn_trace_hits_device on the same rays
 *                        (profiles/reach/bench.txt): hall of mirrors 0.296 ms without a reach; reach +inf 0.331 (+12 %), 20: 0.058, 2: 0.051,
 *                        0.35: 0.050.  level.txt 0.056 ms without a reach (3.7 steps a ray, the launch's floor); +inf 0.062 (+9 %), 2: 0.064,
 *                        0.35: 0.056.  The copies of the top-of-step state cost a tenth per step; a caller without a reach calls pwn_trace_hits.
 */
#define PWN_HIT_FREE   3   /* the ray travelled `reach` and met nothing */
/* Blocking, host memory. */
int pwn_trace_reach(pwn_ctx *ctx, int n, const float *rays, const float *reach, pwn_hit *hits);
/* Device pointers, ONE trace launch, stream-ordered on `stream` (NULL = default stream): d_rays and d_hits 16-byte aligned, d_reach n floats. */
int pwn_trace_reach_device(pwn_ctx *ctx, int n, const void *d_rays, const void *d_reach, int flags, void *d_hits, void *stream);
int pwn_trace_reach_hide_device(pwn_ctx *ctx, int n, const void *d_rays, const void *d_reach, const void *d_hide, int flags,
	void *d_hits, void *stream);

/*
 * The players' step: what produces the cameras of pwn_trace_views[_device].  The motion of the reference's loop (main.c:188-379:
 * turning, walking with push-back out of solid cells, gravity, the step between the floors of a two-high room, walking through a
 * portal with its turn) for a batch of n players at once, on the device, on the level in force -- so that step -> observe -> step
 * of many agents runs on one stream with no host round trip.
 *   a tick               one pwn_player_step(p, k, tdiff, cells, pmap) of host/player.c.  `ticks` of them run with the same keys and
 *                        the same tdiff.
 *   cams                 n x 16 floats, rows x, y, z, w: exactly the cams of pwn_trace_views[_device].  In / out.  Row y (floats
 *                        4..7) is never read or written by the step.
 *   gravity              n x 4 floats, in / out (main.c:48,59).
 *   traversals           n int32, in / out: portals walked through so far (pwn_player.traversals).  May be NULL; it is then neither
 *                        read nor written.
 *   keys                 n bytes: bit i is field i of pwn_keys (host/player.h) = PWN_KEY_* i = main.c:72-79, the PWN_MOVE_* below.
 *   exactness            every float and every counter is bit-identical to `ticks` successive pwn_player_step calls on the level
 *                        pwn_get_level returns, for every state in the domain: all 20 floats finite, |pos.x| and |pos.z| <= 2^20,
 *                        tdiff finite.  Denormals are kept, as on the host; all four lanes of the velocity, the position and the
 *                        gravity take part, the w lane included; sinf / cosf are glibc 2.35's.
 *   outside the domain   (NaN, infinities, positions beyond 2^20, where the host's (int) is undefined) the values of that player are
 *                        unspecified.  The call is PWN_OK all the same and reads nothing outside its tables: every cell index goes
 *                        through get_cell's clamp (util.h:151-158) as an integer, the portal index is c - 'A' of a tested letter.
 *                        The other players of the batch are exact.
 *   the level            the one in force when the call is made; the device form waits on `stream` for its upload if that is still
 *                        pending, as a trace launch does.  A level uploaded after the call does not reach it.
 *   ordering             the device form is ONE launch on `stream` (a hipStream_t, NULL = default stream) with no synchronisation.
 *                        It uses no work-queue counters: the rule for trace launches at the top of this file does not apply to it.
 *                        The host form (blocking) is ordered behind the frames in flight, as pwn_trace_rays, and ends with its
 *                        stream drained.
 *   left alone           everything pwn_trace_view_hits leaves alone, and pwn_stats (no counters, no timings, in either form),
 *                        pwn_launch_order_waits and the sphere tables.
 *   cost                 the host form keeps 85 B per player of pinned host memory and as much device memory between calls, grown to
 *                        the largest batch so far (at least 4096 players); pwn_destroy frees them.
 *   device pointers      d_cams and d_gravity 16-byte aligned, d_traversals 4-byte aligned, d_keys any.
 *   errors               PWN_EINVAL for NULL ctx, NULL keys / cams / gravity with n > 0, n < 0, n > PWN_PLAYERS_MAX, ticks < 1,
 *                        ticks > PWN_TICKS_MAX, a tdiff that is not finite, a misaligned device pointer, any two of the device
 *                        ranges overlapping; PWN_ENOLEVEL before a level; PWN_ENOTSUP on a pwn_init_multi handle; PWN_EBUSY while
 *                        the context runs a row tiling (pwn_tiled_init); PWN_ENOMEM when the host form's buffers cannot grow.
 *                        n == 0 is PWN_OK once the other checks pass, and launches nothing.  A refused call launches nothing.
 */
#define PWN_PLAYERS_MAX (1 << 20)
#define PWN_TICKS_MAX   1024
#define PWN_MOVE_TURN_LEFT 1
#define PWN_MOVE_TURN_RIGHT 2
#define PWN_MOVE_TURN_UP 4       /* read and unused, as main.c:188 */
#define PWN_MOVE_TURN_DOWN 8     /* read and unused */
#define PWN_MOVE_FORWARD 16
#define PWN_MOVE_BACK 32
#define PWN_MOVE_LEFT 64
#define PWN_MOVE_RIGHT 128
/* Blocking, host memory, in / out. */
int pwn_players_step(pwn_ctx *ctx, int n, const uint8_t *keys, float tdiff, int ticks,
	float *cams, float *gravity, int32_t *traversals);
/* Device memory, stream-ordered. */
int pwn_players_step_device(pwn_ctx *ctx, int n, const void *d_keys, float tdiff, int ticks,
	void *d_cams, void *d_gravity, void *d_traversals, void *stream);

/*
 * Frames in flight.  The reference presents every frame on the host
 * (trace_screen_centred fills sbuf, screen_upscale fills screen->pixels, SDL_Flip:
 * main.c:107-109).  Over PCIe that hand-over takes longer than the kernels of a
 * frame, so a host that wants throughput overlaps it: with 2-3 slots, frame i
 * travels to the library's pinned host buffers on a copy stream while the
 * kernels of frame i+1 run.
 *   pwn_frames_config  nslots (1..PWN_MAX_SLOTS; 0 releases them) and what a frame
 *                      delivers to the host (flags 0: nothing, the frame stays on the
 *                      device, pwn_frame.d_*): PWN_FRAME_SBUF the colour plane (main.c:31),
 *                      PWN_FRAME_ZBUF the depth plane (main.c:33), PWN_FRAME_SURFACE
 *                      the scale x scale upscaled surface (screen_upscale,
 *                      screen.h:126-149; pitch_bytes 0 = width*scale*4; bytes between
 *                      the rows of a wider pitch read 0).  Buffers are library-owned
 *                      pinned host memory.
 *   pwn_submit_frame   enqueue trace + blur (+ sink) + the copies for `slot`; returns at
 *                      once.  Uses the tables of the last pwn_upload_spheres /
 *                      pwn_prepare_render / level call, which may be called between
 *                      submits without waiting for anything.  PWN_EBUSY if the slot's
 *                      previous frame has not been waited for.  (A host that is short of
 *                      microseconds prepares the next frame's tables BEFORE it waits for the
 *                      slot it wants to reuse: their upload runs on its own stream during that
 *                      wait and the trace launch then queues no wait for it -- ~5 us per frame.)
 *   pwn_wait_frame     block until the slot's frame is on the host; the pointers in
 *                      *out stay valid until the next submit on that slot.
 *   pwn_frame_ready    1 / 0 without blocking.
 *   depth per slot     every slot has a colour and a depth plane of its own (pwn_frame.d_sbuf / d_zbuf), apart from the
 *                      blocking call's planes, the view slots of pwn_trace_views and the planes of pwn_trace_viewports.  A
 *                      slot's depth plane is zero when allocated and keeps its previous value -- the slot's previous frame --
 *                      where the primary ray runs out of steps (trace.h:677).  EVERY pwn_frames_config allocates the slots
 *                      afresh: their depth planes start from zero again, also when the number of slots stays the same, and
 *                      nothing counts as submitted (pwn_wait_frame: PWN_EINVAL); pwn_frame.seq goes on counting.
 *   shared             the pre-blur plane and, under two or more blur passes, the blocking call's colour plane: the passes of
 *                      a frame in flight take turns on the two and the last lands in the slot's own plane, so behind such a
 *                      frame pwn_screen_upscale(NULL, ...) reads that frame's FIRST pass, not the last blocking frame, until the
 *                      next pwn_trace_screen_centred.  With 0 or 1 passes the blocking call's colour is left alone; its depth
 *                      plane always is.
 * Frames complete in submission order.  The blocking pwn_trace_screen_centred may be
 * mixed in; it is ordered behind the submitted frames.
 */
#define PWN_MAX_SLOTS     4
#define PWN_FRAME_SBUF    1
#define PWN_FRAME_ZBUF    2
#define PWN_FRAME_SURFACE 4
typedef struct pwn_frame
{
	const uint32_t *sbuf;        /* BGRA8, pitch = width          (NULL unless PWN_FRAME_SBUF)    */
	const float *zbuf;           /* fp32 depth, pitch = width     (NULL unless PWN_FRAME_ZBUF)    */
	const uint32_t *surface;     /* upscaled, surface_pitch_bytes (NULL unless PWN_FRAME_SURFACE) */
	int surface_pitch_bytes;
	const void *d_sbuf, *d_zbuf, *d_surface;   /* the same planes on the device (d_surface NULL without the flag) */
	float sec_current;           /* as submitted */
	float trace_ms, blur_ms, sink_ms;   /* device time of this frame's kernels, if timed (PWN_OPT_FRAME_TIMING) */
	int timed;
	uint64_t seq;                /* 1, 2, ... in submission order */
} pwn_frame;
int pwn_frames_config(pwn_ctx *ctx, int nslots, int flags, int scale, int pitch_bytes);
int pwn_submit_frame(pwn_ctx *ctx, const float cam[16], float sec_current, int slot);
/* pwn_wait_frame: PWN_EINVAL for a slot nothing was submitted to (since pwn_frames_config).  On a pwn_init_multi handle, after a failure
   of the group that took frames in flight with it: that failure's code, once per lost slot, *out not written, the slot then free (a
   further wait: PWN_EINVAL) -- never PWN_OK with NULL planes.  pwn_frame_ready: 1 ready (or nothing in flight), 0 not yet; of a lost
   slot the failure's code, until its pwn_wait_frame or the next submit. */
int pwn_wait_frame(pwn_ctx *ctx, int slot, pwn_frame *out);
int pwn_frame_ready(pwn_ctx *ctx, int slot);
/* blocking copy of a device plane of a waited-for frame (pwn_frame.d_*) to host memory, for hosts
   that keep their frames on the device and look at one now and then */
int pwn_read_plane(pwn_ctx *ctx, const void *d_src, void *dst, size_t bytes);

/*
 * Strip forms: the two passes restricted to a band of rows, for callers that run their own
 * choreography (the library's own row tiling, pwn_tiled_* below, is built from the same two
 * launches and does the exchange between the GPUs itself: RCCL send / recv inside the library).
 * Pointers are DEVICE pointers to FULL frames (pitch = width); only rows
 * [y0,y1) are written.  Stream-ordered on `stream` (a hipStream_t, NULL =
 * default stream); they do not synchronise.
 *   trace:  the OpenMP loop of screen.h:61-67 restricted to rows [y0,y1)
 *   blur:   one pass of screen.h:77-121 restricted to rows [y0,y1); reads
 *           the whole pre-blur frame (the role of tsbuf) and depth rows [y0,y1)
 */
int pwn_trace_rows_device(pwn_ctx *ctx, const float cam[16], float sec_current,
	int y0, int y1, void *d_sbuf, void *d_zbuf, void *stream);
int pwn_blur_rows_device(pwn_ctx *ctx, int y0, int y1, const void *d_pre,
	const void *d_zbuf, void *d_out, void *stream);
/*
 * The same pass when the caller exchanged only a bounded halo instead of the
 * whole pre-blur frame: rows [avail_y0, avail_y1) of d_pre hold this frame.
 * A tap outside them (taps reach 0.002*h*|depth-1| rows, screen.h:100-102)
 * adds to the uint32 at d_miss (device memory, caller clears it); the strip
 * is then not valid and has to be repeated with the whole frame present.
 */
int pwn_blur_rows_device_bounded(pwn_ctx *ctx, int y0, int y1, const void *d_pre,
	const void *d_zbuf, void *d_out, int avail_y0, int avail_y1, void *d_miss, void *stream);

/*
 * Row tiling behind the ABI: the choreography of the strip forms with the exchange done by
 * the library -- RCCL over xGMI, two grouped ncclSend/ncclRecv launches per frame.  One
 * process per GPU, each with its own context of the FULL frame size; every rank makes the
 * same calls in the same order (level and sphere uploads included: tables are per rank).
 *   pwn_tiled_unique_id  rank 0: the id of the group (an ncclUniqueId for PWN_TRANSPORT_RCCL);
 *                        the host hands its 128 bytes to the other ranks (a file, a pipe, MPI ...)
 *   pwn_tiled_init       collective.  Rank r owns rows [r*per, (r+1)*per), per = ceil(h/world)
 *                        rounded up to 8 (the OpenMP loops of screen.h:63,77 split by rows) -- to begin with: the cuts move
 *                        with what the rows cost (pwn_tiled_balance below).
 *                        halo_rows: pre-blur rows exchanged with each neighbour strip; < 0 = default
 *                        (depth 24: 0.002*h*24 + 2 rows, screen.h:100-102), 0 = every strip to
 *                        everybody (an all-gather).  The blur counts taps that leave the halo; a frame
 *                        with such a tap is repeated with whole strips before it is delivered, and
 *                        whole strips are used from then on: delivered frames are always exact.
 *                        POSTPROC_BLUR 0 or 1.
 *   pwn_tiled_submit     enqueue one frame on every rank, in order on the frame's compute stream: trace own strip,
 *                        one grouped exchange (the strip's border rows with the neighbour strips), blur the strip,
 *                        a second grouped exchange (the finished strip to the frame's root, the rank's two words to
 *                        every rank).  Frames alternate between two streams, so that a frame's exchange overlaps the
 *                        next frame's trace: a frame then costs max(kernels, exchange), not their sum
 *                        (PWN_OPT_TILED_CHOREO).  At most PWN_TILED_SLOTS - 1 = five frames in flight (PWN_EBUSY).
 *   pwn_tiled_wait       every rank: block until the oldest frame in flight is complete; on rank 0 (the frame's root)
 *                        out->d_sbuf is the full frame on the device (valid until five more frames
 *                        were submitted) and, with PWN_TILED_HOST, out->sbuf a pinned host copy.
 *   pwn_tiled_host_sink  optional, every rank, after pwn_tiled_init and before the first frame: frames are
 *                        delivered to the HOST instead (main.c:107-109 presents every frame there).  `base` is
 *                        host memory for PWN_TILED_SLOTS whole frames (w*h*4 bytes each, pitch = width), the SAME
 *                        memory in every rank -- POSIX shared memory mapped by every process -- which the library
 *                        registers with its device.  Every rank then copies its finished strip straight into the
 *                        frame over its own PCIe link (N links, not rank 0's one) and there is no gather to rank
 *                        0: the grouped exchange carries the halo rows and one word per rank, sent behind that
 *                        rank's copy, so that a frame is delivered when every strip has landed.  pwn_tiled_wait
 *                        then gives out->sbuf on EVERY rank (valid until the second next pwn_tiled_submit),
 *                        out->d_sbuf is NULL.
 *   pwn_tiled_gather_root  optional, collective (the same call on every rank, no frame in flight): which rank a frame is
 *                        gathered on.  PWN_TILED_ROOT_FIXED (default): rank 0, every frame -- its links then carry (N-1)/N
 *                        of every frame, which bounds the frame rate of a tiling whose kernels are faster than that
 *                        (xGMI is point to point: 7 links into one GPU).  PWN_TILED_ROOT_ROTATE: frame f
 *                        (pwn_tiled_frame.seq - 1) is gathered on rank f mod N, for consumers that sit on every GPU
 *                        (an encoder per device, N displays): every rank then takes in 1/N of the frames and each of
 *                        its links carries one strip every N-th frame.  pwn_tiled_wait gives out->d_sbuf (and, with
 *                        PWN_TILED_HOST, out->sbuf) on the frame's root, out->root says which rank that is.
 *   pwn_tiled_shutdown   collective; pwn_destroy does it too.
 *   pwn_tiled_set_timeouts  this rank, any time (also before pwn_tiled_init): how long a call of the tiling may wait for
 *                        the other ranks before it gives up.  The reference's error model is print-and-return
 *                        (level.h:35-37,110-115); a row tiling adds a failure the reference cannot have -- a peer that never
 *                        arrives -- and that must come back as an error too, not as a hang.  init_ms bounds the bring-up
 *                        of pwn_tiled_init (communicator + one word exchanged with EVERY other rank, so that every
 *                        connection a frame will use exists when it returns), wait_ms bounds pwn_tiled_wait (and what
 *                        pwn_tiled_submit may have to wait for inside the transport).  On expiry the RCCL communicator
 *                        is aborted (ncclCommAbort; the kernels it has on the device leave), the call returns
 *                        PWN_ETIMEDOUT with pwn_last_error() naming this rank, what it waited for and how far it got,
 *                        and every later pwn_tiled_submit / _wait returns PWN_ETIMEDOUT at once.  0 keeps a value, < 0
 *                        restores the default (PWN_TILED_INIT_TIMEOUT_MS / PWN_TILED_WAIT_TIMEOUT_MS in the environment,
 *                        else 120 s / 60 s).
 *   pwn_tiled_preflight  this rank, no tiling needed: what a first multi-GPU run wants to know before it starts, as one
 *                        JSON object in `json` -- the devices this process sees and, from the context's device, which of
 *                        them it can reach directly (hipDeviceCanAccessPeer), the librccl that dlopen resolved (path and
 *                        version), how the communicator will be driven (PWN_TILED_RCCL_MODE) and the deadlines.  Returns
 *                        the length written (the text is cut at n - 1), or PWN_E*.
 * PWN_TRANSPORT_SHM moves the same messages through POSIX shared memory instead: for tests
 * on a box with one GPU, where RCCL cannot run two ranks; the ranks may share a device.
 */
#define PWN_TILED_ID_BYTES 128
#define PWN_TRANSPORT_RCCL 0
#define PWN_TRANSPORT_SHM  1
#define PWN_TRANSPORT_LOCAL 2      /* between the members of a group inside one process (pwn_init_multi): device-to-device copies behind events */
#define PWN_TILED_HOST     1
#define PWN_TILED_SLOTS    6       /* frames a host sink holds (at most five in flight and the one being reused) */
#define PWN_TILED_MAX_WORLD 64
#define PWN_TILED_ROOT_FIXED  0
#define PWN_TILED_ROOT_ROTATE 1
typedef struct pwn_tiled_frame
{
	const void *d_sbuf;          /* the frame's root (rank 0 unless pwn_tiled_gather_root): the frame on the device, BGRA8, pitch = width; NULL elsewhere */
	const uint32_t *sbuf;        /* the root with PWN_TILED_HOST: pinned host copy; with a host sink: the frame, on every rank */
	uint64_t seq;                /* 1, 2, ... in submission order */
	int redone;                  /* 1: a tap left the halo and the frame was repeated with whole strips */
	int timed;                   /* PWN_OPT_FRAME_TIMING sampled this frame: */
	float trace_ms, frame_ms;    /*   this rank's trace kernel; its trace .. blur incl. waiting for the exchange */
	float blur_ms;               /*   its blur kernel */
	float halo_ms, gather_ms;    /*   the two grouped exchanges: this frame's halo rows (G1); the gather that carried this frame's
	                                  strips and words (G2; split choreography: 0 when pwn_tiled_wait had to launch it itself) */
	float enqueue_us;            /* host time inside pwn_tiled_submit for this frame (every frame) */
	int y0, y1;                  /* the rows this rank traced of this frame (the cuts move: pwn_tiled_balance) */
	uint32_t cost;               /* what they cost: sum of the trace waves' lifetimes, ticks of the GPU's 100 MHz clock */
	int root;                    /* the rank this frame was gathered on (pwn_tiled_gather_root; -1 with a host sink) */
} pwn_tiled_frame;
typedef struct pwn_tiled_info
{
	int rank, world, y0, y1, rows_per_rank, halo_rows, transport;      /* y0, y1: this rank's rows of the NEXT frame */
	uint64_t frames, frames_redone, groups;        /* delivered frames; repeated ones; grouped exchanges launched */
	uint64_t bytes_sent, bytes_received;           /* by this rank */
	uint64_t bytes_to_host;                        /* host sink: copied into the host frame by this rank */
	int host_sink;                                 /* 1: every rank delivers its strip to the host (pwn_tiled_host_sink) */
	int max_rows;                                  /* the tallest strip a rank may be given (1.5 equal strips) */
	int balance_every;                             /* pwn_tiled_balance */
	int grid_reserve;                              /* workgroups the trace grid leaves free for RCCL's kernels (pwn_tiled_set_reserve) */
	int two_streams;                               /* 1: frames alternate between two compute streams (PWN_OPT_FRAME_OVERLAP at init) */
	uint64_t recuts;                               /* how often the cuts moved */
	int gather_root;                               /* PWN_TILED_ROOT_* (pwn_tiled_gather_root) */
	int rccl_nonblocking;                          /* RCCL transport: 1 = a non-blocking communicator, every call polled against the deadline
	                                                  (PWN_TILED_RCCL_MODE=nonblocking); 0 = a blocking one, bring-up on a helper thread under
	                                                  the deadline (the default) */
	int init_timeout_ms, wait_timeout_ms;          /* pwn_tiled_set_timeouts, as in force */
	int dead;                                      /* 1: a deadline passed or the transport failed; the communicator is gone */
	int compute_streams;                           /* 1, 2 or 3: frame f runs on compute stream f mod this (PWN_OPT_FRAME_OVERLAP, PWN_OPT_TILED_STREAMS) */
	int choreography;                              /* PWN_TILED_CHOREO_* as fixed at pwn_tiled_init */
	int communicators;                             /* RCCL transport: communicators in use (PWN_OPT_TILED_COMMS); 0 over shared memory */
} pwn_tiled_info;
int pwn_tiled_unique_id(void *id128, int transport);
int pwn_tiled_init(pwn_ctx *ctx, int rank, int world, const void *id128, int transport, int halo_rows);
int pwn_tiled_submit(pwn_ctx *ctx, const float cam[16], float sec_current);
int pwn_tiled_wait(pwn_ctx *ctx, int flags, pwn_tiled_frame *out);
int pwn_tiled_host_sink(pwn_ctx *ctx, void *base, size_t bytes);
int pwn_tiled_gather_root(pwn_ctx *ctx, int mode);
int pwn_tiled_get_info(pwn_ctx *ctx, pwn_tiled_info *out);
void pwn_tiled_shutdown(pwn_ctx *ctx);
int pwn_tiled_set_timeouts(pwn_ctx *ctx, int init_ms, int wait_ms);
int pwn_tiled_preflight(pwn_ctx *ctx, char *json, size_t n);
/*
 * Moving cuts.  Equal strips are not equal work (the horizon band of level.txt costs 1.2-1.3x the mean strip of an
 * 8-way tiling), and the reference's answer to that -- OpenMP's static schedule over 32-row chunks, screen.h:63-64 --
 * is the equal split.  Here every rank's trace launch measures what its rows cost (the sum of its waves' lifetimes),
 * the number travels to every rank with the frame's miss word, and every `every_frames` delivered frames all ranks
 * compute the same new cuts from the same numbers: piecewise-linear cost over the rows, cut k where it reaches k / world
 * of the total, multiples of 8 rows, every strip at least the halo and at most pwn_tiled_info.max_rows rows.  New cuts
 * take effect with the next submitted frame; a frame in flight keeps the cuts it was traced with (exchange, blur,
 * gather, host-sink copies, and the repeat after a missed halo all use the frame's own).
 *   pwn_tiled_balance   collective (the same call on every rank, between frames): the period in delivered frames,
 *                       0 = the cuts stay where they are.  Default 8 (PWN_TILED_BALANCE=k in the environment
 *                       overrides; 0 when a strip of the equal split would be empty, or without blur).
 *   pwn_tiled_set_cuts  collective: n = world + 1 boundaries, 0 = cuts[0] < cuts[1] < ... < cuts[world] = height,
 *                       inner ones multiples of 8, strips within [halo, max_rows]; for the next submitted frame.
 *   pwn_tiled_get_cuts  the cuts of the next frame (world + 1 ints) and, if cost != NULL, every rank's cost word of
 *                       the last delivered frame (world words); returns world + 1.
 *   pwn_tiled_set_reserve  this rank, between frames: workgroups the persistent trace grid leaves free so that
 *                       RCCL's send / recv kernels find a CU to start on (default 16 with the RCCL transport, 0 = fill
 *                       every CU; PWN_TILED_RESERVE in the environment sets the default).
 */
int pwn_tiled_balance(pwn_ctx *ctx, int every_frames);
int pwn_tiled_set_cuts(pwn_ctx *ctx, const int *cuts, int n);
int pwn_tiled_get_cuts(pwn_ctx *ctx, int *cuts, uint32_t *cost);
int pwn_tiled_set_reserve(pwn_ctx *ctx, int workgroups);
/* the re-cut rule by itself (no context, no device): cuts[world + 1] and the strips' costs in, out[world + 1]; returns 1
   if the cuts moved, 0 if they stay (balanced within 2 %, a zero cost, constraints that cannot be met) */
int pwn_tiled_recut(const int *cuts, const uint32_t *cost, int world, int height, int min_rows, int max_rows, int *out);

/* screen_upscale (screen.h:126-149): replicate every pixel scale x scale into
   a surface of `pitch_bytes` per row (SDL_Surface->pitch / ->pixels).
   Host form (uploads sbuf... uses the last frame on the device if src is NULL:
   the last pwn_trace_screen_centred's, zeros before the first; a frame in flight
   submitted since under two or more blur passes has left its first pass there,
   see "shared" at pwn_frames_config) and device form. */
int pwn_screen_upscale(pwn_ctx *ctx, const uint32_t *sbuf, int scale, int pitch_bytes,
	uint32_t *pixels);
int pwn_upscale_device(pwn_ctx *ctx, const void *d_src, int scale, int pitch_bytes,
	void *d_dst, void *stream);

int pwn_get_stats(pwn_ctx *ctx, pwn_stats *out);

/* device-side probes of the arithmetic primitives (rcp/rsqrt tables, sinf,
   cosf, expf, sqrt, divide, colour pack, LCG); used by the parity tests.
   op: see PWN_PROBE_*; in/out are HOST arrays of n 32-bit words. */
#define PWN_PROBE_RCP    0
#define PWN_PROBE_RSQRT  1
#define PWN_PROBE_SINF   2
#define PWN_PROBE_COSF   3
#define PWN_PROBE_EXPF   4
#define PWN_PROBE_SQRT   5
#define PWN_PROBE_DIV    6  /* in = pairs (a,b), out = a/b */
#define PWN_PROBE_FTOINT 7  /* in = 4 floats per output word (util.h:48-59) */
#define PWN_PROBE_RANDFS 8  /* in = seed, out = randfs bits (util.h:13-16) */
#define PWN_PROBE_SIN_OF_PAIR 9   /* sinf / cosf halves of the joint sincos used for */
#define PWN_PROBE_COS_OF_PAIR 10  /* the floor normal (trace.h:45-46)                 */
int pwn_probe(pwn_ctx *ctx, int op, const uint32_t *in, uint32_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif
