// trace_refill.hip -- the portal ray-march with wave64 ballot / prefix refill of live rays.
//
// Same arithmetic as trace_kernel.hip (trace_ray_prelude, screen.h:1-28, and trace.h), different schedule: a ray
// segment's set-up, cell step, shading, bounces, jitter and composite are the same text (trace_setup.inc,
// trace_walk.inc, trace_shade.inc, trace_bounce.inc, trace_jitter.inc, trace_composite.inc); what a kernel does
// between them -- the composite stack's push, segment and depth bookkeeping, the stores -- is its own.
// There a wave64 takes a 16x4-pixel
// unit and its 64 lanes run ray set-up, walk and shading in step, three times per pixel
// (REFLECT = 2): a lane whose ray ended waits until the slowest ray of the wave has ended, and
// a lane whose pixel is finished waits for the whole unit.  Rays differ a lot -- portal chains,
// mirror halls -- so the walk loop ran with 0.89 (level.txt), 0.88 (synth64) and 0.74
// (synth256) of its lanes active.
//
// Here a wave is one persistent walk loop.  Every lane carries its own pixel (output offset,
// bounce depth, composite stack, seed) and its own ray.  The loop runs
//
//   A  for the lanes whose ray has ended:  shade; then either bounce (a new ray for the same
//      pixel) or finish the pixel (composite, store) and take a NEW pixel: the lanes that need
//      one are found with a ballot, each takes pixel `handed_out + mbcnt(ballot)` of the wave's
//      current 16x4 unit (prefix rank = compaction of the requests onto consecutive pixels), and
//      the wave pulls the next unit from the work queues when the current one is used up;
//      ray set-up for every lane that got a new ray;
//   B  cell steps for the lanes that walk, until the rays set up in the last pass have all
//      ended, or until the ended ones have waited P.refill_limit lane-steps in sum: rays still
//      walking then are stragglers, and nobody waits for a straggler twice.
//
// Phase A is one pass of straight code whatever the number of lanes that need it (and it is
// 43 % of the kernel's time), so it is entered when a batch of lanes is ready, not per ray.
//
// The per-tile ray add-chain (screen.h:12-18) is still built systolically with DPP by all 64
// lanes when a unit is taken, and parked in LDS (3 or 4 x 64 floats per wave) where the lane that
// is handed pixel p reads entry p.
#include <hip/hip_runtime.h>
#include "trace_common.h"

enum { EV_IDLE = 4, EV_SETUP = 5, EV_DONE = 6 };      // lane states beyond EV_NONE (walking) .. EV_EXHAUSTED

#define RTAB_FLOATS(HAS_W) (((HAS_W) ? 4 : 3) * 64)

template<bool COUNT, bool HAS_W>
__global__ void __launch_bounds__(PWN_BLOCK, PWN_MIN_WAVES)
pwn_trace_refill_kernel(pwn_trace_params P)
{
	constexpr int LISTS = PWN_LF_INDEXED;          // (this scheduler reads the indexed lists: pwn_i_pack_blob packs those for it)
	constexpr bool HITREC = false;       // (trace_walk.inc: nothing kept for hit records; the two names it would write, never touched)
	[[maybe_unused]] uint32_t hit_cxz;
	[[maybe_unused]] int hit_portals;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

	blob_to_lds(lds_raw, P.blob, P.blob_bytes);
	__syncthreads();

	// (the tables are addressed from LDS address 0 on, trace_common.h; the launcher checks that this kernel has
	// no static LDS in front of the dynamic allocation)
	const Lds L = lds_tables(P.off_sph);

	typedef Vec<HAS_W> V;
	V rayb, rdx, rdy, cam_from;
	rayb.x = P.rayb[0]; rayb.y = P.rayb[1]; rayb.z = P.rayb[2]; rayb.w = HAS_W ? P.rayb[3] : 0.0f;
	rdx.x = P.rdx[0]; rdx.y = P.rdx[1]; rdx.z = P.rdx[2]; rdx.w = HAS_W ? P.rdx[3] : 0.0f;
	rdy.x = P.rdy[0]; rdy.y = P.rdy[1]; rdy.z = P.rdy[2]; rdy.w = HAS_W ? P.rdy[3] : 0.0f;
	cam_from.x = P.from[0]; cam_from.y = P.from[1]; cam_from.z = P.from[2]; cam_from.w = HAS_W ? P.from[3] : 1.0f;
	const float sec_current = P.sec_current;

	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int l16 = lane & 15;
	// this wave's ray table: component-major, one float per pixel of the current unit
	float *rtab = (float *)(lds_raw + ((P.blob_bytes + 15u) & ~15u)) + wave * RTAB_FLOATS(HAS_W);

	Counters cnt = {};
	// PWN_OPT_WAVE_LOG: when was this wave resident (the GPU's constant 100 MHz clock)
	unsigned long long t_begin = 0ull;
	if(P.wave_log != NULL) t_begin = __builtin_amdgcn_s_memrealtime();

	// ---- work queues (as in trace_kernel.hip: PWN_QUEUES counters 128 B apart, queue q holds the
	// units u = q (mod PWN_QUEUES); a wave drains its home queue, then helps with the others, and
	// asks for its next unit when it takes one, so the round trip of the atomic hides behind the
	// unit's 64 pixels).  The counters of the NEXT launch of this context are cleared here.
	const uint32_t units_x = ((uint32_t)P.w + 15u) >> 4;
	const uint32_t rows_u = ((uint32_t)(P.y1 - P.y0) + 3u) >> 2;
	const uint32_t units = units_x * rows_u;
	if(blockIdx.x == 0 && threadIdx.x < PWN_QUEUES) P.tickets_next[threadIdx.x * PWN_QUEUE_STRIDE] = 0u;
	if(blockIdx.x == 0 && threadIdx.x == PWN_QUEUES && P.clear_word != NULL) *P.clear_word = 0u;
	uint32_t q = (blockIdx.x * (PWN_BLOCK / 64) + (uint32_t)wave) % PWN_QUEUES;
	uint32_t ticket_v = 0;                 // lane 0: the ticket drawn ahead for queue q
	if(lane == 0) ticket_v = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], 1u);
	int misses = 0;
	bool more_units = true;
	uint32_t handed = 64u;                 // pixels of the current unit already handed out (64: none left)
	int unit_x0 = 0, unit_y0 = 0;          // its origin in the frame

	// ---- per lane: the pixel
	int ev = EV_IDLE;
	uint32_t o = 0u, seed = 0u;
	int depth = 0;
	// icol (screen.h:24; trace.h:90 for a bounced ray) is the colour of the composite stack's top entry (trace_kernel.hip)
	float st_refl0 = 0.0f, st_refl1 = 0.0f, st_fog0 = 0.0f, st_fog1 = 0.0f;
	float sc0x = 1.0f, sc0y = 1.0f, sc0z = 1.0f, sc1x = 0.0f, sc1y = 0.0f, sc1z = 0.0f;
#define icx sc0x
#define icy sc0y
#define icz sc0z
	float w_acc = 0.0f;                                 // stand-in for the colour's w lane (trace_kernel.hip)
	// ---- per lane: the ray (trace.h:186-248)
	V pos, ray, aux_pos;
	pos.x = pos.y = pos.z = pos.w = 0.0f; ray = pos; aux_pos = pos;
	float cdist = 0.0f, fog = 0.0f, aux_dist = __builtin_inff(), aux_diff = 0.0f;
	uint32_t aux_idx = 0u;
	uint32_t cxz = 0u, sx = 1u, sz = 1u << 16;         // cell x | z << 16 and the steps (gx, 0), (0, gz): trace_common.h
	int ldx = FXP, ldz = FZP, ldy = FYP, ldir = FYN, base = BASE_ROOM_Y, maxsteps = 0;
	float wx = 0.0f, wy = 0.0f, wz = 0.0f, iax = 0.0f, iay = 0.0f, iaz = 0.0f, iay_dn = 0.0f;
	uint32_t iay_up_bits = 0u, cw = 0u;

	const int limit = P.refill_limit;                   // lane-steps the ended rays of a batch wait for the others in sum

#pragma unroll 1
	for(;;)
	{
		// =========================================================== A.1: rays that ended
		if(ev >= EV_WALL && ev <= EV_EXHAUSTED)
		{
			if(COUNT) { cnt.apass_lanes++; if((__ffsll((long long)__ballot(1)) - 1) == lane) cnt.apasses++; }
			float vx, vy, vz, vw;
			bool finished;
			if(ev == EV_EXHAUSTED)
			{
				// trace.h:677-678: out of steps -- the walked ray is the colour; a primary ray leaves the old depth in place
				if(COUNT) cnt.exhausted++;
				vx = ray.x; vy = ray.y; vz = ray.z; vw = HAS_W ? ray.w : 0.0f;
				finished = true;
			}
			else
			{
				if(ev == EV_WALL && base == BASE_ROOM_Y) { ldir = ldy; base = (ldy == FYP ? BASE_CEIL : BASE_FLOOR); }
				// zbuf = the PRIMARY ray's hit distance (trace.h:102-105)
				if(depth == 0) P.zbuf[o] = (ev == EV_SPHERE ? aux_dist : cdist);

				// (the segment's colour is computed into the pixel's own registers, as in trace_kernel.hip)
				float refl;
				V aux_norm;
				aux_norm.x = aux_norm.y = aux_norm.z = aux_norm.w = 0.0f;
#define colx vx
#define coly vy
#define colz vz
#include "trace_shade.inc"

				// trace.h:3-7
				if(depth >= REFLECT_MAX || refl == 0.0f) { vw = 0.0f; finished = true; }
				else
				{
#include "trace_bounce.inc"
					// (the jitter goes into the ray in place: set-up below takes the next segment's direction from there)
#define iray ray
#include "trace_jitter.inc"
#undef iray

					// the composite stack as a shift register; its top entry's colour is the next segment's icol
					st_refl1 = st_refl0; st_fog1 = st_fog0; sc1x = sc0x; sc1y = sc0y; sc1z = sc0z;
					st_refl0 = refl; st_fog0 = fog; sc0x = colx; sc0y = coly; sc0z = colz;
					depth++;
					// the bounced ray starts at pos with direction ray (trace.h:90): set up below
					ev = EV_SETUP;
					finished = false;
					vx = vy = vz = vw = 0.0f;
				}
#undef colx
#undef coly
#undef colz
			}
			if(finished)
			{
				// trace.h:91-101
#include "trace_composite.inc"
				// screen.h:22 (col_ftoint, util.h:48-59)
				P.sbuf[o] = col_pack4(vx, vy, vz, vw + w_acc);
				ev = EV_IDLE;
			}
		}

		// =========================================================== A.2: new pixels
		// Lanes without a pixel take the next ones of the wave's unit: the k-th requesting lane
		// (k = number of requesting lanes below it: mbcnt of the ballot) takes pixel handed + k.
		{
			unsigned long long need = __ballot(ev == EV_IDLE);
			while(need != 0ull)
			{
				if(handed >= 64u)
				{
					// ---- the next unit (everything here is wave-uniform; all 64 lanes take part)
					bool got = false;
					uint32_t unit = 0u;
					if(more_units)
					{
						uint32_t ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket_v);
						for(;;)
						{
							// units of queue q: q, q + Q, ...  below `units`
							const uint32_t qlen = (units + PWN_QUEUES - 1u - q) / PWN_QUEUES;
							if(ticket < qlen) { got = true; unit = ticket * PWN_QUEUES + q; break; }
							// A wave that keeps finding queues empty although they looked open stops helping:
							// every queue is drained by its home waves anyway, and this bounds the loop
							// whatever the loads return.
							if(++misses > 2 * (int)PWN_QUEUES) break;
							uint32_t seen = 0xffffffffu;
							// = lane, opaque: keeps the address below out of the kernel's prologue (trace_kernel.hip)
							uint32_t ql = 0u;
							asm volatile("" : "+v"(ql));
							ql = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, ql));
							if(ql < PWN_QUEUES)
								seen = __hip_atomic_load(&P.tickets[ql * PWN_QUEUE_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							const uint32_t len_l = (units + PWN_QUEUES - 1u - (ql & (PWN_QUEUES - 1u))) / PWN_QUEUES;
							const unsigned long long open = __ballot(ql < PWN_QUEUES && seen < len_l);
							if(open == 0ull) break;
							q = next_open_queue(q, open);
							uint32_t t = 0;
							if(lane == 0) t = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], 1u);
							ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
						}
					}
					if(!got)
					{
						// no units left: the requesting lanes are done for good
						more_units = false;
						if(ev == EV_IDLE) ev = EV_DONE;
						break;
					}
					misses = 0;
					if(lane == 0) ticket_v = atomicAdd(&P.tickets[q * PWN_QUEUE_STRIDE], 1u);     // the next one, drawn ahead
					// rows from the middle of the strip outwards: the horizon band, where rays run longest,
					// is started first and the cheap top and bottom edges make up the tail
					const uint32_t ux = unit % units_x, k = unit / units_x;
					const uint32_t mid = rows_u >> 1;
					uint32_t uy;
					{
						const uint32_t d = (k + 1u) >> 1;
						const bool down = (k & 1u) != 0u;            // odd: above the middle
						int cand = down ? (int)mid - (int)d : (int)mid + (int)d;
						if(cand < 0) cand = (int)mid + (int)(k - mid);           // ran past the top: the remaining rows are at the bottom
						else if(cand >= (int)rows_u) cand = (int)mid - (int)(k - (rows_u - 1u - mid));   // ran past the bottom
						uy = (uint32_t)cand;
					}
					const int half = (int)(ux & 1u);                  // left / right half of the 32-wide tile
					const int cx0 = (int)(ux >> 1) * 32;              // the 32-pixel tile of screen.h:6-7 this unit is in
					unit_x0 = (int)ux * 16; unit_y0 = P.y0 + (int)uy * 4;
					const int y = unit_y0 + (lane >> 4);
					// screen.h:12-18 in the reference build's evaluation order, the add-chain built systolically
					// over the 16 lanes of a DPP row (see trace_kernel.hip)
					V rayl = vadd<HAS_W>(vadd<HAS_W>(vscale<HAS_W>((float)cx0, rdx), rayb), vscale<HAS_W>((float)y, rdy));
					if(half)
					{
#pragma unroll
						for(int j = 0; j < 16; j++) rayl = vadd<HAS_W>(rayl, rdx);
					}
					rayl = vadd<HAS_W>(rayl, rdx);
					{
						const bool first = (l16 == 0);
						V add;
						add.x = first ? rayl.x : rdx.x; add.y = first ? rayl.y : rdx.y; add.z = first ? rayl.z : rdx.z;
						add.w = HAS_W ? (first ? rayl.w : rdx.w) : 0.0f;
#pragma unroll
						for(int j = 1; j < 16; j++)
						{
							rayl.x = dpp_row_shr1(rayl.x) + add.x;
							rayl.y = dpp_row_shr1(rayl.y) + add.y;
							rayl.z = dpp_row_shr1(rayl.z) + add.z;
							if constexpr(HAS_W) rayl.w = dpp_row_shr1(rayl.w) + add.w;
						}
					}
					rtab[lane] = rayl.x; rtab[64 + lane] = rayl.y; rtab[128 + lane] = rayl.z;
					if constexpr(HAS_W) rtab[192 + lane] = rayl.w;
					handed = 0u;
				}
				// ---- hand out: prefix rank among the requesting lanes
				const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
				const uint32_t p = handed + rank;
				if(ev == EV_IDLE && p < 64u)
				{
					const int x = unit_x0 + (int)(p & 15u), y = unit_y0 + (int)(p >> 4);
					// (a pixel beyond the frame's edge is used up and the lane asks again)
					if(x < P.w && y < P.y1)
					{
						pos = cam_from;
						ray.x = rtab[p]; ray.y = rtab[64u + p]; ray.z = rtab[128u + p];
						if constexpr(HAS_W) ray.w = rtab[192u + p]; else ray.w = 0.0f;
						o = (uint32_t)y * (uint32_t)P.w + (uint32_t)x;
						seed = pixel_seed(x, y, P.w);
						depth = 0; sc0x = sc0y = sc0z = 1.0f; w_acc = 0.0f;
						ev = EV_SETUP;
					}
				}
				handed = min(64u, handed + (uint32_t)__builtin_popcountll(need));
				need = __ballot(ev == EV_IDLE);
			}
		}

		// =========================================================== A.3: ray set-up (trace.h:186-248)
		unsigned long long fresh = __ballot(ev == EV_SETUP);
		if(ev == EV_SETUP)
		{
			// (this kernel starts every segment with an empty sphere candidate)
			aux_diff = 0.0f; aux_idx = 0u;
			aux_pos.x = aux_pos.y = aux_pos.z = aux_pos.w = 0.0f;
			// the direction came in `ray` (a new pixel's from the ray table, a bounced ray's from the jitter)
			const V iray = ray;
			bool gyp;          // (this kernel keeps ldy)
#include "trace_setup.inc"
			(void)gyp;
			maxsteps = 1000;
		}

		// =========================================================== B: the walk (trace.h:250-675)
		// When to stop walking and make a pass of phase A for the rays that have ended?  Rays of one
		// wave are coherent: started together they mostly end within a few steps of each other, and a
		// ray that ended early is best left waiting for them, so that the pass (one stretch of code
		// whatever the number of lanes in it, 43 % of the kernel's time) runs once for all 64.  Leaving
		// at the first ended ray, or with a fixed number of lanes or steps, splits every such group in
		// two that then wait for each other: measured +60 % time.  What must not hold a wave up is the
		// ray that walks ten or a hundred times as far (portal chains, mirror halls).  So:
		//   - walk while a YOUNG ray (set up in the pass just made) is walking;
		//   - but stop once the lanes whose ray has ended have waited `limit` lane-steps in sum: a pass
		//     costs about as much as four cell steps of the whole wave, so waiting longer than that for
		//     the rest of a batch is what a pass would have bought (the ski-rental bound);
		//   - rays still walking then are stragglers; they stay in their lanes and walk along with the
		//     next batches, and nobody waits for a straggler a second time.
		const unsigned long long walking0 = __ballot(ev == EV_NONE);
		if(walking0 == 0ull) break;           // every lane is EV_DONE: set-up leaves no other state behind
		if(fresh == 0ull) fresh = walking0;   // nothing was set up in this pass: the walkers are the batch
		int waited = 0;
		if(ev == EV_NONE)
		{
			asm volatile("" : "+v"(iay_up_bits));        // keep it a register, not a select per step (trace_kernel.hip)
			bool on;
#pragma unroll 1
			do
			{
#define WALK_EV_KEEP 0
#define WALK_EV_OPEN(e) ((e) == 0)
#include "trace_walk.inc"
#undef WALK_EV_KEEP
#undef WALK_EV_OPEN
				// wave-uniform: a young ray still walks, and the ended ones have not waited too long
				const unsigned long long w = __ballot(ev == EV_NONE);
				waited += (int)__builtin_popcountll(walking0 & ~w);
				on = (w & fresh) != 0ull && waited < limit;
				maxsteps--;
			} while(ev == EV_NONE && maxsteps != 0 && on);
			asm volatile("" : "+v"(ev), "+v"(maxsteps));
			// trace.h:250,677: out of steps
			if(ev == EV_NONE && maxsteps == 0) ev = EV_EXHAUSTED;
			// what the ray ended on is read back from the register (see trace_kernel.hip)
			asm volatile("" : "+v"(ev));
		}
	}

	if(COUNT)
	{
		// (no region counts: the issue model maps the units kernel.  The shared texts' RG() still count into cnt.rg[] in this
		// kernel's counting variants; nothing reads them -- dead work in a diagnostics build, part of its 40 / 20 bytes of scratch)
#define PWN_CNT_REGIONS 0
#include "trace_counters.inc"
#undef PWN_CNT_REGIONS
	}
	// PWN_OPT_WAVE_LOG: every wave's lifetime
	if(P.wave_log != NULL && wave_first_lane())
	{
		unsigned long long *wl = wave_log_slot(P.wave_log);
		wl[0] = t_begin; wl[1] = __builtin_amdgcn_s_memrealtime();
	}
}

typedef TraceKernels<pwn_trace_refill_kernel<true, true>, pwn_trace_refill_kernel<true, false>,
	pwn_trace_refill_kernel<false, true>, pwn_trace_refill_kernel<false, false>> Refill;

extern "C" hipError_t pwn_launch_trace_refill(const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream)
{
	return Refill::launch(P, grid, lds_bytes, count, stream);
}

// LDS a workgroup needs beyond the table blob: the waves' ray tables
extern "C" unsigned pwn_trace_refill_lds_extra(bool has_w)
{
	return (unsigned)((PWN_BLOCK / 64) * RTAB_FLOATS(has_w) * sizeof(float));
}

extern "C" int pwn_trace_refill_blocks_per_cu(size_t lds_bytes, bool count, bool has_w)
{
	return Refill::blocks_per_cu(lds_bytes, count, has_w);
}
