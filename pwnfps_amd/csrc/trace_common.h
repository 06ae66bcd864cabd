// trace_common.h -- what the two trace kernels share that is not a ray segment's arithmetic
// (trace_kernel.hip: a wave64 traces 16x4-pixel units in step; trace_refill.hip: lanes are
// refilled with new rays by ballot + prefix rank while the others walk on):
//   - constants, the LDS table pointers, the packed cell coordinates, Vec and its operations, the counters;
//   - small pieces of the scheduling code as inline functions: pixel_seed, blob_to_lds, next_open_queue,
//     wave_log_slot, wave_first_lane (each leaves the units kernel's assembly as it was);
//   - the host side: launch_kernel / kernel_blocks_per_cu for one instantiation, TraceKernels for the four
//     a launch's count and has_w pick from.
// The segment's arithmetic itself is one text per piece, textually included by both kernels: trace_setup.inc,
// trace_walk.inc (with trace_sphere.inc), trace_shade.inc, trace_bounce.inc, trace_jitter.inc,
// trace_composite.inc; trace_counters.inc flushes the counters.  Each says at its top which names it
// expects in scope and which it writes.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "dev_math.h"
#include "tables.h"

#define EPS 0.0000000000001f      // defs.h:1
#define REFLECT_BLUR_F 0.03f      // defs.h:5
#define REFLECT_MAX 2             // defs.h:7
enum { FXP = 0, FZP, FXN, FZN, FYP, FYN };   // defs.h:25-33

// workgroup = PWN_BLOCK threads sharing one copy of the blob in LDS; a wave's unit of work is
// 16 x 4 pixels (half the width of the 32-pixel tile of screen.h:6-7, one DPP row per pixel row)
#ifndef PWN_BLOCK
#define PWN_BLOCK 256
#endif
#define TILE_W 16
#define TILE_H 4

// min waves per SIMD the register allocator must leave room for (Makefile MINW)
#ifndef PWN_MIN_WAVES
#define PWN_MIN_WAVES 3
#endif

// The tables of the blob sit at CONSTANT offsets of the workgroup's LDS (tables.h; the kernels have no static
// __shared__ data, so the dynamic allocation they are copied into starts at LDS address 0 -- the kernels check
// that once).  They are addressed through LDS-address-space pointers made from those constants, so a table
// access is a ds_read with an immediate offset; through the `extern __shared__` symbol every access adds that
// symbol's address (0, but known too late to fold): 21 `v_add_u32 v, 0, v` in the kernel, one per cell step.
#define PWN_LDS __attribute__((address_space(3)))
// (the kernel's arguments where the hardware puts them: pwn_trace_params is the one argument of both trace kernels, at offset 0)
#define PWN_KARGS __attribute__((address_space(4)))
template<class T> __device__ __forceinline__ const PWN_LDS T *lds_at(uint32_t byte) { return (const PWN_LDS T *)(uintptr_t)byte; }
// (16-byte LDS loads as a built-in vector type: HIP's float4 class has no constructor from another address space)
typedef float pwn_f4 __attribute__((ext_vector_type(4)));
struct Lds
{
	const PWN_LDS uint32_t *cellinfo;
	const PWN_LDS uint16_t *rcp, *rsq;
	const PWN_LDS unsigned char *eprec;   // the portals' endpoint records (cell_bake.h), set back by the two states that have none: see ep_rec
	const PWN_LDS uint16_t *binidx;
	const PWN_LDS uint16_t *recsph;       // inline sphere records (tables.h): which sphere a record is of
	const PWN_LDS float *sph;
	const PWN_LDS uint64_t *exp2;         // tables.h PWN_T_EXP2
	const PWN_LDS pwn_f4 *faces;           // tables.h PWN_T_FACES: [0..4) wall colours, [4 + 2 * face ..] face constants
	// the lists' global form (tables.h PWN_LF_GLOBAL; lds_tables_global): binidx is then `liststart`, u32 per non-empty cell, and
	// these three are the device-memory sections -- records, which sphere (an index), spheres.  Not set otherwise.
	const pwn_f4 *g_rec;
	const uint32_t *g_which;
	const pwn_f4 *g_sph;
};
__device__ __forceinline__ Lds lds_tables(uint32_t off_sph, uint32_t off_recsph = 0u)
{
	Lds L;
	L.cellinfo = lds_at<uint32_t>(PWN_T_CELLINFO);
	L.rcp = lds_at<uint16_t>(PWN_T_RCP);
	L.rsq = lds_at<uint16_t>(PWN_T_RSQ);
	L.eprec = lds_at<unsigned char>(PWN_T_EPREC - PWN_PST_REC0 * 4u);
	L.binidx = lds_at<uint16_t>(PWN_T_BINIDX);
	L.faces = lds_at<pwn_f4>(PWN_T_FACES);
	L.exp2 = lds_at<uint64_t>(PWN_T_EXP2);
	L.sph = lds_at<float>(off_sph);
	L.recsph = lds_at<uint16_t>(off_recsph);
	L.g_rec = nullptr; L.g_which = nullptr; L.g_sph = nullptr;
	return L;
}
__device__ __forceinline__ Lds lds_tables_global(const pwn_trace_params &P)
{
	Lds L = lds_tables(0u);
	L.g_rec = (const pwn_f4 *)P.g_rec; L.g_which = P.g_which; L.g_sph = (const pwn_f4 *)P.g_sph;
	return L;
}

// util.h:151-158 (per-axis clamp to 0) -> the packed cell word.  The table has
// 65 rows / columns; index 64 repeats index 0 (tables.h), so the clamp is a min.
__device__ __forceinline__ uint32_t cellword_at(const Lds &L, int cx, int cz)
{
	uint32_t ux = min((uint32_t)cx, 64u), uz = min((uint32_t)cz, 64u);
	return L.cellinfo[uz * PWN_GRID_PITCH + ux];
}

// The walk keeps the cell coordinates as two signed 16-bit fields of ONE register (x low, z high; a ray
// makes at most 1000 steps from a cell of the 64 x 64 grid, so 16 bits hold them), and its per-axis steps
// (gx, 0) / (0, gz) the same way.  A cell step is then one packed add, get_cell's per-axis clamp one
// packed unsigned min (a negative coordinate is a large unsigned one: 64, the repeat of index 0) and
// the byte offset x*4 + z*260 one v_dot2_u32_u16: 4 VALU where separate ints took 9.
typedef unsigned short pwn_us2 __attribute__((ext_vector_type(2)));
typedef short pwn_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cxz_pack(int cx, int cz) { return ((uint32_t)cx & 0xffffu) | ((uint32_t)cz << 16); }
// The cell a segment STARTS in comes from a float position, which can be anything -- a ray that came back from
// 10^13 units away, an infinity (the conversion saturates to INT_MIN / INT_MAX): 16 bits would fold such a cell
// back into or near the grid.  A start further out than 16383 cells is outside the grid for all of the
// segment's <= 1000 steps whatever its exact number, so it is pinned there.  (Found by lattice scenes of
// tools/fuzz_parity.py, seeds 9002 / 9004: tests/golden/far_starts.npz.)
__device__ __forceinline__ uint32_t cxz_pack_start(int cx, int cz)
{
	return cxz_pack(max(min(cx, 16383), -16384), max(min(cz, 16383), -16384));
}
__device__ __forceinline__ int cxz_x(uint32_t c) { return (int)(int16_t)(uint16_t)(c & 0xffffu); }
__device__ __forceinline__ int cxz_z(uint32_t c) { return (int)c >> 16; }
__device__ __forceinline__ uint32_t cxz_add(uint32_t c, uint32_t step)
{
	return __builtin_bit_cast(uint32_t, (pwn_s2)(__builtin_bit_cast(pwn_s2, c) + __builtin_bit_cast(pwn_s2, step)));
}
__device__ __forceinline__ uint32_t cellword_pk(const Lds &L, uint32_t cxz)
{
	const pwn_us2 lim = { 64, 64 }, pitch = { 4, (unsigned short)(PWN_GRID_PITCH * 4u) };
	const pwn_us2 c = __builtin_elementwise_min(__builtin_bit_cast(pwn_us2, cxz), lim);
	const uint32_t byte = __builtin_amdgcn_udot2(c, pitch, 0u, false);
	return *(const PWN_LDS uint32_t *)((const PWN_LDS unsigned char *)L.cellinfo + byte);
}

// The endpoint record of a portal cell whose state says it has one (cell_bake.h): the state field sits at bit 2 of the cell
// word and a record is 4 bytes -- the field in place is the record's byte offset.  What comes back is what the reference adds
// to the position on the way to the other endpoint: x, z (two half floats, exact for these whole numbers).
static_assert(PWN_C_PST_SHIFT == 2u && PWN_T_EPREC + PWN_EP_MAX * 4u <= PWN_T_BINIDX, "ep_rec takes the state field as a byte offset; 52 records fit");
// The rotation of an endpoint cell (PWN_C_PROT_SHIFT) sits in the two bits that say which way a ramp tilts: they are read behind
// PWN_C_RAMP only, and a letter's cell has PWN_C_PORTAL and no other class bit.
static_assert(PWN_C_RAMPX == (1u << PWN_C_PROT_SHIFT) && PWN_C_RAMPM == (2u << PWN_C_PROT_SHIFT), "the rotation takes the place of RAMPX | RAMPM");
static_assert(pwn_cell_class('A') == PWN_C_PORTAL && pwn_cell_class('M') == PWN_C_PORTAL && pwn_cell_class('Z') == PWN_C_PORTAL, "a letter's cell has no ramp bit");
static_assert((PWN_C_PST_MASK | PWN_C_LT2 | PWN_C_LTDQ) == 0xffu, "the baked byte lies below the class bits");
typedef _Float16 pwn_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pwn_h2 ep_rec(const Lds &L, uint32_t pst_in_place)
{
	return __builtin_bit_cast(pwn_h2, *(const PWN_LDS uint32_t *)(L.eprec + pst_in_place));
}

// HAS_W = false: the camera rows x,y,z carry w = 0 and the position w = 1
// (mat4_iden + rotations, main.c:61-64).  Then every ray has w = +-0 and every
// position w = 1, sphere-relative vectors have w = 0, and each 4-lane dot
// (x+z)+(y+w) of util.h:18-30 equals (x+z)+y bit for bit (a product of zeros
// adds +0; the only sign-of-zero effect is on a dot that is itself +-0, which
// the code only compares with 0 or squares).  The w lanes are dropped.
template<bool HAS_W> struct Vec { float x, y, z, w; };

template<bool W> __device__ __forceinline__ float dot3(const Vec<W> &a, const Vec<W> &b)
{
	if constexpr(W) return (a.x * b.x + a.z * b.z) + (a.y * b.y + a.w * b.w);
	else return (a.x * b.x + a.z * b.z) + a.y * b.y;
}
template<bool W> __device__ __forceinline__ Vec<W> vscale(float s, const Vec<W> &a)
{
	Vec<W> r; r.x = s * a.x; r.y = s * a.y; r.z = s * a.z;
	if constexpr(W) r.w = s * a.w; else r.w = 0.0f;
	return r;
}
template<bool W> __device__ __forceinline__ Vec<W> vadd(const Vec<W> &a, const Vec<W> &b)
{
	Vec<W> r; r.x = a.x + b.x; r.y = a.y + b.y; r.z = a.z + b.z;
	if constexpr(W) r.w = a.w + b.w; else r.w = 0.0f;
	return r;
}
template<bool W> __device__ __forceinline__ Vec<W> vsub(const Vec<W> &a, const Vec<W> &b)
{
	Vec<W> r; r.x = a.x - b.x; r.y = a.y - b.y; r.z = a.z - b.z;
	if constexpr(W) r.w = a.w - b.w; else r.w = 0.0f;
	return r;
}
// util.h:32-46
template<bool W> __device__ __forceinline__ Vec<W> vnormalise(const PWN_LDS uint16_t *rsq, const Vec<W> &a)
{
	return vscale<W>(tab_rsqrt(rsq, dot3<W>(a, a)), a);
}

// lane j of each 16-lane DPP row reads lane j-1; lane 0 reads 0.0f
__device__ __forceinline__ float dpp_row_shr1(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111 /* row_shr:1 */, 0xf, 0xf, true));
}

enum { EV_NONE = 0, EV_WALL, EV_SPHERE, EV_EXHAUSTED };
// BASE_ROOM_Y: the ray left a room through its floor / ceiling (trace.h:323-329,373-379);
// the face and the colour follow from the ray's y sign after the walk
enum { BASE_CEIL = 0, BASE_FLOOR, BASE_WALL, BASE_MAGENTA, BASE_ROOM_Y };

// Regions of the kernel for the issue model (tools/issue_model.py): `//@R name` comments in the sources mark their
// extent, RG(k) counts -- in the counting variants -- how often a wave64 enters one with at least one lane
// (pwn_stats.regions).  The walk's own paths are the older wave_paths counters (WAVE_PATH) and wave_steps.
enum { RG_SEG = 0, RG_SETUP_SLOW, RG_EXHAUSTED, RG_WALL, RG_SPHERE, RG_FLOOR, RG_SPHREFL, RG_JITTER, RG_COMP1, RG_COMP1_FOG,
	RG_COMP2, RG_COMP2_FOG, RG_HELP, RG_UNIT, RG_SPHTEST, RG_SPHUPD, RG_ELSE,
	RG_UNIT_HALF, RG_HC_R2, RG_HC_OUT, RG_PORTAL_WALL, RG_PORTAL_GO, RG_PORTAL_ODD, RG_PORTAL_ROT2,
	RG_SPHBOUND, RG_SPHSKIP,       // a list's ball is tested by the wave (trace_walk.inc, sphere_bound.h); ... and the list skipped
	RG_UNIT_RIGHT,                 // tile pairs: a tile's right half is rebuilt from what its left half put aside (trace_kernel.hip)
	// The units kernel holds the segment's text once per bounce depth (trace_segment.inc): RG_SEG counts the entries of all copies,
	// these the entries of copy 1 and of copy 2 alone (copy 0's are the rest), and the walk iterations of copy 1 and of copy 2 (of
	// pwn_stats.wave_steps, which counts all).  A wave enters copy d + 1 exactly when it ran copy d's jitter: RG_SEG1 and RG_SEG2 are
	// also the per-copy split of RG_JITTER.
	// RG_COMP1 / RG_COMP1_FOG there: the composite with entry A, the first surface (lanes of depth >= 1); RG_COMP2 / RG_COMP2_FOG:
	// with entry B, the second surface (lanes of depth 2), which runs first.  The entry counts are those of the shifted stack's two
	// levels; the FOG counts are per ENTRY now, where they were per stack level (top, below) before.
	RG_SEG1, RG_SEG2, RG_WSTEPS1, RG_WSTEPS2,
	RG_N };
static_assert(RG_N + 1 <= 32, "pwn_stats.regions: the regions, then the waves of the launch");
struct Counters { uint32_t rays, steps, portals, tests, exhausted, wsteps, wp[8], apasses, apass_lanes, rg[RG_N]; };
// one count per wave64 that enters a code path with at least one lane (pwn_stats.wave_paths)
#define WAVE_PATH(k) do { if(COUNT && (__ffsll((long long)__ballot(1)) - 1) == (int)(threadIdx.x & 63)) cnt.wp[k]++; } while(0)
#define RG(k) do { if(COUNT && (__ffsll((long long)__ballot(1)) - 1) == (int)(threadIdx.x & 63)) cnt.rg[k]++; } while(0)

// ---- pieces of the kernels' scheduling code that both write the same way

// screen.h:19-21 (uint32 wrap-around), doubled: the generator runs on the doubled state (lcg2_fs, dev_math.h)
__device__ __forceinline__ uint32_t pixel_seed(int x, int y, int w)
{
	uint32_t seed = (uint32_t)x + (uint32_t)y * (uint32_t)y * ((uint32_t)w + 1u);
	seed *= seed * seed;
	seed *= seed * seed;
	return seed << 1;
}

// the level blob HBM -> LDS by the whole workgroup, 16 B per lane per trip (the caller synchronises)
__device__ __forceinline__ void blob_to_lds(unsigned char *lds, const void *blob, uint32_t blob_bytes)
{
	const uint4 *src = (const uint4 *)blob;
	uint4 *dst = (uint4 *)lds;
	int n16 = (int)(blob_bytes >> 4);
	for(int i = threadIdx.x; i < n16; i += PWN_BLOCK) dst[i] = src[i];
}

// the next open queue after q, cyclically (open: one bit per queue, not 0): bit i of the shifted double mask is queue q+1+i
__device__ __forceinline__ uint32_t next_open_queue(uint32_t q, unsigned long long open)
{
	static_assert(PWN_QUEUES <= 64u && (PWN_QUEUES & (PWN_QUEUES - 1u)) == 0u, "a power of two, one lane per queue");
	if constexpr(PWN_QUEUES == 64u)
	{
		const uint32_t rot = q + 1u;                 // 1..64
		const unsigned long long r = rot == 64u ? open : ((open >> rot) | (open << (64u - rot)));
		return (q + 1u + (uint32_t)__builtin_ctzll(r)) & 63u;
	}
	else
		return (q + 1u + (uint32_t)__builtin_ctzll((open | (open << (PWN_QUEUES & 31u))) >> (q + 1u))) & (PWN_QUEUES - 1u);
}

// PWN_OPT_WAVE_LOG: this wave's two words of the log (pwn_stats.wave_time ..., tools/wave_log.py).
// Which wave of the workgroup this is comes from the hardware: the four waves of a 256-thread workgroup
// sit on the four SIMDs of their CU, HW_ID.simd_id is bits 5:4 of hardware register 4.  (Keeping threadIdx.x
// alive to the end of the kernel costs a scratch slot per lane, and a shared append counter serialises the
// waves' exits and stretches the very tail it measures.)
__device__ __forceinline__ unsigned long long *wave_log_slot(unsigned long long *wave_log)
{
	static_assert(PWN_BLOCK == 256, "one wave per SIMD: simd_id tells the waves of a workgroup apart");
	const unsigned simd = __builtin_amdgcn_s_getreg(4 | (4 << 6) | ((2 - 1) << 11));
	const size_t wid = 1u + (size_t)blockIdx.x * 4u + simd;
	return wave_log + 2 * wid;
}
// lane 0 of the wave without threadIdx.x: the lane number from mbcnt
__device__ __forceinline__ bool wave_first_lane()
{
	return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u;
}

// ---- host side: launching the instantiations of a trace kernel

// One instantiation KERNEL (a __global__ void(pwn_trace_params)) with lds_bytes of dynamic LDS.
template<auto KERNEL>
static hipError_t launch_kernel(const pwn_trace_params *P, int grid, size_t lds_bytes, hipStream_t stream)
{
	// the dynamic-LDS limit is a per-function attribute: raise it only when the blob grew
	// (high-water mark per device and instantiation; contexts of several threads share it, so the
	// check and the raise happen under a lock and the mark only ever grows)
	static size_t lds_mark[64];
	static std::mutex lds_lock;
	int dev = 0;
	(void)hipGetDevice(&dev);
	{
		std::lock_guard<std::mutex> g(lds_lock);
		size_t &lds_set = lds_mark[dev & 63];
		if(lds_bytes > lds_set)
		{
			// the kernel addresses its tables from LDS address 0 (above): that holds while it has no
			// static LDS, which would be laid out in front of the dynamic allocation
			hipFuncAttributes fa;
			hipError_t e = hipFuncGetAttributes(&fa, (const void *)KERNEL);
			if(e != hipSuccess) return e;
			if(fa.sharedSizeBytes != 0) return hipErrorInvalidConfiguration;
			e = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
			if(e != hipSuccess) return e;
			lds_set = lds_bytes;
		}
	}
	hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(PWN_BLOCK), lds_bytes, stream, *P);
	return hipGetLastError();
}

// resident 256-thread workgroups per CU of one instantiation with this much LDS
template<auto KERNEL>
static int kernel_blocks_per_cu(size_t lds_bytes)
{
	int n = 0;
	hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, KERNEL, PWN_BLOCK, lds_bytes);
	if(e != hipSuccess || n < 1) n = 2;
	return n;
}

// The four instantiations of a kernel template for <COUNT, HAS_W> = <1,1>, <1,0>, <0,1>, <0,0>: a launch's
// count and has_w pick one.  (In an unnamed namespace: the library exports the C ABI only.)
namespace {
template<auto K11, auto K10, auto K01, auto K00>
struct TraceKernels
{
	static hipError_t launch(const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t stream)
	{
		if(count) return P->has_w ? launch_kernel<K11>(P, grid, lds_bytes, stream) : launch_kernel<K10>(P, grid, lds_bytes, stream);
		return P->has_w ? launch_kernel<K01>(P, grid, lds_bytes, stream) : launch_kernel<K00>(P, grid, lds_bytes, stream);
	}
	static int blocks_per_cu(size_t lds_bytes, bool count, bool has_w)
	{
		if(count) return has_w ? kernel_blocks_per_cu<K11>(lds_bytes) : kernel_blocks_per_cu<K10>(lds_bytes);
		return has_w ? kernel_blocks_per_cu<K01>(lds_bytes) : kernel_blocks_per_cu<K00>(lds_bytes);
	}
};
}
