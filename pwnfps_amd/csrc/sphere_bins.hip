// sphere_bins.hip -- the sphere tables built on the device (pwn_upload_spheres_device): level_prepare_render's binning
// (level_host.c pwn_bin_spheres) and pwn_i_pack_blob's packing of the lists' device-memory form (tables.h PWN_LF_GLOBAL), from n
// sphere records in device memory, in four launches on the caller's stream:
//   boxes   one thread per sphere: its clamped box as one word (sphere_box.h) and its 32-byte table record; further workgroups copy
//           the level's part of the blob (the base copy) into this copy of the tables
//   count   one wave per cell walks the boxes in object order, 64 at a time, staged through LDS per workgroup: a ballot of "covers
//           this cell" and a popcount give the cell's count -- 4096 x ceil(n / 64) wave iterations, whatever the spheres are
//   scan    one workgroup over the 4096 counts: list starts, the non-empty cells' ordinals, the totals, the longest list, the
//           overflow decision, the status words; liststart and the patched cell words go into the blob unless the tables overflow
//   fill    the count pass again with a lane's rank in the ballot added to a running base: the 16-byte records in object order,
//           the sign of r*r set on a list's last, which[], and the one read-ahead record behind the last
// No sort and no memory atomics: a list's order is the order of the sphere indices, by construction.  Every address is made of a
// cell number, a sphere index below n, and sums of counted values that the scan has held against max_pairs; the sphere records'
// bits reach the box word (four fields clamped to 0 .. 63) and the records' payload, never an address.
//
// Built WITHOUT the denormal flush and with -ffp-contract=off (Makefile): sphere_box.h is the host's arithmetic, which keeps
// denormals; r*r is flushed by its explicit comparison.  Positions, refl and colours are moved as 32-bit words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwn_internal.h"
#include "sphere_box.h"

#define SB_BLOCK 256u                       /* boxes, count, fill: four waves */
#define SB_SCAN_BLOCK 1024u                 /* scan: four cells a thread */
#define SB_BASE_WORDS (PWN_T_BINIDX / 16u)  /* the base copy in 16-byte words */

static_assert(PWN_T_BINIDX % 16u == 0u, "the base copy is moved in 16-byte words");
static_assert(sizeof(pwn_sphere) == 32, "a sphere record is two 16-byte words");
static_assert(PWN_SD_BOX_WORDS >= PWN_OBJ_MAX, "one box word per sphere");

// in: n records r, refl, x, y | z, cb, cg, cr.  out: box[< n]; g_sph[< 2 n] = x, y, z, r*r | refl, cb, cg, cr.
// Workgroups from sph_blocks on: blob[< SB_BASE_WORDS] = base[same].
__global__ void __launch_bounds__(SB_BLOCK)
pwn_sphere_boxes_kernel(const uint4 *__restrict__ in, uint32_t n, uint32_t *__restrict__ box, uint4 *__restrict__ g_sph,
	const uint4 *__restrict__ base, uint4 *__restrict__ blob, uint32_t sph_blocks)
{
	if(blockIdx.x >= sph_blocks)
	{
		const uint32_t i = (blockIdx.x - sph_blocks) * SB_BLOCK + threadIdx.x;
		if(i < SB_BASE_WORDS) blob[i] = base[i];
		return;
	}
	const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
	if(i >= n) return;
	const uint4 a = in[2 * (size_t)i], b = in[2 * (size_t)i + 1];
	const float r = __uint_as_float(a.x);
	box[i] = pwn_box_pack(__uint_as_float(a.z), __uint_as_float(b.x), r);
	g_sph[2 * (size_t)i] = make_uint4(a.z, a.w, b.x, __float_as_uint(pwn_box_r2(r)));
	g_sph[2 * (size_t)i + 1] = make_uint4(a.y, b.y, b.z, b.w);
}

// One wave per cell, cell = 4 * workgroup + wave.  FILL = false: count[cell] = the spheres whose box covers the cell.
// FILL = true (behind the scan): nothing at all when status[PWN_SD_ST_REASON] != 0; else the cell's records g_rec[start[cell] ..
// + count[cell]) and which[] of the same indices, in sphere order, and g_rec[pairs] = 0 by cell 0.
template<bool FILL>
__global__ void __launch_bounds__(SB_BLOCK)
pwn_sphere_lists_kernel(const uint32_t *__restrict__ box, uint32_t n, uint32_t *__restrict__ count, const uint32_t *__restrict__ start,
	const uint32_t *__restrict__ status, const uint4 *__restrict__ g_sph, uint4 *__restrict__ g_rec, uint32_t *__restrict__ g_which)
{
	__shared__ uint32_t sbox[SB_BLOCK];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t cell = blockIdx.x * 4u + wave, cx = cell & 63u, cz = cell >> 6;
	uint32_t run = 0u, last = 0u;
	if(FILL)
	{
		if(status[PWN_SD_ST_REASON] != 0u) return;        // (the same word for every thread of the launch)
		run = start[cell];
		last = run + count[cell];                         // one past the cell's last record
		if(cell == 0u && lane == 0u) g_rec[status[PWN_SD_ST_PAIRS]] = make_uint4(0u, 0u, 0u, 0u);
	}
	for(uint32_t at = 0u; at < n; at += SB_BLOCK)
	{
		sbox[threadIdx.x] = at + threadIdx.x < n ? box[at + threadIdx.x] : PWN_BOX_EMPTY;
		__syncthreads();
		for(uint32_t sub = 0u; sub < SB_BLOCK && at + sub < n; sub += 64u)
		{
			const bool cov = pwn_box_covers(sbox[sub + lane], cx, cz) != 0;
			const unsigned long long m = __ballot(cov);
			if(FILL)
			{
				const uint32_t k = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
				if(cov && k < last)
				{
					const uint32_t i = at + sub + lane;
					uint4 rec = g_sph[2 * (size_t)i];
					if(k + 1u == last) rec.w |= 0x80000000u;
					g_rec[k] = rec;
					g_which[k] = i;
				}
			}
			run += (uint32_t)__popcll(m);
		}
		__syncthreads();
	}
	if(!FILL && lane == 0u) count[cell] = run;
}

// One workgroup.  In: count[4096], max_pairs.  Out: start[4096] (the exclusive sums), status[]; unless the tables overflow,
// liststart[ordinal] = start for the non-empty cells and their cell words |= PWN_C_SPH | ordinal << 16 in the blob (which holds
// the base copy: the boxes launch, in front of this one on the stream).
__global__ void __launch_bounds__(SB_SCAN_BLOCK)
pwn_sphere_scan_kernel(const uint32_t *__restrict__ count, uint32_t *__restrict__ start, uint32_t *__restrict__ status,
	uint32_t *__restrict__ blob, uint32_t n, uint32_t max_pairs)
{
	__shared__ uint32_t s_sum[SB_SCAN_BLOCK], s_nz[SB_SCAN_BLOCK], s_max[SB_SCAN_BLOCK];
	const uint32_t t = threadIdx.x;
	const uint4 c4 = ((const uint4 *)count)[t];
	const uint32_t c[4] = { c4.x, c4.y, c4.z, c4.w };
	uint32_t sum = 0u, nz = 0u, mx = 0u;
	for(int i = 0; i < 4; i++) { sum += c[i]; nz += c[i] != 0u; mx = c[i] > mx ? c[i] : mx; }
	s_sum[t] = sum; s_nz[t] = nz; s_max[t] = mx;
	__syncthreads();
	// inclusive sums (and the running maximum) over the 1024 threads, ten doubling steps
	for(uint32_t d = 1u; d < SB_SCAN_BLOCK; d <<= 1)
	{
		uint32_t a = 0u, b = 0u, m = 0u;
		if(t >= d) { a = s_sum[t - d]; b = s_nz[t - d]; m = s_max[t - d]; }
		__syncthreads();
		s_sum[t] += a; s_nz[t] += b; s_max[t] = m > s_max[t] ? m : s_max[t];
		__syncthreads();
	}
	const uint32_t pairs = s_sum[SB_SCAN_BLOCK - 1u], ncell = s_nz[SB_SCAN_BLOCK - 1u], longest = s_max[SB_SCAN_BLOCK - 1u];
	const uint32_t reason = pairs > max_pairs ? 1u : (longest > (uint32_t)PWN_LIST_MAX ? 2u : 0u);
	if(t == 0u)
	{
		status[PWN_SD_ST_PAIRS] = pairs; status[PWN_SD_ST_NCELL] = ncell; status[PWN_SD_ST_LONGEST] = longest; status[PWN_SD_ST_REASON] = reason;
		status[PWN_SD_ST_N] = n; status[PWN_SD_ST_MAX_PAIRS] = max_pairs;
	}
	uint32_t at = s_sum[t] - sum, ord = s_nz[t] - nz;
	uint32_t *liststart = blob + PWN_T_BINIDX / 4u, *cells = blob + PWN_T_CELLINFO / 4u;
	for(int i = 0; i < 4; i++)
	{
		const uint32_t cell = 4u * t + (uint32_t)i;
		start[cell] = at;
		if(reason == 0u && c[i] != 0u)
		{
			// (ord < ncell <= min(4096, pairs) <= min(4096, max_pairs): inside the LDS part the host laid out)
			liststart[ord] = at;
			cells[(cell >> 6) * PWN_GRID_PITCH + (cell & 63u)] |= PWN_C_SPH | (ord << 16);
			ord++;
		}
		at += c[i];
	}
}

// The four launches.  d_spheres: n records, 16-byte aligned (n == 0: not read).  d_scratch: PWN_SD_SCRATCH_BYTES of the context's.
// d_base: PWN_T_BINIDX bytes.  d_blob: room for pwn_t_total_glb(min(4096, max_pairs)).  d_big: room for pwn_g_total(max_pairs, n),
// sections at which_off and sph_off.
extern "C" hipError_t pwn_launch_sphere_bins(const void *d_spheres, uint32_t n, uint32_t max_pairs, void *d_scratch, const void *d_base,
	void *d_blob, void *d_big, uint64_t which_off, uint64_t sph_off, hipStream_t stream)
{
	uint32_t *box = (uint32_t *)d_scratch, *count = box + PWN_SD_BOX_WORDS, *start = count + 4096, *status = start + 4096;
	uint4 *g_rec = (uint4 *)d_big, *g_sph = (uint4 *)((uint8_t *)d_big + sph_off);
	uint32_t *g_which = (uint32_t *)((uint8_t *)d_big + which_off);
	const uint32_t sph_blocks = (n + SB_BLOCK - 1u) / SB_BLOCK, base_blocks = (SB_BASE_WORDS + SB_BLOCK - 1u) / SB_BLOCK;
	hipLaunchKernelGGL(pwn_sphere_boxes_kernel, dim3(sph_blocks + base_blocks), dim3(SB_BLOCK), 0, stream, (const uint4 *)d_spheres, n, box, g_sph,
		(const uint4 *)d_base, (uint4 *)d_blob, sph_blocks);
	hipLaunchKernelGGL(pwn_sphere_lists_kernel<false>, dim3(1024), dim3(SB_BLOCK), 0, stream, (const uint32_t *)box, n, count, (const uint32_t *)start,
		(const uint32_t *)status, (const uint4 *)g_sph, g_rec, g_which);
	hipLaunchKernelGGL(pwn_sphere_scan_kernel, dim3(1), dim3(SB_SCAN_BLOCK), 0, stream, (const uint32_t *)count, start, status, (uint32_t *)d_blob, n, max_pairs);
	hipLaunchKernelGGL(pwn_sphere_lists_kernel<true>, dim3(1024), dim3(SB_BLOCK), 0, stream, (const uint32_t *)box, n, count, (const uint32_t *)start,
		(const uint32_t *)status, (const uint4 *)g_sph, g_rec, g_which);
	return hipGetLastError();
}
