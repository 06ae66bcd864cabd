// level_bake.hip -- a level's part of the tables made on the device (pwn_upload_level_device): what pwn_parse_level derives,
// pwn_check_portals decides and pwn_bake_cells bakes on the host (level_host.c), from a grid of 4096 cell bytes and, where given, a
// portal table in device memory.  The rules themselves are level_bake.h's, shared with a CPU program.
//
// ONE launch of ONE workgroup of 1024 threads (sixteen waves): the whole level is 4 KB of cells and 728 bytes of table, it fits LDS
// many times over, and the three steps need each other's whole result -- separate launches would only put the same bytes through
// device memory twice more.  Wave w owns the 64-cell chunks 4w .. 4w + 3, a lane one cell of each, so a chunk is a row of the grid
// and a ballot over it is that row's mask.
//   table    (d_pmap NULL) the first and second sighting of each letter: LDS atomicMin on the cell number, twice -- the second pass
//            skips the cell the first found.  At most two ds_min per thread and pass against 26 ballots per chunk for the other form;
//            then 26 lanes derive rot12, c1, c2 (level_bake.h pwn_lb_derive_letter).  Given a table, 182 lanes copy it as it is.
//   verdict  26 lanes hold their letter's four coordinates against -1 .. 63, 130 lanes the cells at (-1, t) and (t, -1) against
//            the rule for cells outside the grid; the lowest offending letter of either rule by LDS atomicMin.  A coordinate out of
//            range decides before the other rule is looked at.
//   bake     only on verdict 0 -- differences of coordinates and their half floats are formed behind the range check, never in
//            front of it.  A chunk's endpoint cells by ballot; 64 lanes sum the 64 masks' popcounts in front of each chunk; a cell's
//            record number is that sum plus the lanes below it in its own mask: the rank in scan order, at most 51.
//   commit   verdict 0: the 65 x 65 cell words and the 52 records into the base copy, the walk table (cells, the table as given or
//            derived, padding 0) into the buffer chosen for it.  Any other verdict: the base copy is not touched and the previous
//            walk buffer is copied into the chosen one.  The status words either way.
// Every address is made of a thread number, a cell number below 4096 or a rank held below PWN_EP_MAX; the grid's bytes and the
// table's words are compared, or'ed into words and copied, and the derived table's coordinates are cell numbers the kernel counted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwn_internal.h"
#include "level_bake.h"

#define LB_BLOCK 1024u
#define LB_PM_WORDS (26u * PWN_LB_PM_WORDS)
#define LB_WALK_WORDS (PWN_WALK_BYTES / 4u)

static_assert(sizeof(pwn_walk_table) == PWN_WALK_BYTES && PWN_WALK_BYTES % 16u == 0u, "the walk table is moved in words");
static_assert(LB_PM_WORDS + 1024u + 2u == LB_WALK_WORDS, "cells, table, two words of padding");
static_assert(LB_BLOCK * 4u == 4096u, "a thread has four cells");

__global__ void __launch_bounds__(LB_BLOCK)
pwn_level_bake_kernel(const uint32_t *__restrict__ d_cells, const int32_t *__restrict__ d_pmap, uint32_t *__restrict__ base,
	uint32_t *__restrict__ walk, const uint32_t *__restrict__ walk_prev, uint32_t *__restrict__ status, uint32_t prev_dev)
{
	__shared__ uint32_t s_cellw[1024];                     // the grid, as words
	__shared__ int32_t s_pmap[LB_PM_WORDS];
	__shared__ uint32_t s_first[26], s_second[26];
	__shared__ uint32_t s_bad[2];                          // the lowest offending letter of rule 1, of rule 2 (26: none)
	__shared__ unsigned long long s_mask[64];              // per chunk: its endpoint cells
	__shared__ uint32_t s_before[64 + 1];                  // endpoint cells in front of a chunk; [64] = all of them
	__shared__ uint32_t s_recs[PWN_EP_MAX];
	const uint8_t *s_cells = (const uint8_t *)s_cellw;
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const bool derived = d_pmap == NULL;

	s_cellw[t] = d_cells[t];
	if(t < 26u) { s_first[t] = 0xffffffffu; s_second[t] = 0xffffffffu; }
	if(t < 2u) s_bad[t] = 26u;
	if(t < PWN_EP_MAX) s_recs[t] = 0u;
	if(!derived && t < LB_PM_WORDS) s_pmap[t] = d_pmap[t];
	__syncthreads();

	// ---- table
	if(derived)
	{
		for(uint32_t k = 0u; k < 4u; k++)
		{
			const uint32_t cell = (wave * 4u + k) * 64u + lane, c = s_cells[cell];
			if(c >= 'A' && c <= 'Z') atomicMin(&s_first[c - 'A'], cell);
		}
		__syncthreads();
		for(uint32_t k = 0u; k < 4u; k++)
		{
			const uint32_t cell = (wave * 4u + k) * 64u + lane, c = s_cells[cell];
			if(c >= 'A' && c <= 'Z' && s_first[c - 'A'] != cell) atomicMin(&s_second[c - 'A'], cell);
		}
		__syncthreads();
		if(t < 26u) pwn_lb_derive_letter(s_cells, s_first[t], s_second[t], &s_pmap[PWN_LB_PM_WORDS * t]);
		__syncthreads();
	}

	// ---- verdict
	if(t < 26u) { if(pwn_lb_coords_bad(&s_pmap[PWN_LB_PM_WORDS * t])) atomicMin(&s_bad[0], t); }
	else if(t >= 64u && t < 64u + 130u)
	{
		const int letter = pwn_lb_outside_letter_nth(s_cells, s_pmap, (int)(t - 64u));
		if(letter >= 0) atomicMin(&s_bad[1], (uint32_t)letter);
	}
	__syncthreads();
	const uint32_t verdict = s_bad[0] < 26u ? (uint32_t)PWN_LB_BAD_COORD : (s_bad[1] < 26u ? (uint32_t)PWN_LB_BAD_OUTSIDE : (uint32_t)PWN_LB_TAKEN);

	if(verdict != PWN_LB_TAKEN)
	{
		// the level in force stays: its walk table into the buffer this copy of the tables will refer to
		for(uint32_t i = t; i < LB_WALK_WORDS; i += LB_BLOCK) walk[i] = walk_prev[i];
		if(t == 0u)
		{
			const uint32_t dev = prev_dev ? status[7] : 0u;
			status[0] = verdict; status[1] = verdict == PWN_LB_BAD_COORD ? s_bad[0] : s_bad[1];
			status[2] = 0u; status[3] = 0u; status[4] = derived ? 1u : 0u; status[5] = 0u; status[6] = 0u; status[7] = dev;
		}
		return;
	}

	// ---- bake
	for(uint32_t k = 0u; k < 4u; k++)
	{
		const uint32_t chunk = wave * 4u + k, cell = chunk * 64u + lane;
		const unsigned long long m = __ballot(pwn_lb_is_endpoint(s_cells[cell], (int)lane, (int)chunk, s_pmap) != 0);
		if(lane == 0u) s_mask[chunk] = m;
	}
	__syncthreads();
	if(t <= 64u)
	{
		uint32_t sum = 0u;
		for(uint32_t j = 0u; j < t; j++) sum += (uint32_t)__popcll(s_mask[j]);
		s_before[t] = sum;
	}
	__syncthreads();
	uint32_t *words = base + PWN_T_CELLINFO / 4u;
	for(uint32_t k = 0u; k < 4u; k++)
	{
		const uint32_t chunk = wave * 4u + k, cell = chunk * 64u + lane, c = s_cells[cell];
		const unsigned long long m = s_mask[chunk];
		const uint32_t rank = s_before[chunk] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
		uint32_t inside, outside, rec = 0u;
		const int has = pwn_lb_cell_bits((int)c, (int)lane, (int)chunk, s_pmap, rank, &inside, &outside, &rec);
		if(has && rank < PWN_EP_MAX) s_recs[rank] = rec;
		const uint32_t cls = pwn_cell_class(c);
		words[chunk * PWN_GRID_PITCH + lane] = cls | inside;
		// what get_cell returns outside the grid on that axis (util.h:151-158): never at an endpoint, never with spheres
		if(lane == 0u) words[chunk * PWN_GRID_PITCH + 64u] = cls | outside;
		if(chunk == 0u) words[64u * PWN_GRID_PITCH + lane] = cls | outside;
		if(cell == 0u) words[64u * PWN_GRID_PITCH + 64u] = cls | outside;
	}
	__syncthreads();

	// ---- commit: the records, the walk table, the status words
	if(t < PWN_EP_MAX) base[PWN_T_EPREC / 4u + t] = s_recs[t];
	walk[t] = s_cellw[t];
	if(t < LB_PM_WORDS) walk[1024u + t] = (uint32_t)s_pmap[t];
	if(t < 2u) walk[1024u + LB_PM_WORDS + t] = 0u;
	if(t == 0u)
	{
		uint32_t paired = 0u;
		for(uint32_t i = 0u; i < 26u; i++) paired += s_pmap[PWN_LB_PM_WORDS * i + PWN_LB_X1] != -1 && s_pmap[PWN_LB_PM_WORDS * i + PWN_LB_X2] != -1;
		status[0] = PWN_LB_TAKEN; status[1] = 26u; status[2] = s_before[64]; status[3] = paired; status[4] = derived ? 1u : 0u;
		status[5] = 0u; status[6] = 0u; status[7] = 1u;
	}
}

// d_data: 4096 bytes, d_pmap: 26 x 7 int32 or NULL, both 16-byte aligned.  d_base: the base copy, PWN_T_BINIDX bytes.  d_walk: the
// walk buffer chosen, d_walk_prev: the one of the tables in force (another buffer).  d_status: PWN_LD_STATUS_WORDS words; word 7
// carries "a device-built level is in force" from build to build, and is read only where prev_dev says the build before this one left it.
extern "C" hipError_t pwn_launch_level_bake(const void *d_data, const void *d_pmap, void *d_base, pwn_walk_table *d_walk,
	const pwn_walk_table *d_walk_prev, uint32_t *d_status, int prev_dev, hipStream_t stream)
{
	hipLaunchKernelGGL(pwn_level_bake_kernel, dim3(1), dim3(LB_BLOCK), 0, stream, (const uint32_t *)d_data, (const int32_t *)d_pmap,
		(uint32_t *)d_base, (uint32_t *)d_walk, (const uint32_t *)d_walk_prev, d_status, (uint32_t)(prev_dev != 0));
	return hipGetLastError();
}
