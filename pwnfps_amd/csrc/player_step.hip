// player_step.hip -- the motion of the reference's loop (main.c:188-379) for a batch of players on the device
// (pwn_players_step / pwn_players_step_device): host/player.c's pwn_player_step, one thread per player, the state in registers
// across the ticks of a call.
//
// Built like view_setup.hip, with -fno-gpu-flush-denormals-to-zero and -ffp-contract=off (csrc/Makefile): host/player.c is
// plain C that keeps denormals and rounds every product and sum by itself, and every float here has to be its float.
// The walk reads the raw cell characters and the portal table (pwn_walk_table, tables.h), which the baked cell words of the
// trace kernels do not hold.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_math.h"
#include "pwn_internal.h"

static_assert(sizeof(pwn_walk_table) == PWN_WALK_BYTES, "the walk table is 4096 cell bytes, 26 portals of 7 int32, padded to 16");
static_assert(sizeof(pwn_portal) == 28, "a portal is seven int32");

#define PLAYER_BBOX 0.2f          /* defs.h:6 */

// util.h:151-158: the clamp is on the integers, after the conversion -- whatever the float was, the index is inside the table
template<class CP> __device__ __forceinline__ int cell_at(CP cells, int cx, int cz)
{
	if(cx < 0 || cx >= 64) cx = 0;
	if(cz < 0 || cz >= 64) cz = 0;
	return cells[cz * 64 + cx];
}

// util.h:112-126: can a player at height y NOT stand in a cell of type c, coming from oldcell.  The reference's chain of tests, as
// selects: a wave's players stand before different kinds of cell, and five inlined copies of the chain as branches made a tick
// 1500 instructions that every wave walked through (profiles/players/step.txt).  Rooms and ramps are solid outside [lo, hi); a
// letter where it has no second endpoint; everything else always.  The portal index is c - 'A' of a byte that was tested to be
// a letter (any other cell reads letter A's word and does not use it).
// (The kinds of cell as bit masks over the characters 32 .. 63 -- all of them but '^' lie there -- because a chain of == on one
// byte is a switch to the compiler, and comes back as the branches it was written to avoid.)
#define CELL_BIT(ch) (1u << ((ch) - 32))
__device__ __forceinline__ bool cell_in(unsigned mask, int c)
{
	const unsigned d = (unsigned)c - 32u;
	return ((mask >> (d & 31u)) & (d < 32u ? 1u : 0u)) != 0u;
}
template<class PP> __device__ __forceinline__ bool is_solid(PP pmap, int c, int oldcell, float y)
{
	const unsigned TWO = CELL_BIT('#') | CELL_BIT('&');
	const unsigned LOW = CELL_BIT(';') | CELL_BIT('$') | CELL_BIT('"') | CELL_BIT('>') | CELL_BIT('<') | CELL_BIT(',');
	const bool two = cell_in(TWO, c);
	const bool dq_from_two = (c == '"') & cell_in(TWO, oldcell);
	const bool low = cell_in(LOW, c) | (c == '^');
	const bool letter = (unsigned)(c - 'A') <= (unsigned)('Z' - 'A');
	const float lo = dq_from_two ? 1.0f : 0.0f, hi = (two | dq_from_two) ? 2.0f : 1.0f;
	const bool by_height = (y < lo) | (y >= hi);
	const bool unpaired = pmap[(letter ? c - 'A' : 0) * 7 + 2] == -1;
	return (two | low) ? by_height : (letter ? unpaired : true);
}

// (int differences of cells that may be anything outside the domain: wrapped, never undefined)
__device__ __forceinline__ int isub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int iadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// One pwn_player_step (host/player.c) behind the turn: rx / rz are the camera's rows x and z, pos its row w.  vs / vc are
// sinf / cosf of the tick's angle, the same in every tick of a call.
template<class CP, class PP> __device__ __forceinline__ void player_tick(float4 &rx, float4 &rz, float4 &pos, float4 &grav, int &traversals,
	CP cells, PP pmap, float vs, float vc, float fwd, float side, float gdrop)
{
	// util.h:91-110
	{
		const float vxx = rx.x, vxz = rx.z, vzx = rz.x, vzz = rz.z;
		rx.x = vc * vxx + vs * vxz;
		rx.z = vc * vxz - vs * vxx;
		rz.x = vc * vzx + vs * vzz;
		rz.z = vc * vzz - vs * vzx;
	}

	// main.c:195-210: old cell, velocity along the forward and right rows, move
	const int cx1 = (int)pos.x, cz1 = (int)pos.z;
	const float velx = rz.x * fwd + rx.x * side, vely = rz.y * fwd + rx.y * side;
	const float velz = rz.z * fwd + rx.z * side, velw = rz.w * fwd + rx.w * side;
	pos.x += velx; pos.y += vely; pos.z += velz; pos.w += velw;

	// main.c:212-266: push back out of solid cells, by the corner of the bounding box that leads
	const float px1 = pos.x, py1 = pos.y, pz1 = pos.z;
	const int gx1 = velx < 0.0f ? -1 : 1, gz1 = velz < 0.0f ? -1 : 1;
	const int bcx = (int)(px1 + (float)gx1 * PLAYER_BBOX), bcz = (int)(pz1 + (float)gz1 * PLAYER_BBOX);
	const int oldcell = cell_at(cells, cx1, cz1);
	const float backx = (float)cx1 + 0.5f + (0.5f - PLAYER_BBOX) * (float)gx1;
	const float backz = (float)cz1 + 0.5f + (0.5f - PLAYER_BBOX) * (float)gz1;
	// The three arms of main.c:212-266 in one: off the diagonal the one cell looked at, (bcx, bcz), IS the x arm's (bcz == cz1) or the
	// z arm's (bcx == cx1) neighbour; on it, x is pushed when its neighbour is solid, z when its neighbour is, or -- with x free --
	// when the corner is.  No arm for a wave to take in turns.
	{
		const bool dx = cx1 != bcx, dz = cz1 != bcz;
		const bool solx = is_solid(pmap, cell_at(cells, bcx, cz1), oldcell, py1);
		const bool solz = is_solid(pmap, cell_at(cells, cx1, bcz), oldcell, py1);
		const bool solc = is_solid(pmap, cell_at(cells, bcx, bcz), oldcell, py1);
		if(dx & solx) pos.x = backx;
		if(dz & (solz | (dx & !solx & solc))) pos.z = backz;
	}

	// main.c:268-276: gravity
	pos.x += grav.x; pos.y += grav.y; pos.z += grav.z; pos.w += grav.w;
	grav.y -= gdrop;
	if(pos.y < 0.4f) { pos.y = 0.4f; grav.y = 0.0f; }

	// main.c:278-378: a new cell: steps of a two-high room, portals
	const int cx2 = (int)pos.x, cz2 = (int)pos.z;
	if(cx1 == cx2 && cz1 == cz2) return;
	const int c1 = oldcell, c2 = cell_at(cells, cx2, cz2);
	if((c1 == '#' || c1 == '&') && c2 == '"') pos.y -= 1.0f;
	else if(c1 == '"' && (c2 == '#' || c2 == '&')) pos.y += 1.0f;
	else if(c2 >= 'A' && c2 <= 'Z')
	{
		const int pi = (c2 - 'A') * 7;
		const int px1_ = pmap[pi + 0], pz1_ = pmap[pi + 1], px2_ = pmap[pi + 2], pz2_ = pmap[pi + 3], rot12 = pmap[pi + 4];
		traversals++;
		int rot = 0;
		float qx = pos.x, qz = pos.z, rcx = (float)cx2, rcz = (float)cz2;
		float rvxx = rx.x, rvxz = rx.z, rvzx = rz.x, rvzz = rz.z;
		if(px2_ == -1) { /* an unpaired letter: nothing happens (main.c:308-310) */ }
		else if(px1_ == cx2 && pz1_ == cz2)
		{
			qx += (float)iadd(isub(cx2, cx1), isub(px2_, px1_));
			qz += (float)iadd(isub(cz2, cz1), isub(pz2_, pz1_));
			rcx = (float)px2_; rcz = (float)pz2_;
			rot = (-rot12) & 3;
		}
		else if(px2_ == cx2 && pz2_ == cz2)
		{
			qx += (float)isub(isub(cx2, cx1), isub(px2_, px1_));
			qz += (float)isub(isub(cz2, cz1), isub(pz2_, pz1_));
			rcx = (float)px1_; rcz = (float)pz1_;
			rot = rot12 & 3;
		}
		const float trx = qx, trz = qz, trvxx = rvxx, trvxz = rvxz, trvzx = rvzx, trvzz = rvzz;
		switch(rot)
		{
			case 1:
				qx = (rcx + 0.5f) + (trz - (rcz + 0.5f));
				qz = (rcz + 0.5f) - (trx - (rcx + 0.5f));
				rvxx = trvxz; rvxz = -trvxx; rvzx = trvzz; rvzz = -trvzx;
				break;
			case 2:
				qx = (rcx + 0.5f) * 2.0f - qx;
				qz = (rcz + 0.5f) * 2.0f - qz;
				rvxx = -trvxx; rvxz = -trvxz; rvzx = -trvzx; rvzz = -trvzz;
				break;
			case 3:
				qx = (rcx + 0.5f) - (trz - (rcz + 0.5f));
				qz = (rcz + 0.5f) + (trx - (rcx + 0.5f));
				rvxx = -trvxz; rvxz = trvxx; rvzx = -trvzz; rvzz = trvzx;
				break;
			default: break;
		}
		pos.x = qx; pos.z = qz;
		rx.x = rvxx; rx.z = rvxz; rz.x = rvzx; rz.z = rvzz;
	}
}

// One thread per player.  cams: n x 4 float4 (rows x, y, z, w; row y is neither read nor written), gravity: n float4,
// traversals: n int32 or NULL, keys: n bytes (bit i = PWN_MOVE_* i).  STAGE: the workgroup copies the walk table into LDS first --
// what every call does; the other instantiation is the comparison's other arm (PWN_PLAYERS_STAGE=0; profiles/players/step.txt).
template<bool STAGE> __global__ void __launch_bounds__(64)
pwn_players_step_kernel(float4 *__restrict__ cams, float4 *__restrict__ gravity, int32_t *__restrict__ traversals,
	const uint8_t *__restrict__ keys, int n, float tdiff, int ticks, const pwn_walk_table *__restrict__ walk)
{
	__shared__ uint4 sh[STAGE ? PWN_WALK_BYTES / 16 : 1];
	if(STAGE)
	{
		const uint4 *src = (const uint4 *)walk;
		for(int k = threadIdx.x; k < PWN_WALK_BYTES / 16; k += 64) sh[k] = src[k];
		__syncthreads();
	}
	const int i = blockIdx.x * 64 + threadIdx.x;
	if(i >= n) return;
	const unsigned k = keys[i];
	float4 rx = cams[4 * (size_t)i + 0], rz = cams[4 * (size_t)i + 2], pos = cams[4 * (size_t)i + 3];
	float4 grav = gravity[i];
	int trav = traversals != NULL ? traversals[i] : 0;

	// what a tick takes from the keys and tdiff is the same in every tick (main.c:188, :197-198, :270)
	const float ang = tdiff * 3.0f * (float)((int)(k & 1u) - (int)((k >> 1) & 1u));
	const float fwd = tdiff * 5.0f * (float)((int)((k >> 4) & 1u) - (int)((k >> 5) & 1u));
	const float side = tdiff * 5.0f * (float)((int)((k >> 6) & 1u) - (int)((k >> 7) & 1u));
	const float gdrop = 3.0f * tdiff * tdiff;
	const float2 sc = glibc_sincosf_both(ang);        // x = sinf, y = cosf

	if(STAGE)
	{
		const uint8_t *cells = (const uint8_t *)sh;
		const int32_t *pmap = (const int32_t *)((const uint8_t *)sh + 4096);
		for(int t = 0; t < ticks; t++) player_tick(rx, rz, pos, grav, trav, cells, pmap, sc.x, sc.y, fwd, side, gdrop);
	}
	else
	{
		const uint8_t *cells = walk->cells;
		const int32_t *pmap = walk->pmap;
		for(int t = 0; t < ticks; t++) player_tick(rx, rz, pos, grav, trav, cells, pmap, sc.x, sc.y, fwd, side, gdrop);
	}

	cams[4 * (size_t)i + 0] = rx; cams[4 * (size_t)i + 2] = rz; cams[4 * (size_t)i + 3] = pos;
	gravity[i] = grav;
	if(traversals != NULL) traversals[i] = trav;
}

// d_cams and d_gravity 16-byte aligned, d_traversals 4-byte aligned or NULL; stage: 1 = through LDS, 0 = from device memory
extern "C" hipError_t pwn_launch_players_step(float *d_cams, float *d_gravity, int32_t *d_traversals, const uint8_t *d_keys, int n,
	float tdiff, int ticks, const pwn_walk_table *d_walk, int stage, hipStream_t stream)
{
	if(n <= 0) return hipSuccess;
	const dim3 grid((unsigned)((n + 63) / 64)), block(64);
	if(stage)
		hipLaunchKernelGGL(pwn_players_step_kernel<true>, grid, block, 0, stream, (float4 *)d_cams, (float4 *)d_gravity, d_traversals, d_keys, n, tdiff, ticks, d_walk);
	else
		hipLaunchKernelGGL(pwn_players_step_kernel<false>, grid, block, 0, stream, (float4 *)d_cams, (float4 *)d_gravity, d_traversals, d_keys, n, tdiff, ticks, d_walk);
	return hipGetLastError();
}
