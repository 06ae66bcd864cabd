// pixel_rays.hip -- the second half of pwn_pixel_rays on the device (pwn_pixel_rays_device): from the view records that the camera
// set-up (view_setup.hip) wrote, the ray record and the seed of chosen pixels, one thread per ray.
//
// Built by the Makefile's general rule: WITH the denormal flush and -ffp-contract=off.  The host runs this half under FTZ|DAZ
// (pwn_launch.cpp pwn_pixel_rays), as the trace kernels run their add chain, and rounds every product and sum by itself; the half
// that keeps denormals is the set-up kernel's, in its own file for that reason.  The origin is never computed with: it is moved
// as four 32-bit words, so a denormal there stays what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwn_internal.h"

static_assert(sizeof(pwn_view_rec) == PWN_PIXEL_WORK_BYTES, "a camera's scratch is its view record");

#define PIXEL_RAYS_BLOCK 256

// n / d by launch_plan.h's pwn_unit_div_magic (exact below 2^31; shift < 0: d == 1)
__device__ __forceinline__ uint32_t div_magic(uint32_t n, uint32_t magic, int shift)
{
	return shift >= 0 ? __umulhi(n, magic) >> shift : n;
}

// Ray i * m + j is camera i's pixel j.  xy: the pixels, m of them (shared != 0) or total of them, camera-major; NULL = the whole
// frame, pixel j at (j % width, j / width).  seeds: NULL = none written.
// The last workgroup's surplus threads compute the last ray again and store nothing, so that the test for a wave of one camera sees
// every lane: what is read is recs[< n], xy[< m or < total]; what is written is rays[< 2 total], seeds[< total].
// Each lane stores its own record's two 16-byte halves, one behind the other: a wave's two stores fill 2 KiB of consecutive bytes
// between them.  Passing the records through LDS first, so that each store instruction alone covers 1 KiB of consecutive bytes, measured
// the same (profiles/pixel_rays/bench.txt), and is not done.
__global__ void __launch_bounds__(PIXEL_RAYS_BLOCK)
pwn_pixel_rays_kernel(const float4 *__restrict__ recs, const int2 *__restrict__ xy, uint4 *__restrict__ rays, uint32_t *__restrict__ seeds,
	uint32_t total, uint32_t m, uint32_t m_magic, int m_shift, int shared, uint32_t width, uint32_t w_magic, int w_shift)
{
	const uint32_t idx = blockIdx.x * PIXEL_RAYS_BLOCK + threadIdx.x;
	const bool live = idx < total;
	const uint32_t i = live ? idx : total - 1u;
	const uint32_t cam = div_magic(i, m_magic, m_shift), j = i - cam * m;

	// the camera's record: where the wave's rays are all of one camera (always, once m is a multiple of 64; mostly, once it is
	// large) scalar loads of its 64 bytes serve the wave, otherwise every lane reads its own
	float4 rayb, rdx, rdy; uint4 from;
	const uint32_t cam0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cam);
	if(__all(cam == cam0))
	{
		typedef const __attribute__((address_space(4))) float cfloat;
		typedef const __attribute__((address_space(4))) uint32_t cu32;
		const cfloat *r = (const cfloat *)((uintptr_t)recs + (uintptr_t)cam0 * PWN_PIXEL_WORK_BYTES);
		const cu32 *ru = (const cu32 *)r;
		rayb = make_float4(r[0], r[1], r[2], r[3]);
		rdx = make_float4(r[4], r[5], r[6], r[7]);
		rdy = make_float4(r[8], r[9], r[10], r[11]);
		from = make_uint4(ru[12], ru[13], ru[14], ru[15]);
	}
	else
	{
		const float4 *r = recs + 5 * (size_t)cam;
		rayb = r[0]; rdx = r[1]; rdy = r[2];
		from = *(const uint4 *)(r + 3);
	}

	int x, y;
	if(xy != NULL)
	{
		const int2 p = xy[shared ? j : i];
		x = p.x; y = p.y;
	}
	else
	{
		const uint32_t row = div_magic(j, w_magic, w_shift);
		x = (int)(j - row * width); y = (int)row;
	}

	// screen.h:12-18 in the reference build's order, as pwn_pixel_rays and the trace kernel's unit loop: rayl = (cx0 * rdx + rayb)
	// + y * rdy, then one "+= rdx" per pixel of the 32-wide tile up to and including this one -- (x & 31) + 1 of them, whatever x is
	const int cx0 = x & ~31;
	const float fx = (float)cx0, fy = (float)y;
	float4 v;
	v.x = (fx * rdx.x + rayb.x) + fy * rdy.x;
	v.y = (fx * rdx.y + rayb.y) + fy * rdy.y;
	v.z = (fx * rdx.z + rayb.z) + fy * rdy.z;
	v.w = (fx * rdx.w + rayb.w) + fy * rdy.w;
	const int adds = (x & 31) + 1;
	for(int k = 0; k < adds; k++) { v.x += rdx.x; v.y += rdx.y; v.z += rdx.z; v.w += rdx.w; }
	const uint4 dir = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));

	if(!live) return;
	rays[2 * (size_t)idx] = from; rays[2 * (size_t)idx + 1] = dir;
	if(seeds != NULL)
	{
		// screen.h:19-21 (uint32 wrap-around), not doubled: what pwn_pixel_rays hands out and pwn_trace_rays takes
		uint32_t sd = (uint32_t)x + (uint32_t)y * (uint32_t)y * (width + 1u);
		sd *= sd * sd;
		sd *= sd * sd;
		seeds[idx] = sd;
	}
}

// d_recs and d_rays 16-byte aligned, d_xy 8-byte aligned or NULL (the whole frame: m == width * height), d_seeds or NULL;
// total = n x m <= PWN_RAYS_MAX rays, m >= 1.  The divisors' magic numbers come from the caller (launch_plan.h is host code).
extern "C" hipError_t pwn_launch_pixel_rays(const pwn_view_rec *d_recs, const int32_t *d_xy, float *d_rays, uint32_t *d_seeds, uint32_t total,
	uint32_t m, uint32_t m_magic, int m_shift, int shared, int width, uint32_t w_magic, int w_shift, hipStream_t stream)
{
	if(total == 0u) return hipSuccess;
	const dim3 grid((total + PIXEL_RAYS_BLOCK - 1u) / PIXEL_RAYS_BLOCK), block(PIXEL_RAYS_BLOCK);
	hipLaunchKernelGGL(pwn_pixel_rays_kernel, grid, block, 0, stream, (const float4 *)d_recs, (const int2 *)d_xy, (uint4 *)d_rays, d_seeds,
		total, m, m_magic, m_shift, shared, (uint32_t)width, w_magic, w_shift);
	return hipGetLastError();
}
