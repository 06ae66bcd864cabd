// viewport_setup.hip -- the records of pwn_trace_viewports_device on the device: one thread per record of the launch, which takes the
// record's geometry words from the layout's master copy (baked on the host at layout creation, pwn_calls.cpp
// pwn_i_viewport_recs_bake) and makes its head -- frame_setup of pwn_internal.h for a frame of the VIEW's own size -- from the camera
// of the rectangle the record stands for, which is already in device memory.
//
// Built as view_setup.hip is (csrc/Makefile: -fno-gpu-flush-denormals-to-zero, -ffp-contract=off), for the same reason: frame_setup
// runs on the host with denormals kept and every multiply and add rounded on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwn_internal.h"

static_assert(sizeof(pwn_viewport_rec) == PWN_VP_REC_BYTES, "a viewport record is eight 16-byte words");
static_assert(offsetof(pwn_viewport_rec, sec_current) == 64 && offsetof(pwn_viewport_rec, x) == 68, "the head is four 16-byte words and the time");
static_assert(offsetof(pwn_viewport_rec, hide) == 120, "the hide word is word 30: the third of the record's last 16-byte word");

// Record j stands for rectangle perm[j] (the records are in order of rising units, the cameras in the caller's order).
// scal[j] = (-yrat, xsrat, ysrat, 0) of the view's own w x h (pwn_frame_setup_scalars, computed on the host: the divisions stay there).
// Every index is j, or a perm[j] that the library wrote and checked to be below n: no bit of a camera reaches an address.
__global__ void __launch_bounds__(64)
pwn_viewport_setup_kernel(const uint4 *__restrict__ master, const float4 *__restrict__ scal, const uint32_t *__restrict__ perm,
	const float4 *__restrict__ cams, const uint32_t *__restrict__ secs, const int32_t *__restrict__ hide, uint4 *__restrict__ out, int n)
{
	const int j = blockIdx.x * 64 + threadIdx.x;
	if(j >= n) return;
	const uint32_t i = perm[j];
	if(i >= (uint32_t)n) return;
	const float4 s = scal[j];
	const float yrat_neg = s.x, xsrat = s.y, ysrat = s.z;
	const float4 cx = cams[4 * (size_t)i + 0], cy = cams[4 * (size_t)i + 1], cz = cams[4 * (size_t)i + 2];
	const uint4 cw = ((const uint4 *)cams)[4 * (size_t)i + 3];        // (row w: copied as bits)
	float4 rayb, rdx, rdy;
	rayb.x = (cx.x + cz.x) + yrat_neg * cy.x; rayb.y = (cx.y + cz.y) + yrat_neg * cy.y;
	rayb.z = (cx.z + cz.z) + yrat_neg * cy.z; rayb.w = (cx.w + cz.w) + yrat_neg * cy.w;
	rdx.x = xsrat * cx.x; rdx.y = xsrat * cx.y; rdx.z = xsrat * cx.z; rdx.w = xsrat * cx.w;
	rdy.x = ysrat * cy.x; rdy.y = ysrat * cy.y; rdy.z = ysrat * cy.z; rdy.w = ysrat * cy.w;
	const uint4 *m = master + 8 * (size_t)j;
	uint4 g4 = m[4];                 // sec_current (the master's is 0), x, y, w
	g4.x = secs != NULL ? secs[i] : 0u;        // (no times: pwn_trace_viewport_hits_device, whose launch reads none)
	uint4 *r = out + 8 * (size_t)j;
	r[0] = make_uint4(__float_as_uint(rayb.x), __float_as_uint(rayb.y), __float_as_uint(rayb.z), __float_as_uint(rayb.w));
	r[1] = make_uint4(__float_as_uint(rdx.x), __float_as_uint(rdx.y), __float_as_uint(rdx.z), __float_as_uint(rdx.w));
	r[2] = make_uint4(__float_as_uint(rdy.x), __float_as_uint(rdy.y), __float_as_uint(rdy.z), __float_as_uint(rdy.w));
	r[3] = cw;
	// The record's `hide` word (tables.h pwn_viewport_rec, view_setup.hip's rule): k + 1 for a value k that can be a sphere's index, 0 for
	// every other one and where the call has no array (the master's word is 0: pwn_i_viewport_recs_bake).  The entry is the RECTANGLE's,
	// hide[perm[j]], as the camera is.  The value is compared and incremented, nothing else.
	uint4 g7 = m[7];                 // seg_magic, seg_shift, hide, padding
	if(hide != NULL)
	{
		const int32_t k = hide[i];
		g7.z = k >= 0 && k < PWN_OBJ_MAX ? (uint32_t)k + 1u : 0u;
	}
	r[4] = g4; r[5] = m[5]; r[6] = m[6]; r[7] = g7;        // h, units_x, ux_magic, ux_shift; rows_u, units, seg_first, seg_round; seg_magic, seg_shift, hide, padding
}

// (d_master, d_scal, d_cams and d_out 16-byte aligned: the kernel moves whole 16-byte words)
// (d_hide: NULL, or n int32 in the caller's order, each rectangle's hidden sphere -- pwn_trace_viewports_hide_device)
extern "C" hipError_t pwn_launch_viewport_setup_hide(const pwn_viewport_rec *d_master, const float *d_scal, const uint32_t *d_perm,
	const float *d_cams, const float *d_secs, const int32_t *d_hide, pwn_viewport_rec *d_out, int n, hipStream_t stream)
{
	if(n <= 0) return hipSuccess;
	hipLaunchKernelGGL(pwn_viewport_setup_kernel, dim3((n + 63) / 64), dim3(64), 0, stream,
		(const uint4 *)d_master, (const float4 *)d_scal, d_perm, (const float4 *)d_cams, (const uint32_t *)d_secs, d_hide, (uint4 *)d_out, n);
	return hipGetLastError();
}
extern "C" hipError_t pwn_launch_viewport_setup(const pwn_viewport_rec *d_master, const float *d_scal, const uint32_t *d_perm,
	const float *d_cams, const float *d_secs, pwn_viewport_rec *d_out, int n, hipStream_t stream)
{
	return pwn_launch_viewport_setup_hide(d_master, d_scal, d_perm, d_cams, d_secs, NULL, d_out, n, stream);
}
