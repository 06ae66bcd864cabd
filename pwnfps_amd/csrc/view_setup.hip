// view_setup.hip -- the camera set-up of a batch of views on the device (pwn_trace_views_device): frame_setup of pwn_internal.h,
// one thread per view, from cameras that are already in device memory.
//
// This file is built with -fno-gpu-flush-denormals-to-zero (csrc/Makefile), alone of all the HIP files here: frame_setup runs
// on the host with denormals kept, so the sum of two denormal camera entries is a normal number there, and must be here.  The
// trace kernel flushes what it reads from the record, as it flushes what the host's set-up hands it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwn_internal.h"

static_assert(sizeof(pwn_view_rec) == PWN_VIEWS_REC_BYTES, "a view record is five 16-byte words");

// yrat_neg = -yrat, xsrat and ysrat are frame_setup's camera-independent scalars, computed on the host (pwn_internal.h
// pwn_setup_scalars): the divisions stay there.  Every multiply and add below is rounded on its own (-ffp-contract=off).
__global__ void __launch_bounds__(64)
pwn_view_setup_kernel(const float4 *__restrict__ cams, const float *__restrict__ secs, const int32_t *__restrict__ hide,
	float4 *__restrict__ out, int n, float yrat_neg, float xsrat, float ysrat)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	if(i >= n) return;
	const float4 cx = cams[4 * (size_t)i + 0], cy = cams[4 * (size_t)i + 1], cz = cams[4 * (size_t)i + 2], cw = cams[4 * (size_t)i + 3];
	float4 rayb, rdx, rdy;
	rayb.x = (cx.x + cz.x) + yrat_neg * cy.x; rayb.y = (cx.y + cz.y) + yrat_neg * cy.y;
	rayb.z = (cx.z + cz.z) + yrat_neg * cy.z; rayb.w = (cx.w + cz.w) + yrat_neg * cy.w;
	rdx.x = xsrat * cx.x; rdx.y = xsrat * cx.y; rdx.z = xsrat * cx.z; rdx.w = xsrat * cx.w;
	rdy.x = ysrat * cy.x; rdy.y = ysrat * cy.y; rdy.z = ysrat * cy.z; rdy.w = ysrat * cy.w;
	float4 *r = out + 5 * (size_t)i;
	r[0] = rayb; r[1] = rdx; r[2] = rdy; r[3] = cw;
	// The record's `hide` word (tables.h pwn_view_rec): k + 1 for a value k that can be a sphere's index, 0 for every other one and
	// where the call has no array.  The value is compared and incremented, nothing else.
	uint32_t hide1 = 0u;
	if(hide != NULL)
	{
		const int32_t k = hide[i];
		if(k >= 0 && k < PWN_OBJ_MAX) hide1 = (uint32_t)k + 1u;
	}
	r[4] = make_float4(secs != NULL ? secs[i] : 0.0f, __uint_as_float(hide1), 0.0f, 0.0f);        // sec_current (none: pwn_trace_view_hits_device), hide, the padding
}

// (d_cams and d_out 16-byte aligned: the kernel moves whole float4)
// (d_hide: NULL, or n int32, each view's hidden sphere -- pwn_trace_views_hide_device)
extern "C" hipError_t pwn_launch_view_setup_hide(const float *d_cams, const float *d_secs, const int32_t *d_hide, pwn_view_rec *d_out, int n, int w, int h, hipStream_t stream)
{
	if(n <= 0) return hipSuccess;
	const pwn_setup_scalars S = pwn_frame_setup_scalars(w, h);
	hipLaunchKernelGGL(pwn_view_setup_kernel, dim3((n + 63) / 64), dim3(64), 0, stream,
		(const float4 *)d_cams, d_secs, d_hide, (float4 *)d_out, n, -S.yrat, S.xsrat, S.ysrat);
	return hipGetLastError();
}
extern "C" hipError_t pwn_launch_view_setup(const float *d_cams, const float *d_secs, pwn_view_rec *d_out, int n, int w, int h, hipStream_t stream)
{
	return pwn_launch_view_setup_hide(d_cams, d_secs, NULL, d_out, n, w, h, stream);
}
