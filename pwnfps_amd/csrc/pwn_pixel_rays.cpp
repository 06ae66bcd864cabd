// pwn_pixel_rays.cpp -- pwn_pixel_rays_device: the ray records and seeds of chosen pixels of a batch of cameras, made on the
// device from cameras that are already there.  Two launches on the caller's stream and nothing else: the camera set-up of
// pwn_trace_views_device (view_setup.hip, denormals kept) into the caller's scratch, then the add chain per ray (pixel_rays.hip,
// flushed) -- the two halves of the host's pwn_pixel_rays (pwn_launch.cpp), each under the floating-point mode the host runs it in.
// The call owns no buffer, reads no tables and needs no level.
#include "pwn_internal.h"
#include "launch_plan.h"

extern "C" int pwn_pixel_rays_device(pwn_ctx *c, int width, int height, int n, const void *d_cams, int m, const void *d_xy, int flags,
	void *d_work, void *d_rays, void *d_seeds, void *stream)
{
	GRP_REFUSE(c, "pwn_pixel_rays_device");
	if(c == NULL || width < 1 || height < 1 || width > 32768 || height > 32768 || n < 0 || n > PWN_PLAYERS_MAX || m < 0) return PWN_EINVAL;
	const uint64_t total = (uint64_t)n * (uint64_t)m;
	if(total > (uint64_t)PWN_RAYS_MAX || (flags & ~PWN_PIXELS_SHARED) != 0) return PWN_EINVAL;
	const bool shared = (flags & PWN_PIXELS_SHARED) != 0;
	if(total > 0 && (d_cams == NULL || d_work == NULL || d_rays == NULL)) return PWN_EINVAL;
	// (no pixels given: the whole frame, which every camera then shares)
	if(total > 0 && d_xy == NULL && !(shared && (uint64_t)m == (uint64_t)width * (uint64_t)height)) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_work | (uintptr_t)d_rays) & 15u) != 0 || ((uintptr_t)d_xy & 7u) != 0 || ((uintptr_t)d_seeds & 3u) != 0) return PWN_EINVAL;
	{
		const uintptr_t N = (uintptr_t)n, T = (uintptr_t)total;
		const uintptr_t p[5] = { (uintptr_t)d_cams, (uintptr_t)d_xy, (uintptr_t)d_work, (uintptr_t)d_rays, (uintptr_t)d_seeds };
		const uintptr_t b[5] = { 64 * N, 8 * (shared ? (uintptr_t)m : T), PWN_PIXEL_WORK_BYTES * N, 32 * T, 4 * T };
		for(int i = 0; i < 5; i++) for(int k = i + 1; k < 5; k++)
			if(p[i] != 0 && p[k] != 0 && b[i] != 0 && b[k] != 0 && p[i] < p[k] + b[k] && p[k] < p[i] + b[i]) return PWN_EINVAL;
	}
	// (pwn_i_batch_refuse's rule for a context that runs a row tiling; no level is needed)
	if(c->tiled != NULL) return PWN_EBUSY;
	if(total == 0) return PWN_OK;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	HIPCHK(c, pwn_launch_view_setup((const float *)d_cams, NULL, (pwn_view_rec *)d_work, n, width, height, s));
	uint32_t m_magic, w_magic; int m_shift, w_shift;
	pwn_unit_div_magic((uint32_t)m, &m_magic, &m_shift);
	pwn_unit_div_magic((uint32_t)width, &w_magic, &w_shift);
	HIPCHK(c, pwn_launch_pixel_rays((const pwn_view_rec *)d_work, (const int32_t *)d_xy, (float *)d_rays, (uint32_t *)d_seeds, (uint32_t)total,
		(uint32_t)m, m_magic, m_shift, shared ? 1 : 0, width, w_magic, w_shift, s));
	return PWN_OK;
}
