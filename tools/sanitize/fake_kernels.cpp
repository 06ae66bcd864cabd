// CPU stand-ins for libpwnhip's kernels, for the sanitizer builds of its host logic (tools/sanitize/README.txt).  They do NOT
// compute the product's pixels.  What they keep is what the choreography depends on:
//   trace   writes a value per pixel that depends on (x, y, sec, camera, the tables' checksum): a stale table or a stale row shows;
//           depth is small except in a band of rows that FAKE_DEEP_ROWS moves through the frame, where it is large
//   blur    out(x, y) mixes the pixel with the one `reach(depth)` rows below it, like the reference's taps reach 0.002*h*|depth-1| rows
//           (screen.h:100-102): a missing halo row shows as a wrong pixel, a tap outside the rows it was given is counted in *miss
// so that a frame row-tiled over N members equals the frame of one context, bit for bit, exactly when strips, halo rows, the
// repeat after a missed halo, the gather and the delivery are right.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <initializer_list>
#include "pwn_internal.h"
#include "trace_variants.h"

static uint32_t mix(uint32_t a, uint32_t b) { a ^= b + 0x9e3779b9u + (a << 6) + (a >> 2); return a * 2654435761u; }

// (tables_driver.cpp looks at what a launch is handed: the tables as the kernels would read them; calls_driver.cpp writes every
// launch down: the trace and blur launches with their parameters, the small ones with their name, source, destination and sizes;
// players_driver.cpp looks at the walk table a step is handed)
extern "C" {
void (*pwn_fake_trace_hook)(const pwn_trace_params *P, int grid, size_t lds_bytes) = NULL;
void (*pwn_fake_blur_hook)(const pwn_blur_params *B) = NULL;
void (*pwn_fake_launch_hook)(const char *name, const void *src, const void *dst, int nsizes, const size_t *sizes) = NULL;
void (*pwn_fake_players_hook)(const pwn_walk_table *walk, int n, int ticks, int stage) = NULL;
void (*pwn_fake_sphere_bins_hook)(const void *d_scratch, const void *d_base, const void *d_blob) = NULL;
void (*pwn_fake_viewport_setup_hook)(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm, const pwn_viewport_rec *out, int n) = NULL;
}
static void small_launch(const char *name, const void *src, const void *dst, std::initializer_list<size_t> sizes)
{
	if(pwn_fake_launch_hook != NULL) pwn_fake_launch_hook(name, src, dst, (int)sizes.size(), sizes.begin());
}
// (the mode of the calling thread's last trace launch, set before the hook runs: the drivers require the exact mode per call; -1: none
// yet.  Per thread: a group's members launch from threads of their own)
extern "C" { thread_local int pwn_fake_trace_mode = -1; }
static hipError_t reach_records(const pwn_trace_params *P, bool count);
extern "C" hipError_t pwn_launch_trace(int mode, int, bool, const pwn_trace_params *P, int grid, size_t lds_bytes, bool count, hipStream_t)
{
	// (a mode without a row of the table is no kernel, as in trace_kernel.hip; the refill kernel's launches come with PWN_KM_FRAME)
	switch(mode)
	{
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) case (MODE):
	PWN_TRACE_VARIANTS(PWN_ROW)
#undef PWN_ROW
		break;
		default: return hipErrorInvalidValue;
	}
	pwn_fake_trace_mode = mode;
	if(pwn_fake_trace_hook != NULL) pwn_fake_trace_hook(P, grid, lds_bytes);
	if((mode & PWN_KM_REACH) != 0) return reach_records(P, count);
	// first-hit planes of views (pwn_trace_view_hits; view_hits_driver.cpp): a word per pixel of every plane given that depends on the
	// plane, the view's record and the pixel -- every word of n x h x w, and none beside them
	const int what = mode & ~(PWN_KM_HIDE | PWN_KM_REACH);
	if(what == PWN_KM_VIEW_HITS)
	{
		for(int v = 0; v < P->nviews; v++)
		{
			uint32_t rec = 0;
			for(int i = 0; i < 20; i++) { uint32_t u; memcpy(&u, (const float *)&P->views[v] + i, 4); rec = mix(rec, u); }
			for(int y = P->y0; y < P->y1; y++)
				for(int x = 0; x < P->w; x++)
				{
					const size_t o = (size_t)v * P->plane + (size_t)y * P->w + x;
					const uint32_t k = mix(mix((uint32_t)x, (uint32_t)y), rec);
					((uint32_t *)P->hits)[o] = k;
					if(P->sbuf != NULL) P->sbuf[o] = k ^ 0x11111111u;
					if(P->zbuf != NULL) P->zbuf[o] = (float)(k >> 8);
				}
		}
		if(P->tickets_next) for(unsigned q = 0; q < PWN_QUEUES; q++) P->tickets_next[q * PWN_QUEUE_STRIDE] = 0u;
		if(count && P->counters) P->counters[0] += (unsigned long long)P->nviews * P->plane;
		return hipSuccess;
	}
	// first-hit planes of views of their own sizes (pwn_trace_viewport_hits; viewport_hits_driver.cpp): a word per pixel of every
	// rectangle in every plane given, at (rec.y + y) * w + rec.x + x, that depends on the plane, the record's head and rectangle and
	// the LOCAL pixel -- every word of every rectangle, and none beside them
	if(what == PWN_KM_VIEWPORT_HITS)
	{
		unsigned long long pixels = 0;
		for(int v = 0; v < P->nvp; v++)
		{
			const pwn_viewport_rec &r = P->vps[v];
			uint32_t rec = 0;
			for(int i = 0; i < 16; i++) { uint32_t u; memcpy(&u, (const float *)&r + i, 4); rec = mix(rec, u); }
			rec = mix(mix(rec, (uint32_t)r.w), (uint32_t)r.h);
			for(int y = 0; y < r.h; y++)
				for(int x = 0; x < r.w; x++)
				{
					const size_t o = (size_t)(r.y + y) * P->w + (size_t)(r.x + x);
					const uint32_t k = mix(mix((uint32_t)x, (uint32_t)y), rec) | 1u;
					((uint32_t *)P->hits)[o] = k;
					if(P->sbuf != NULL) P->sbuf[o] = k ^ 0x11111110u;
					if(P->zbuf != NULL) P->zbuf[o] = (float)(k >> 8) + 1.0f;
				}
			pixels += (unsigned long long)r.w * r.h;
		}
		if(P->tickets_next) for(unsigned q = 0; q < PWN_QUEUES; q++) P->tickets_next[q * PWN_QUEUE_STRIDE] = 0u;
		if(count && P->counters) P->counters[0] += pixels;
		return hipSuccess;
	}
	uint32_t tab = 0;
	for(uint32_t i = 0; i < P->blob_bytes / 4; i += 7) tab = mix(tab, P->blob[i]);
	uint32_t secbits, cambits = 0;
	memcpy(&secbits, &P->sec_current, 4);
	for(int i = 0; i < 4; i++) { uint32_t u; memcpy(&u, &P->rayb[i], 4); cambits = mix(cambits, u); memcpy(&u, &P->from[i], 4); cambits = mix(cambits, u); }
	const int deep0 = (int)(fabsf(P->sec_current) * 37.0f) % (P->h > 8 ? P->h - 8 : 1);
	for(int y = P->y0; y < P->y1; y++)
		for(int x = 0; x < P->w; x++)
		{
			const size_t o = (size_t)y * P->w + x;
			P->sbuf[o] = mix(mix(mix((uint32_t)x, (uint32_t)y), secbits ^ tab), cambits);
			// (like a ray that runs out of steps, trace.h:677: every 97th pixel keeps the depth it had)
			if((x + 3 * y) % 97 != 0) P->zbuf[o] = (P->sec_current >= 100.0f && y >= deep0 && y < deep0 + 8) ? 400.0f : 1.0f + (float)((x + y + (secbits >> 20)) % 9);
		}
	if(P->clear_word) *P->clear_word = 0u;
	if(P->cost_word) *P->cost_word += (uint32_t)(P->y1 - P->y0) * 10u + (uint32_t)(P->y0 % 7);
	if(P->tickets_next) for(unsigned q = 0; q < PWN_QUEUES; q++) P->tickets_next[q * PWN_QUEUE_STRIDE] = 0u;
	if(count && P->counters) { P->counters[0] += (unsigned long long)(P->y1 - P->y0) * P->w * 3ull; P->counters[1] += (unsigned long long)(P->y1 - P->y0) * P->w * 12ull; }
	return hipSuccess;
}
extern "C" hipError_t pwn_launch_trace_refill(const pwn_trace_params *P, int g, size_t l, bool c, hipStream_t s) { return pwn_launch_trace(PWN_KM_FRAME, PWN_LF_INDEXED, false, P, g, l, c, s); }
// (the HIDE bit of a mode changes nothing here: what the hide words do to a pixel is the kernels' business)
// (the REACH bit; reach_driver.cpp: a record per ray made of the ray's number, its eight floats, its reach and its hide word -- exactly n
// entries of each array are read, exactly n records written)
static hipError_t reach_records(const pwn_trace_params *P, bool count)
{
	for(uint32_t i = 0; i < P->nrays; i++)
	{
		uint32_t k = mix(i, P->ray_hide != NULL ? (uint32_t)P->ray_hide[i] : 0x5555u), u;
		for(int q = 0; q < 8; q++) { memcpy(&u, P->rays + 8 * (size_t)i + q, 4); k = mix(k, (P->ray_w || (q & 3) != 3) ? u : 0u); }
		memcpy(&u, P->ray_reach + i, 4);
		k = mix(k, u);
		uint32_t *o = (uint32_t *)((unsigned char *)P->hits + (size_t)i * PWN_HIT_REC_BYTES);
		for(uint32_t q = 0; q < PWN_HIT_REC_BYTES / 4u; q++) o[q] = mix(k, q);
	}
	if(P->tickets_next) for(unsigned q = 0; q < PWN_QUEUES; q++) P->tickets_next[q * PWN_QUEUE_STRIDE] = 0u;
	if(count && P->counters) P->counters[0] += P->nrays;
	return hipSuccess;
}
extern "C" unsigned pwn_trace_refill_lds_extra(bool) { return 16u; }
extern "C" int pwn_trace_refill_blocks_per_cu(size_t, bool, bool) { return 4; }
extern "C" int pwn_trace_blocks_per_cu(size_t, bool, bool) { return 5; }
extern "C" int pwn_trace_global_blocks_per_cu(size_t, bool, bool) { return 5; }
extern "C" int pwn_trace_tile_h(void) { return 4; }
extern "C" int pwn_trace_tile_w(void) { return 16; }
extern "C" unsigned pwn_trace_lds_extra(void) { return 16u; }

extern "C" hipError_t pwn_launch_blur(const pwn_blur_params *B, hipStream_t)
{
	if(pwn_fake_blur_hook != NULL) pwn_fake_blur_hook(B);
	if(B->cost_acc != NULL) { *B->cost_out = (uint32_t)((unsigned long long)*B->cost_acc * B->cost_mul / B->cost_div); *B->cost_acc = 0u; }
	unsigned missed = 0;
	for(int y = B->y0; y < B->y1; y++)
		for(int x = 0; x < B->w; x++)
		{
			const size_t o = (size_t)y * B->w + x;
			const float z = B->zbuf[o];
			int reach = (int)(0.002f * (float)B->h * fabsf(z - 1.0f));
			int ty = y + ((x & 1) ? reach : -reach);
			ty = ty < 0 ? 0 : (ty >= B->h ? B->h - 1 : ty);
			if(B->miss != NULL && (unsigned)(ty - B->avail_y0) >= (unsigned)(B->avail_y1 - B->avail_y0)) missed++;
			B->out[o] = mix(B->pre[o], B->pre[(size_t)ty * B->w + x]);
		}
	if(B->miss != NULL && missed) *B->miss += missed;
	return hipSuccess;
}
extern "C" hipError_t pwn_launch_order(const uint16_t *cost, uint32_t units, uint32_t cap, uint32_t *perm, hipStream_t) { small_launch("order", cost, perm, { units, cap }); return hipSuccess; }
extern "C" hipError_t pwn_launch_upscale(const uint32_t *src, uint32_t *dst, int w, int h, int scale, int pitch, hipStream_t)
{
	small_launch("upscale", src, dst, { (size_t)w, (size_t)h, (size_t)scale, (size_t)pitch });
	const size_t rowadv = (size_t)w * scale + (size_t)pitch * (scale - 1);
	for(int dy = 0; dy < h * scale; dy++) for(int dx = 0; dx < w * scale; dx++)
		dst[(size_t)(dy / scale) * rowadv + (size_t)(dy % scale) * pitch + dx] = src[(size_t)(dy / scale) * w + dx / scale];
	return hipSuccess;
}
extern "C" hipError_t pwn_launch_upload(const void *src, void *dst, size_t bytes, hipStream_t) { small_launch("upload", src, dst, { bytes }); memcpy(dst, src, bytes); return hipSuccess; }
// (the camera set-up of pwn_trace_views_device: view_setup.hip's arithmetic, on "device" memory that is host memory here)
static hipError_t view_setup(const float *cams, const float *secs, const int32_t *hide, pwn_view_rec *out, int n, int w, int h);
extern "C" hipError_t pwn_launch_view_setup(const float *cams, const float *secs, pwn_view_rec *out, int n, int w, int h, hipStream_t)
{
	small_launch("view_setup", cams, out, { (size_t)n, (size_t)w, (size_t)h });
	return view_setup(cams, secs, NULL, out, n, w, h);
}
// (... with every view's hidden sphere, pwn_trace_views_hide_device: reads exactly n entries of hide)
extern "C" hipError_t pwn_launch_view_setup_hide(const float *cams, const float *secs, const int32_t *hide, pwn_view_rec *out, int n, int w, int h, hipStream_t)
{
	small_launch("view_setup_hide", cams, out, { (size_t)n, (size_t)w, (size_t)h });
	return view_setup(cams, secs, hide, out, n, w, h);
}
static hipError_t view_setup(const float *cams, const float *secs, const int32_t *hide, pwn_view_rec *out, int n, int w, int h)
{
	const pwn_setup_scalars S = pwn_frame_setup_scalars(w, h);
	for(int v = 0; v < n; v++)
	{
		const float *cam = cams + 16 * (size_t)v;
		pwn_view_rec r;
		memset(&r, 0, sizeof(r));
		for(int i = 0; i < 4; i++)
		{
			r.rayb[i] = (cam[0 + i] + cam[8 + i]) + (-S.yrat) * cam[4 + i];
			r.rdx[i] = S.xsrat * cam[0 + i];
			r.rdy[i] = S.ysrat * cam[4 + i];
			r.from[i] = cam[12 + i];
		}
		r.sec_current = secs != NULL ? secs[v] : 0.0f;
		if(hide != NULL && hide[v] >= 0 && hide[v] < PWN_OBJ_MAX) r.hide = (uint32_t)hide[v] + 1u;
		out[v] = r;
	}
	return hipSuccess;
}
// (the records of pwn_trace_viewports_device; viewports_device_driver.cpp: viewport_setup.hip's algorithm, one record after the other --
// the geometry words from the master copy, the head from camera perm[j] with the view's own scalars, every product and sum rounded
// by itself.  Reads exactly n master records, n scalar words, n perm entries, n cameras and n times, writes n records.)
static hipError_t viewport_setup(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm, const float *cams, const float *secs,
	const int32_t *hide, pwn_viewport_rec *out, int n);
extern "C" hipError_t pwn_launch_viewport_setup(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm,
	const float *cams, const float *secs, pwn_viewport_rec *out, int n, hipStream_t)
{
	small_launch("viewport_setup", cams, out, { (size_t)n });
	return viewport_setup(master, scal, perm, cams, secs, NULL, out, n);
}
// (... with every rectangle's hidden sphere, pwn_trace_viewports_hide_device: reads exactly n entries of hide, entry perm[j] for record j.
// The same launch name: the drivers count set-up launches by it; pwn_fake_viewport_hide_hook says which array one was handed)
extern "C" void (*pwn_fake_viewport_hide_hook)(const int32_t *hide, int n);
void (*pwn_fake_viewport_hide_hook)(const int32_t *hide, int n) = NULL;
extern "C" hipError_t pwn_launch_viewport_setup_hide(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm,
	const float *cams, const float *secs, const int32_t *hide, pwn_viewport_rec *out, int n, hipStream_t)
{
	small_launch("viewport_setup", cams, out, { (size_t)n });
	if(pwn_fake_viewport_hide_hook != NULL) pwn_fake_viewport_hide_hook(hide, n);
	return viewport_setup(master, scal, perm, cams, secs, hide, out, n);
}
static hipError_t viewport_setup(const pwn_viewport_rec *master, const float *scal, const uint32_t *perm, const float *cams, const float *secs,
	const int32_t *hide, pwn_viewport_rec *out, int n)
{
	for(int j = 0; j < n; j++)
	{
		const uint32_t i = perm[j];
		if(i >= (uint32_t)n) continue;
		const float *cam = cams + 16 * (size_t)i, yrat_neg = scal[4 * (size_t)j], xsrat = scal[4 * (size_t)j + 1], ysrat = scal[4 * (size_t)j + 2];
		pwn_viewport_rec r = master[j];
		for(int k = 0; k < 4; k++)
		{
			r.rayb[k] = (cam[0 + k] + cam[8 + k]) + yrat_neg * cam[4 + k];
			r.rdx[k] = xsrat * cam[0 + k];
			r.rdy[k] = ysrat * cam[4 + k];
		}
		memcpy(r.from, cam + 12, 16);
		if(secs != NULL) memcpy(&r.sec_current, secs + i, 4);
		else r.sec_current = 0.0f;
		if(hide != NULL) r.hide = hide[i] >= 0 && hide[i] < PWN_OBJ_MAX ? (uint32_t)hide[i] + 1u : 0u;
		out[j] = r;
	}
	if(pwn_fake_viewport_setup_hook != NULL) pwn_fake_viewport_setup_hook(master, scal, perm, out, n);
	return hipSuccess;
}
// (the players' step: every player's position moves by a number that depends on its key byte, the ticks and the walk table -- which
// player, which keys and which level a call was given shows; host/player.c is the arithmetic's model, not this)
extern "C" hipError_t pwn_launch_players_step(float *cams, float *gravity, int32_t *traversals, const uint8_t *keys, int n, float tdiff, int ticks,
	const pwn_walk_table *walk, int stage, hipStream_t)
{
	small_launch("players_step", keys, cams, { (size_t)n, (size_t)ticks, (size_t)stage });
	if(pwn_fake_players_hook != NULL) pwn_fake_players_hook(walk, n, ticks, stage);
	uint32_t tab = 0;
	for(int i = 0; i < 4096; i += 5) tab = mix(tab, walk->cells[i]);
	for(int i = 0; i < n; i++)
	{
		cams[16 * (size_t)i + 12] += tdiff * (float)ticks * (float)(keys[i] + 1) + (float)(tab & 7u);
		gravity[4 * (size_t)i + 1] -= tdiff;
		if(traversals != NULL) traversals[i] += ticks;
	}
	return hipSuccess;
}
// (the rays of pwn_pixel_rays_device; pixel_rays_driver.cpp: every byte of the two output ranges and none beside them, each word
// made of the ray's number, its camera's record and its pixel -- every record and every pixel pair of the ranges given is read, and
// which camera, which pixel and which layout a call was given shows; pwn_pixel_rays is the arithmetic's model, not this)
extern "C" hipError_t pwn_launch_pixel_rays(const pwn_view_rec *recs, const int32_t *xy, float *rays, uint32_t *seeds, uint32_t total,
	uint32_t m, uint32_t m_magic, int m_shift, int shared, int width, uint32_t w_magic, int w_shift, hipStream_t)
{
	small_launch("pixel_rays", recs, rays, { (size_t)total, (size_t)m, (size_t)shared, (size_t)width });
	for(uint32_t i = 0; i < total; i++)
	{
		const uint32_t cam = m_shift >= 0 ? (uint32_t)(((unsigned long long)i * m_magic) >> 32) >> m_shift : i, j = i - cam * m;
		int32_t x, y;
		if(xy != NULL) { x = xy[2 * (size_t)(shared ? j : i)]; y = xy[2 * (size_t)(shared ? j : i) + 1]; }
		else { const uint32_t row = w_shift >= 0 ? (uint32_t)(((unsigned long long)j * w_magic) >> 32) >> w_shift : j; x = (int32_t)(j - row * (uint32_t)width); y = (int32_t)row; }
		uint32_t rec = 0;
		for(int k = 0; k < 20; k++) { uint32_t u; memcpy(&u, (const float *)&recs[cam] + k, 4); rec = mix(rec, u); }
		const uint32_t key = mix(mix(rec, (uint32_t)x), mix((uint32_t)y, i));
		for(int k = 0; k < 8; k++) { const uint32_t u = mix(key, (uint32_t)k) & 0x3fffffffu; memcpy(&rays[8 * (size_t)i + k], &u, 4); }
		if(seeds != NULL) seeds[i] = key;
	}
	return hipSuccess;
}
// (the tables of pwn_upload_spheres_device; spheres_device_driver.cpp: sphere_bins.hip's four launches as one sequential pass that reads
// and writes exactly what they do -- the n records, the whole base copy, the scratch's words, the blob's level part and liststart
// below the non-empty cells, the device-memory part's records up to and including the read-ahead one, which[] and the spheres --
// through sphere_box.h, the arithmetic the kernels share with the host.  Here the stand-in IS the model: the tables it leaves
// are held against pwn_i_pack_blob's by the driver.)
#include "sphere_box.h"
extern "C" hipError_t pwn_launch_sphere_bins(const void *d_spheres, uint32_t n, uint32_t max_pairs, void *d_scratch, const void *d_base,
	void *d_blob, void *d_big, uint64_t which_off, uint64_t sph_off, hipStream_t)
{
	small_launch("sphere_bins", d_spheres, d_big, { (size_t)n, (size_t)max_pairs, (size_t)which_off, (size_t)sph_off });
	if(pwn_fake_sphere_bins_hook != NULL) pwn_fake_sphere_bins_hook(d_scratch, d_base, d_blob);
	uint32_t *box = (uint32_t *)d_scratch, *count = box + PWN_SD_BOX_WORDS, *start = count + 4096, *status = box + PWN_SD_STATUS_WORD;
	uint32_t *rec = (uint32_t *)d_big, *which = (uint32_t *)((uint8_t *)d_big + which_off), *sph = (uint32_t *)((uint8_t *)d_big + sph_off);
	const uint32_t *in = (const uint32_t *)d_spheres;
	memcpy(d_blob, d_base, PWN_T_BINIDX);
	for(uint32_t i = 0; i < n; i++)
	{
		const uint32_t *q = in + 8 * (size_t)i;
		float r, x, z;
		memcpy(&r, q + 0, 4); memcpy(&x, q + 2, 4); memcpy(&z, q + 4, 4);
		box[i] = pwn_box_pack(x, z, r);
		const float r2 = pwn_box_r2(r);
		uint32_t *o = sph + 8 * (size_t)i;
		o[0] = q[2]; o[1] = q[3]; o[2] = q[4]; memcpy(o + 3, &r2, 4);
		o[4] = q[1]; o[5] = q[5]; o[6] = q[6]; o[7] = q[7];
	}
	uint32_t pairs = 0, ncell = 0, longest = 0;
	for(uint32_t cell = 0; cell < 4096; cell++)
	{
		uint32_t k = 0;
		for(uint32_t i = 0; i < n; i++) k += pwn_box_covers(box[i], cell & 63u, cell >> 6) != 0;
		count[cell] = k; start[cell] = pairs;
		pairs += k; ncell += k != 0; if(k > longest) longest = k;
	}
	const uint32_t reason = pairs > max_pairs ? 1u : (longest > (uint32_t)PWN_LIST_MAX ? 2u : 0u);
	status[PWN_SD_ST_PAIRS] = pairs; status[PWN_SD_ST_NCELL] = ncell; status[PWN_SD_ST_LONGEST] = longest; status[PWN_SD_ST_REASON] = reason;
	status[PWN_SD_ST_N] = n; status[PWN_SD_ST_MAX_PAIRS] = max_pairs;
	if(reason != 0u) return hipSuccess;
	uint32_t *cells = (uint32_t *)d_blob + PWN_T_CELLINFO / 4u, *liststart = (uint32_t *)d_blob + PWN_T_BINIDX / 4u, ord = 0;
	for(uint32_t cell = 0; cell < 4096; cell++)
	{
		if(count[cell] == 0u) continue;
		liststart[ord] = start[cell];
		cells[(cell >> 6) * PWN_GRID_PITCH + (cell & 63u)] |= PWN_C_SPH | (ord << 16);
		ord++;
		uint32_t k = start[cell];
		for(uint32_t i = 0; i < n; i++)
		{
			if(!pwn_box_covers(box[i], cell & 63u, cell >> 6)) continue;
			memcpy(rec + 4 * (size_t)k, sph + 8 * (size_t)i, 16);
			if(k + 1u == start[cell] + count[cell]) rec[4 * (size_t)k + 3] |= 0x80000000u;
			which[k++] = i;
		}
	}
	memset(rec + 4 * (size_t)pairs, 0, 16);
	return hipSuccess;
}
extern "C" hipError_t pwn_launch_words(const uint32_t *all, const uint32_t *own, uint32_t *h, int world, hipStream_t)
{
	for(int i = 0; i < 2 * world + 2; i++) h[i] = i < 2 * world ? all[i] : own[i - 2 * world];
	return hipSuccess;
}
extern "C" hipError_t pwn_launch_probe(int, const uint32_t *in, uint32_t *out, int n, const uint16_t *, hipStream_t) { for(int i = 0; i < n; i++) out[i] = in[i]; return hipSuccess; }
// (the level of pwn_upload_level_device; level_device_driver.cpp: level_bake.hip's algorithm, sequentially, over level_bake.h -- the rules the
// kernel shares with the host.  Reads exactly the 4096 cell bytes and, where given, the 182 words of the table; writes the cell words
// and the records of the base copy and the walk table, or on another verdict the walk table alone, from the previous one; and the
// status words.  Here too the stand-in IS the model: the driver holds what it leaves against pwn_bake_cells.)
#include "level_bake.h"
extern "C" { void (*pwn_fake_level_bake_hook)(const void *d_data, const void *d_pmap, const void *d_base, const void *d_walk, const void *d_walk_prev, const void *d_status) = NULL; }
extern "C" hipError_t pwn_launch_level_bake(const void *d_data, const void *d_pmap, void *d_base, pwn_walk_table *d_walk,
	const pwn_walk_table *d_walk_prev, uint32_t *status, int prev_dev, hipStream_t)
{
	small_launch("level_bake", d_data, d_walk, { (size_t)(d_pmap != NULL), (size_t)(prev_dev != 0) });
	if(pwn_fake_level_bake_hook != NULL) pwn_fake_level_bake_hook(d_data, d_pmap, d_base, d_walk, d_walk_prev, status);
	uint8_t cells[4096];
	int32_t pmap[26 * PWN_LB_PM_WORDS];
	memcpy(cells, d_data, 4096);
	const bool derived = d_pmap == NULL;
	if(!derived) memcpy(pmap, d_pmap, sizeof(pmap));
	else
	{
		uint32_t first[26], second[26];
		for(int i = 0; i < 26; i++) first[i] = second[i] = 0xffffffffu;
		for(uint32_t cell = 0; cell < 4096u; cell++)
		{
			const int c = cells[cell];
			if(c < 'A' || c > 'Z') continue;
			if(first[c - 'A'] == 0xffffffffu) first[c - 'A'] = cell;
			else if(second[c - 'A'] == 0xffffffffu) second[c - 'A'] = cell;
		}
		for(int i = 0; i < 26; i++) pwn_lb_derive_letter(cells, first[i], second[i], pmap + PWN_LB_PM_WORDS * i);
	}
	uint32_t bad1 = 26u, bad2 = 26u;
	for(int i = 25; i >= 0; i--) if(pwn_lb_coords_bad(pmap + PWN_LB_PM_WORDS * i)) bad1 = (uint32_t)i;
	for(int t = 0; t < 130; t++) { const int l = pwn_lb_outside_letter_nth(cells, pmap, t); if(l >= 0 && (uint32_t)l < bad2) bad2 = (uint32_t)l; }
	const uint32_t verdict = bad1 < 26u ? (uint32_t)PWN_LB_BAD_COORD : (bad2 < 26u ? (uint32_t)PWN_LB_BAD_OUTSIDE : (uint32_t)PWN_LB_TAKEN);
	if(verdict != PWN_LB_TAKEN)
	{
		const uint32_t dev = prev_dev ? status[PWN_LD_ST_DEV] : 0u;
		memcpy(d_walk, d_walk_prev, sizeof(pwn_walk_table));
		memset(status, 0, PWN_LD_STATUS_WORDS * 4u);
		status[PWN_LD_ST_VERDICT] = verdict; status[PWN_LD_ST_LETTER] = verdict == PWN_LB_BAD_COORD ? bad1 : bad2;
		status[PWN_LD_ST_DERIVED] = derived; status[PWN_LD_ST_DEV] = dev;
		return hipSuccess;
	}
	uint32_t *words = (uint32_t *)((uint8_t *)d_base + PWN_T_CELLINFO), *recs = (uint32_t *)((uint8_t *)d_base + PWN_T_EPREC), nrec = 0;
	memset(recs, 0, PWN_EP_MAX * 4u);
	for(int z = 0; z < 64; z++) for(int x = 0; x < 64; x++)
	{
		const int c = cells[z * 64 + x];
		uint32_t inside, outside, rec = 0;
		const int has = pwn_lb_cell_bits(c, x, z, pmap, nrec, &inside, &outside, &rec);
		if(has && nrec < PWN_EP_MAX) recs[nrec++] = rec;
		const uint32_t cls = pwn_cell_class((uint32_t)c);
		words[z * PWN_GRID_PITCH + x] = cls | inside;
		if(x == 0) words[z * PWN_GRID_PITCH + 64] = cls | outside;
		if(z == 0) words[64 * PWN_GRID_PITCH + x] = cls | outside;
		if(x == 0 && z == 0) words[64 * PWN_GRID_PITCH + 64] = cls | outside;
	}
	memset(d_walk, 0, sizeof(pwn_walk_table));
	memcpy(d_walk->cells, cells, 4096);
	memcpy(d_walk->pmap, pmap, sizeof(pmap));
	uint32_t paired = 0;
	for(int i = 0; i < 26; i++) paired += pmap[PWN_LB_PM_WORDS * i + PWN_LB_X1] != -1 && pmap[PWN_LB_PM_WORDS * i + PWN_LB_X2] != -1;
	memset(status, 0, PWN_LD_STATUS_WORDS * 4u);
	status[PWN_LD_ST_LETTER] = 26u; status[PWN_LD_ST_RECS] = nrec; status[PWN_LD_ST_PAIRED] = paired; status[PWN_LD_ST_DERIVED] = derived; status[PWN_LD_ST_DEV] = 1u;
	return hipSuccess;
}
