// pwn_spheres_device.cpp -- pwn_upload_spheres_device: the sphere tables built on the device (sphere_bins.hip) from spheres that are
// already there, on the caller's stream, into the next copy of the tables' ring (pwn_tables.cpp), in the lists' device-memory form
// laid out for the capacity the caller declares.  At most five launches and no host wait: the four of the build and, once per level,
// the upload of the level's part of the blob (the base copy) from one pinned slot.  pwn_spheres_device_state reads the last build's
// status words back.
#include <string.h>
#include "pwn_internal.h"

static inline uint32_t lds_cells(int max_pairs) { return max_pairs < 4096 ? (uint32_t)max_pairs : 4096u; }

// The builder's own buffers, once: the scratch of a build, the base copy and its pinned slot, two events
int pwn_i_sd_buffers(pwn_ctx *c)
{
	pwn_ctx::spheres_device_state &d = c->sd;
	if(d.d_scratch != NULL) return PWN_OK;
	uint8_t *scratch = NULL, *base = NULL, *hbase = NULL;
	hipEvent_t e0 = NULL, e1 = NULL;
	if(hipMalloc((void **)&scratch, PWN_SD_SCRATCH_BYTES) != hipSuccess || hipMalloc((void **)&base, PWN_T_BINIDX) != hipSuccess ||
	   hipHostMalloc((void **)&hbase, PWN_T_BINIDX, hipHostMallocDefault) != hipSuccess ||
	   hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess)
	{
		(void)hipGetLastError();
		(void)hipFree(scratch); (void)hipFree(base);
		if(hbase) (void)hipHostFree(hbase);
		if(e0) (void)hipEventDestroy(e0);
		if(e1) (void)hipEventDestroy(e1);
		return PWN_ENOMEM;
	}
	d.d_scratch = scratch; d.d_base = base; d.h_base = hbase; d.ev_base = e0; d.ev_build = e1;
	return PWN_OK;
}

void pwn_i_spheres_device_release(pwn_ctx *c)
{
	pwn_ctx::spheres_device_state &d = c->sd;
	(void)hipFree(d.d_scratch); (void)hipFree(d.d_base);
	if(d.h_base) (void)hipHostFree(d.h_base);
	if(d.ev_base) (void)hipEventDestroy(d.ev_base);
	if(d.ev_build) (void)hipEventDestroy(d.ev_build);
	memset(&d, 0, sizeof(d));
}

// Room for `need` bytes of the device-memory part in copy nb (pwn_tables.cpp big_reserve without the staging): grown to the largest
// part so far, the device synchronised before a buffer that a launch may still read is freed
int pwn_i_sd_big_reserve(pwn_ctx *c, int nb, size_t need)
{
	if(need > c->big_high) c->big_high = (need + 65535u) & ~(size_t)65535u;
	if(need <= c->d_big_cap[nb]) return PWN_OK;
	uint8_t *p = NULL;
	if(c->d_big[nb] != NULL) HIPCHK(c, hipDeviceSynchronize());
	if(hipMalloc((void **)&p, c->big_high) != hipSuccess) { (void)hipGetLastError(); return PWN_ENOMEM; }
	(void)hipFree(c->d_big[nb]);
	c->d_big[nb] = p; c->d_big_cap[nb] = c->big_high;
	return PWN_OK;
}

// The base copy of the level in force, behind every build that read the one before it
int pwn_i_sd_base(pwn_ctx *c, hipStream_t s)
{
	pwn_ctx::spheres_device_state &d = c->sd;
	if(d.base_ok) return PWN_OK;
	if(d.base_used) HIPCHK(c, hipEventSynchronize(d.ev_base));      // (the pinned slot: once per level)
	uint8_t *b = d.h_base;
	memset(b, 0, PWN_T_BINIDX);
	memcpy(b + PWN_T_RCP, c->tabs, 4096);
	memcpy(b + PWN_T_RSQ, c->tabs + 2048, 4096);
	pwn_fill_faces((float *)(b + PWN_T_FACES));
	memcpy(b + PWN_T_CELLINFO, c->cell_base, sizeof(c->cell_base));
	memcpy(b + PWN_T_EPREC, c->ep_recs, sizeof(c->ep_recs));
	HIPCHK(c, pwn_launch_upload(b, d.d_base, PWN_T_BINIDX, s));
	HIPCHK(c, hipEventRecord(d.ev_base, s));
	d.base_used = true; d.base_ok = true;
	return PWN_OK;
}

extern "C" int pwn_upload_spheres_device(pwn_ctx *c, int n, const void *d_spheres, int max_pairs, void *stream)
{
	GRP_REFUSE(c, "pwn_upload_spheres_device");
	if(c == NULL || n < 0 || n > PWN_OBJ_MAX || max_pairs < 0) return PWN_EINVAL;
	if(n > 0 && (d_spheres == NULL || ((uintptr_t)d_spheres & 15u) != 0)) return PWN_EINVAL;
	const uint64_t big_bytes = pwn_g_total((uint64_t)max_pairs, (uint64_t)n);
	if(big_bytes > PWN_TABLES_MAX) return PWN_ETOOBIG;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	pwn_ctx::spheres_device_state &d = c->sd;
	// (a level whose tables never went up -- a failed upload -- is sent first: the walk table and the baked cell words come with it)
	if(c->blob_dirty && !d.in_force) { rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	rc = pwn_i_sd_buffers(c);
	if(rc != PWN_OK) return rc;
	const int nb = (c->blob_cur + 1) % PWN_NBLOB;
	rc = pwn_i_sd_big_reserve(c, nb, (size_t)big_bytes);
	if(rc != PWN_OK) return rc;

	// from here on the runtime is talked to.  The build before this one shares the scratch and the base copy ...
	if(d.built && d.build_stream != s) HIPCHK(c, hipStreamWaitEvent(s, d.ev_build, 0));
	rc = pwn_i_sd_base(c, s);
	if(rc != PWN_OK) return rc;
	// ... copy nb may still be on its way up, or be read by launches and players' steps: the build waits for them on ITS stream
	if(c->upload_pending[nb]) HIPCHK(c, hipStreamWaitEvent(s, c->ev_upload[nb], 0));
	if(c->tables_in_use[nb]) HIPCHK(c, hipStreamWaitEvent(s, c->tables_wait[nb], 0));
	if(c->walk_in_use[nb]) { HIPCHK(c, hipStreamWaitEvent(s, c->ev_walk[nb], 0)); c->walk_in_use[nb] = false; }
	HIPCHK(c, pwn_launch_sphere_bins(d_spheres, (uint32_t)n, (uint32_t)max_pairs, d.d_scratch, d.d_base, c->d_blob[nb], c->d_big[nb],
		pwn_g_which_offset((uint64_t)max_pairs), pwn_g_sph_offset((uint64_t)max_pairs), s));
	HIPCHK(c, hipEventRecord(d.ev_build, s));
	HIPCHK(c, hipEventRecord(c->ev_upload[nb], s));
	// Uploads from the host run on their own stream and are ordered among themselves by it: they come behind this build too, and
	// with it behind everything it waited for (pwn_i_pack_blob's invariant for the walk tables: what read a buffer is in front of
	// the upload stream).
	HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->ev_upload[nb], 0));

	// the tables in force: what params_tables hands a launch
	c->blob.resize(pwn_t_total_glb(lds_cells(max_pairs)));
	c->off_sph = 0u; c->off_recsph = 0u;
	c->lists_form = PWN_LF_GLOBAL;
	c->big_which = pwn_g_which_offset((uint64_t)max_pairs); c->big_sph = pwn_g_sph_offset((uint64_t)max_pairs);
	c->nbounds = 0;
	c->walk_of[nb] = c->walk_of[c->blob_cur];        // (the walk table is handed on, as by an upload of spheres alone)
	c->upload_pending[nb] = true;
	c->blob_has_static[nb] = true;
	c->blob_cur = nb;
	d.in_force = true; d.built = true; d.build_stream = s;
	d.n = n; d.max_pairs = max_pairs; d.uploads++;
	return PWN_OK;
}

extern "C" int pwn_spheres_device_state(pwn_ctx *c, unsigned long long out[8])
{
	GRP_REFUSE(c, "pwn_spheres_device_state");
	if(c == NULL || out == NULL) return PWN_EINVAL;
	if(c->tiled != NULL) return PWN_EBUSY;
	memset(out, 0, 8 * sizeof(out[0]));
	const pwn_ctx::spheres_device_state &d = c->sd;
	if(!d.built) return PWN_OK;
	(void)hipSetDevice(c->device);
	uint32_t st[8];
	HIPCHK(c, hipEventSynchronize(d.ev_build));
	HIPCHK(c, hipMemcpy(st, d.d_scratch + (size_t)PWN_SD_STATUS_WORD * 4u, sizeof(st), hipMemcpyDeviceToHost));
	out[0] = d.in_force ? 1u : 0u;
	out[1] = (unsigned long long)d.n; out[2] = (unsigned long long)d.max_pairs;
	out[3] = st[PWN_SD_ST_PAIRS]; out[4] = st[PWN_SD_ST_NCELL]; out[5] = st[PWN_SD_ST_LONGEST]; out[6] = st[PWN_SD_ST_REASON];
	out[7] = d.uploads;
	return PWN_OK;
}
