// pwn_level_device.cpp -- pwn_upload_level_device: the level's part of the tables baked on the device (level_bake.hip) from a grid and
// a portal table that are already there, on the caller's stream: into the device builder's base copy (pwn_spheres_device.cpp) and a
// walk table no other copy of the tables refers to, then sphere-less tables from that base copy into the next copy of the ring, as
// pwn_upload_spheres_device builds them for n = 0.  FIVE launches and no host wait: one of the bake, four of the build; in a context's
// first device build one more, which brings the static head of the tables into the base copy.  pwn_level_device_state reads the last
// bake's status words back, pwn_get_level_device the walk table of a device-built level in force.
#include <string.h>
#include "pwn_internal.h"

static int ld_buffers(pwn_ctx *c)
{
	pwn_ctx::level_device_state &l = c->ld;
	if(l.d_status != NULL) return PWN_OK;
	uint32_t *st = NULL;
	hipEvent_t e = NULL;
	if(hipMalloc((void **)&st, PWN_LD_STATUS_WORDS * 4u) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
	{
		(void)hipGetLastError();
		(void)hipFree(st);
		return PWN_ENOMEM;
	}
	l.d_status = st; l.ev_order = e;
	return PWN_OK;
}

void pwn_i_level_device_release(pwn_ctx *c)
{
	pwn_ctx::level_device_state &l = c->ld;
	(void)hipFree(l.d_status);
	if(l.ev_order) (void)hipEventDestroy(l.ev_order);
	memset(&l, 0, sizeof(l));
}

extern "C" int pwn_upload_level_device(pwn_ctx *c, const void *d_data, const void *d_pmap, void *stream)
{
	GRP_REFUSE(c, "pwn_upload_level_device");
	if(c == NULL || d_data == NULL || (((uintptr_t)d_data | (uintptr_t)d_pmap) & 15u) != 0) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	pwn_ctx::spheres_device_state &d = c->sd;
	pwn_ctx::level_device_state &l = c->ld;
	// (a level whose tables never went up -- a failed upload -- is sent first: a refused table leaves THAT level in force)
	if(c->blob_dirty && !d.in_force) { rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	rc = pwn_i_sd_buffers(c);
	if(rc == PWN_OK) rc = ld_buffers(c);
	if(rc != PWN_OK) return rc;
	const int nb = (c->blob_cur + 1) % PWN_NBLOB;
	rc = pwn_i_sd_big_reserve(c, nb, (size_t)pwn_g_total(0u, 0u));
	if(rc != PWN_OK) return rc;

	// from here on the runtime is talked to.  The bake writes the base copy and the status words, which the build before this one --
	// of spheres or of a level -- reads or writes: behind it where the stream differs ...
	if(d.built && d.build_stream != s) HIPCHK(c, hipStreamWaitEvent(s, d.ev_build, 0));
	// ... and the base copy is there: the host's level unless a device-built one has replaced it (base_ok).  A refused table leaves it so.
	rc = pwn_i_sd_base(c, s);
	if(rc != PWN_OK) return rc;
	// copy nb may still be on its way up, or be read by launches and players' steps: waited for on THIS stream, as a device build does
	if(c->upload_pending[nb]) HIPCHK(c, hipStreamWaitEvent(s, c->ev_upload[nb], 0));
	if(c->tables_in_use[nb]) HIPCHK(c, hipStreamWaitEvent(s, c->tables_wait[nb], 0));
	if(c->walk_in_use[nb]) { HIPCHK(c, hipStreamWaitEvent(s, c->ev_walk[nb], 0)); c->walk_in_use[nb] = false; }
	// The walk buffer: one that no OTHER copy refers to, as pwn_i_pack_blob picks it.  What read it did so through copy nb (waited for
	// above), or through a copy whose reference has since changed -- by a host upload, which waited for that copy's steps on the
	// upload stream, or by a device build, which waited for them on its stream and put the upload stream behind itself; and a step
	// on a second stream put the upload stream behind the record it replaced (pwn_players.cpp).  So the upload stream is behind every
	// reader of the buffer, and this stream goes behind the upload stream as it stands now.
	int wb = 0;
	for(; wb < PWN_NBLOB - 1; wb++)
	{
		bool taken = false;
		for(int i = 0; i < PWN_NBLOB; i++) if(i != nb && c->walk_of[i] == wb) taken = true;
		if(!taken) break;
	}
	HIPCHK(c, hipEventRecord(l.ev_order, c->up_stream));
	HIPCHK(c, hipStreamWaitEvent(s, l.ev_order, 0));
	HIPCHK(c, pwn_launch_level_bake(d_data, d_pmap, d.d_base, c->d_walk[wb], c->d_walk[c->walk_of[c->blob_cur]], l.d_status, l.in_force ? 1 : 0, s));
	HIPCHK(c, pwn_launch_sphere_bins(NULL, 0u, 0u, d.d_scratch, d.d_base, c->d_blob[nb], c->d_big[nb], pwn_g_which_offset(0u), pwn_g_sph_offset(0u), s));
	HIPCHK(c, hipEventRecord(d.ev_build, s));
	HIPCHK(c, hipEventRecord(c->ev_upload[nb], s));
	// (uploads from the host come behind this build, and with it behind everything it waited for: pwn_upload_spheres_device)
	HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->ev_upload[nb], 0));

	// the tables in force: those of pwn_upload_spheres_device(n = 0, max_pairs = 0)
	c->blob.resize(pwn_t_total_glb(0u));
	c->off_sph = 0u; c->off_recsph = 0u;
	c->lists_form = PWN_LF_GLOBAL;
	c->big_which = pwn_g_which_offset(0u); c->big_sph = pwn_g_sph_offset(0u);
	c->nbounds = 0;
	c->walk_of[nb] = wb;
	c->walk_dirty = true;            // (the host's next upload sends the HOST's walk table again, whatever this bake decided)
	c->upload_pending[nb] = true;
	c->blob_has_static[nb] = true;
	c->blob_cur = nb;
	d.in_force = true; d.built = true; d.build_stream = s;
	d.n = 0; d.max_pairs = 0;
	l.in_force = true; l.built = true; l.uploads++;
	return PWN_OK;
}

// the last bake's status words, behind the last build of either kind (which is behind the bake)
static int ld_status(pwn_ctx *c, uint32_t st[PWN_LD_STATUS_WORDS])
{
	(void)hipSetDevice(c->device);
	HIPCHK(c, hipEventSynchronize(c->sd.ev_build));
	HIPCHK(c, hipMemcpy(st, c->ld.d_status, PWN_LD_STATUS_WORDS * 4u, hipMemcpyDeviceToHost));
	return PWN_OK;
}

extern "C" int pwn_level_device_state(pwn_ctx *c, unsigned long long out[8])
{
	GRP_REFUSE(c, "pwn_level_device_state");
	if(c == NULL || out == NULL) return PWN_EINVAL;
	if(c->tiled != NULL) return PWN_EBUSY;
	memset(out, 0, 8 * sizeof(out[0]));
	const pwn_ctx::level_device_state &l = c->ld;
	if(!l.built) return PWN_OK;
	uint32_t st[PWN_LD_STATUS_WORDS];
	const int rc = ld_status(c, st);
	if(rc != PWN_OK) return rc;
	out[0] = (l.in_force && st[PWN_LD_ST_DEV] != 0u) ? 1u : 0u;
	out[1] = l.uploads;
	out[2] = st[PWN_LD_ST_VERDICT]; out[3] = st[PWN_LD_ST_LETTER]; out[4] = st[PWN_LD_ST_RECS]; out[5] = st[PWN_LD_ST_PAIRED];
	out[6] = st[PWN_LD_ST_DERIVED];
	return PWN_OK;
}

extern "C" int pwn_get_level_device(pwn_ctx *c, uint8_t data[4096], pwn_portal pmap[26])
{
	GRP_REFUSE(c, "pwn_get_level_device");
	if(c == NULL) return PWN_EINVAL;
	if(c->tiled != NULL) return PWN_EBUSY;
	const pwn_ctx::level_device_state &l = c->ld;
	if(!l.in_force) return PWN_EINVAL;
	uint32_t st[PWN_LD_STATUS_WORDS];
	const int rc = ld_status(c, st);
	if(rc != PWN_OK) return rc;
	if(st[PWN_LD_ST_DEV] == 0u) return PWN_EINVAL;
	static_assert(sizeof(pwn_portal) == 7 * sizeof(int32_t), "the walk table holds the portal table as it is");
	const pwn_walk_table *w = c->d_walk[c->walk_of[c->blob_cur]];
	if(data) HIPCHK(c, hipMemcpy(data, w->cells, 4096, hipMemcpyDeviceToHost));
	if(pmap) HIPCHK(c, hipMemcpy(pmap, w->pmap, 26 * sizeof(pwn_portal), hipMemcpyDeviceToHost));
	return PWN_OK;
}
