// pwn_tables.cpp -- the level, the objects and the sphere tables of a context: the size rules (pwn_i_tables_plan), the blob and its
// device-memory part packed and uploaded through the ring of copies (pwn_i_pack_blob), the entry points that change them.
#include <stdlib.h>
#include <string.h>
#include "pwn_internal.h"
#include "launch_plan.h"
#include "level_host.h"
#include "approx_tables.inc"

// ---- level / spheres --------------------------------------------------------

// RCPPS / RSQRTPS tables in the form the kernels read (dev_math.h, tables.h):
// entry = (1 - exponent offset) << 12 | result mantissa bits 22..11.
// approx_tables.inc entry: bit 12 = exponent offset, bits 11..0 = that mantissa.
void pwn_i_expand_tables(uint16_t *rcp, uint16_t *rsq)
{
	for(int i = 0; i < 2048; i++)
	{
		rcp[i] = (uint16_t)(pwn_host_rcp_tab[i] ^ 0x1000u);
		// kernel index = input bits 23..13: bit 10 = low exponent bit; the generated
		// table is indexed by parity of (e - 127), i.e. with that bit flipped
		rsq[i] = (uint16_t)(pwn_host_rsqrt_tab[i ^ 0x400] ^ 0x1000u);
	}
}

int pwn_i_forced_lists(void)
{
	const char *e = getenv("PWN_SPHERE_LISTS");
	if(e == NULL) return 0;
	return strcmp(e, "indexed") == 0 ? 1 : (strcmp(e, "inline") == 0 ? 2 : (strcmp(e, "global") == 0 ? 3 : 0));
}

// The size rules (pwn_internal.h): pwn_i_pack_blob, pwn_i_bin_spheres, upload_live and pwn_sphere_tables_plan all ask here.
int pwn_i_tables_plan(const int32_t off[4097], uint32_t nsph, int scheduler, int forced, pwn_tables_plan *out)
{
	pwn_tables_plan p;
	memset(&p, 0, sizeof(p));
	p.nsph = nsph;
	// per-cell sphere lists, each closed by PWN_LIST_END in the indexed form; only non-empty cells get one
	uint64_t nbin = 0;
	for(int i = 0; i < 4096; i++)
	{
		const uint32_t cnt = (uint32_t)(off[i + 1] - off[i]);
		if(cnt) { nbin += cnt + 1u; p.ncell++; if(cnt > p.longest) p.longest = cnt; }
	}
	p.nrec = (uint32_t)off[4096];
	p.nbin = (uint32_t)nbin;
	// The forms that live in LDS: list entries are byte offsets (index * 32) in 16 bits, the cell word has 15 bits for a list's
	// start, and the blob is copied whole into every workgroup's LDS.
	const uint32_t total_idx = nbin > 32767u ? 0u : (pwn_t_total(p.nbin, nsph) + 15u) & ~15u;
	const bool in_lds = !(nbin > 32767u || nsph * 32u >= PWN_LIST_END || total_idx > PWN_BLOB_MAX);
	if(in_lds && forced != 3)
	{
		// Which of the two (tables.h): inline sphere records -- one LDS read per test instead of two dependent ones --
		// for the unit scheduler's kernels wherever the bigger blob leaves as many workgroups per CU as the indexed one (launch_plan.h
		// pwn_lds_fit); level.txt 26.5 against 26.3 KB, synth64 30.0 against 28.3 (both five), synth256 32.8 against
		// 30.5 (four against five: indexed).  PWN_SPHERE_LISTS=indexed|inline in the environment forces one (experiments, tests).
		const uint32_t nrec = p.nrec;
		const uint32_t total_inl = (pwn_t_total_inl(nrec, nsph) + 15u) & ~15u;
		const uint32_t extra = pwn_trace_lds_extra();
		const uint32_t fit_idx = pwn_lds_fit(total_idx + extra), fit_inl = pwn_lds_fit(total_inl + extra);
		bool inl = scheduler == PWN_SCHED_UNITS && nrec > 0u && total_inl <= PWN_BLOB_MAX && fit_inl >= (fit_idx < 5u ? fit_idx : 5u);
		if(forced == 1) inl = false;
		if(forced == 2) inl = scheduler == PWN_SCHED_UNITS && nrec > 0u && total_inl <= PWN_BLOB_MAX;
		p.form = inl ? PWN_LF_INLINE : PWN_LF_INDEXED;
		p.blob_bytes = inl ? total_inl : total_idx;
	}
	else
	{
		// The lists in device memory (tables.h): whatever the LDS forms refuse, or PWN_SPHERE_LISTS=global (tests: small scenes
		// through those kernels).  Any scheduler: pwn_i_launch_trace runs the units kernel on such tables.
		p.form = PWN_LF_GLOBAL;
		p.blob_bytes = pwn_t_total_glb(p.ncell);
		p.big_bytes = pwn_g_total(p.nrec, nsph);
	}
	*out = p;
	// (pwnhip.h: the two things that bound tables in device memory -- their bytes, and how long a ray can be held in one cell)
	return (p.big_bytes > PWN_TABLES_MAX || (p.form == PWN_LF_GLOBAL && p.longest > PWN_LIST_MAX)) ? PWN_ETOOBIG : PWN_OK;
}

// Room for `need` bytes of the device-memory part in copy nb of the tables and in staging buffer st.  Buffers grow to the largest
// part so far and never shrink.  A device buffer that grows may still be read by a launch in flight (copy nb's, four uploads
// ago) and is freed here: the device is synchronised first -- on growth only, an upload that fits waits for nothing.  The staging
// buffer is free already (pwn_i_pack_blob has waited for its event).
static int big_reserve(pwn_ctx *c, int nb, unsigned st, size_t need)
{
	if(need > c->big_high) c->big_high = (need + 65535u) & ~(size_t)65535u;
	if(need > c->d_big_cap[nb])
	{
		if(c->d_big[nb] != NULL) { HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(c->d_big[nb]); c->d_big[nb] = NULL; c->d_big_cap[nb] = 0; }
		if(hipMalloc((void **)&c->d_big[nb], c->big_high) != hipSuccess) { (void)hipGetLastError(); c->d_big[nb] = NULL; return PWN_ENOMEM; }
		c->d_big_cap[nb] = c->big_high;
	}
	if(need > c->h_big_cap[st])
	{
		if(c->h_big[st] != NULL) { (void)hipHostFree(c->h_big[st]); c->h_big[st] = NULL; c->h_big_cap[st] = 0; }
		if(hipHostMalloc((void **)&c->h_big[st], c->big_high, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); c->h_big[st] = NULL; return PWN_ENOMEM; }
		c->h_big_cap[st] = c->big_high;
	}
	return PWN_OK;
}

int pwn_i_pack_blob(pwn_ctx *c)
{
	const uint32_t nsph = (uint32_t)c->spheres.size();
	pwn_tables_plan plan;
	{
		const int rc = pwn_i_tables_plan(c->bin_off.data(), nsph, c->scheduler, c->dbg_sphere_lists, &plan);
		if(rc != PWN_OK) return rc;
	}
	const uint32_t nbin = plan.nbin, nrec = plan.nrec;
	const uint32_t total = plan.blob_bytes;
	const bool inl = plan.form == PWN_LF_INLINE, glb = plan.form == PWN_LF_GLOBAL;
	c->blob.assign(total, 0);        // (nothing has changed up to here: a failed call leaves the context as it was)
	uint8_t *b = c->blob.data();
	uint32_t *ci = (uint32_t *)(b + PWN_T_CELLINFO);
	uint16_t *bi = (uint16_t *)(b + PWN_T_BINIDX);
	// the level's part of the cell words (class bits + what the portal arms ask of a cell: cell_bake.h) and the endpoint records are the
	// same until the level or its portal table changes: baked once, the words copied per upload and patched where a cell has spheres
	if(!c->cell_base_ok)
	{
		std::vector<uint16_t> bits(65 * 65);
		pwn_bake_cells(c->cells, c->pmap, bits.data(), c->ep_recs);
		// row / column 64 = what get_cell returns outside the grid on that axis (util.h:151-158),
		// never with spheres (the sphere loop runs for in-grid cells only, trace.h:252)
		for(int z = 0; z <= 64; z++)
		for(int x = 0; x <= 64; x++)
			c->cell_base[z * PWN_GRID_PITCH + x] = (uint32_t)bits[z * PWN_GRID_PITCH + x] | pwn_cell_class(c->cells[(z & 63) * 64 + (x & 63)]);
		c->cell_base_ok = true;
		c->sd.base_ok = false;       // (the device builder's copy of these words is the previous level's: pwn_spheres_device.cpp)
	}
	memcpy(ci, c->cell_base, sizeof(c->cell_base));
	uint32_t at = 0;
	for(int i = 0; i < 4096 && !inl && !glb; i++)
	{
		int32_t k0 = c->bin_off[i], k1 = c->bin_off[i + 1];
		if(k1 > k0)
		{
			ci[(i >> 6) * PWN_GRID_PITCH + (i & 63)] |= PWN_C_SPH | (at << 16);
			for(int32_t k = k0; k < k1; k++) bi[at++] = (uint16_t)(c->bin_idx[k] * 32);
			bi[at++] = (uint16_t)PWN_LIST_END;
		}
	}
	if(inl)
	{
		// records in the lists' order (bin_idx is that order already: cell by cell, object order inside a cell), the last of a cell signed
		float *rec = (float *)(b + PWN_T_BINIDX);
		uint16_t *which = (uint16_t *)(b + pwn_t_recsph_offset(nrec));
		for(int i = 0; i < 4096; i++)
		{
			const int32_t k0 = c->bin_off[i], k1 = c->bin_off[i + 1];
			if(k1 <= k0) continue;
			ci[(i >> 6) * PWN_GRID_PITCH + (i & 63)] |= PWN_C_SPH | ((uint32_t)k0 << 16);
			for(int32_t k = k0; k < k1; k++)
			{
				const pwn_sphere &q = c->spheres[(size_t)c->bin_idx[k]];
				float r2 = q.r * q.r;
				if(r2 < 1.17549435e-38f) r2 = 0.0f;          // (as below: the reference build's flush to zero)
				rec[4 * k + 0] = q.x; rec[4 * k + 1] = q.y; rec[4 * k + 2] = q.z;
				uint32_t wbits;
				memcpy(&wbits, &r2, 4);
				if(k == k1 - 1) wbits |= 0x80000000u;
				memcpy(&rec[4 * k + 3], &wbits, 4);
				which[k] = (uint16_t)(c->bin_idx[k] * 32);
			}
		}
	}
	c->big.clear();
	if(glb)
	{
		// the global form (tables.h): the records are the inline form's, in device memory; LDS gets one u32 per non-empty cell
		c->big.assign((size_t)plan.big_bytes, 0);
		c->big_which = pwn_g_which_offset(nrec); c->big_sph = pwn_g_sph_offset(nrec);
		uint32_t *start = (uint32_t *)(b + PWN_T_BINIDX);
		float *rec = (float *)c->big.data();
		uint32_t *which = (uint32_t *)(c->big.data() + c->big_which);
		uint32_t ord = 0;
		for(int i = 0; i < 4096; i++)
		{
			const int32_t k0 = c->bin_off[i], k1 = c->bin_off[i + 1];
			if(k1 <= k0) continue;
			ci[(i >> 6) * PWN_GRID_PITCH + (i & 63)] |= PWN_C_SPH | (ord << 16);
			start[ord++] = (uint32_t)k0;
			for(int32_t k = k0; k < k1; k++)
			{
				const pwn_sphere &q = c->spheres[(size_t)c->bin_idx[k]];
				float r2 = q.r * q.r;
				if(r2 < 1.17549435e-38f) r2 = 0.0f;          // (as below: the reference build's flush to zero)
				rec[4 * (size_t)k + 0] = q.x; rec[4 * (size_t)k + 1] = q.y; rec[4 * (size_t)k + 2] = q.z;
				uint32_t wbits;
				memcpy(&wbits, &r2, 4);
				if(k == k1 - 1) wbits |= 0x80000000u;
				memcpy(&rec[4 * (size_t)k + 3], &wbits, 4);
				which[k] = (uint32_t)c->bin_idx[k];
			}
		}
	}
	memcpy(b + PWN_T_RCP, c->tabs, 4096);
	memcpy(b + PWN_T_RSQ, c->tabs + 2048, 4096);
	pwn_fill_faces((float *)(b + PWN_T_FACES));
	memcpy(b + PWN_T_EPREC, c->ep_recs, sizeof(c->ep_recs));
	c->off_sph = glb ? 0u : (inl ? pwn_t_sph_offset_inl(nrec) : pwn_t_sph_offset(nbin));
	c->off_recsph = inl ? pwn_t_recsph_offset(nrec) : 0u;
	c->lists_form = plan.form;
	// the balls of the longest lists (sphere_bound.h), with the ids these very tables give the lists: they travel in every launch's
	// arguments (pwn_i_launch_trace)
	static_assert(PWN_LF_INDEXED == 0 && PWN_LF_INLINE == 1 && PWN_LF_GLOBAL == 2, "pwn_sphere_bounds_build takes the form as a number");
	c->nbounds = nsph > 0u ? pwn_sphere_bounds_build(c->spheres.data(), c->bin_off.data(), c->bin_idx.data(), plan.form, c->bounds) : 0;
	// the kernels' layout of a sphere (tables.h): position and r*r in one 16-byte half, the rest in the other
	{
		float *sp = glb ? (float *)(c->big.data() + c->big_sph) : (float *)(b + c->off_sph);
		for(uint32_t i = 0; i < nsph; i++, sp += 8)
		{
			const pwn_sphere &q = c->spheres[i];
			float r2 = q.r * q.r;                 // trace.h:262 `rad*rad`, one fp32 multiply
			if(r2 < 1.17549435e-38f) r2 = 0.0f;   // ... whose result the device flushes like the reference build (FTZ)
			sp[0] = q.x; sp[1] = q.y; sp[2] = q.z; sp[3] = r2;
			sp[4] = q.refl; sp[5] = q.cb; sp[6] = q.cg; sp[7] = q.cr;
		}
	}

	// Upload into the copy no launch in flight reads.  The rcp / rsqrt head of the blob never
	// changes: once a copy has it, only [cellinfo, end) travels (cell words carry the sphere-list
	// offsets, so they change with the spheres).  Nothing here blocks on the GPU except re-use
	// of a staging buffer that is still being read, four uploads later.
	const int nb = (c->blob_cur + 1) % PWN_NBLOB;
	const uint32_t from = c->blob_has_static[nb] ? PWN_T_CELLINFO : 0u;
	const unsigned st = c->stage_next++ % PWN_NSTAGE;
	if(c->stage_used[st]) HIPCHK(c, hipEventSynchronize(c->ev_stage[st]));
	memcpy(c->h_stage[st], b + from, total - from);
	// the global form: the device-memory part travels with the same upload -- the same copy number, staging slot, stream and events
	if(glb)
	{
		const int rc = big_reserve(c, nb, st, c->big.size());
		if(rc != PWN_OK) return rc;
		memcpy(c->h_big[st], c->big.data(), c->big.size());
	}
	// launches still reading that copy (two uploads ago) finish first -- a wait between streams
	if(c->tables_in_use[nb]) HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->tables_wait[nb], 0));
	if(c->walk_in_use[nb]) { HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->ev_walk[nb], 0)); c->walk_in_use[nb] = false; }      // ... and the players' steps that read it
	// (a kernel that reads the pinned buffer, not a DMA copy: see pwn_upload_kernel; total and from are multiples of 16)
	HIPCHK(c, pwn_launch_upload(c->h_stage[st], c->d_blob[nb] + from, total - from, c->up_stream));
	if(glb) HIPCHK(c, pwn_launch_upload(c->h_big[st], c->d_big[nb], c->big.size(), c->up_stream));
	// The walk table of the players' step (tables.h pwn_walk_table; pwn_internal.h d_walk).  A new level: into a buffer that no
	// other copy of the tables refers to (of four buffers the other three copies leave one free; what read it did so through a copy
	// whose later upload, earlier on this stream, waited for it, or through copy nb).  Spheres alone: the copy made current takes
	// the current copy's buffer over, and nothing travels.
	if(c->walk_dirty)
	{
		// INVARIANT: a buffer no OTHER copy refers to is safe to fill behind what this upload has waited for.  Its readers read it
		// through copy nb (waited for above: ev_walk[nb]), or through a copy j whose reference has since changed -- by an upload into
		// j, which waited for ev_walk[j] earlier on this same stream -- and a step on a second stream put this stream behind the
		// record it replaced (pwn_players.cpp step_launch).  So everything that read the buffer is in front of us on up_stream.
		int wb = 0;
		for(; wb < PWN_NBLOB - 1; wb++)
		{
			bool taken = false;
			for(int i = 0; i < PWN_NBLOB; i++) if(i != nb && c->walk_of[i] == wb) taken = true;
			if(!taken) break;
		}
		pwn_walk_table *hw = c->h_walk[st];
		memset(hw, 0, sizeof(*hw));
		memcpy(hw->cells, c->cells, 4096);
		for(int i = 0; i < 26; i++)
		{
			const pwn_portal &q = c->pmap[i];
			const int32_t v[7] = { q.x1, q.z1, q.x2, q.z2, q.rot12, q.c1, q.c2 };
			memcpy(hw->pmap + 7 * i, v, sizeof(v));
		}
		HIPCHK(c, pwn_launch_upload(hw, c->d_walk[wb], sizeof(*hw), c->up_stream));
		c->walk_of[nb] = wb;
		c->walk_dirty = false;
	}
	else c->walk_of[nb] = c->walk_of[c->blob_cur];
	HIPCHK(c, hipEventRecord(c->ev_stage[st], c->up_stream));
	HIPCHK(c, hipEventRecord(c->ev_upload[nb], c->up_stream));
	c->stage_used[st] = true;
	c->upload_pending[nb] = true;
	c->blob_has_static[nb] = true;
	c->blob_cur = nb;
	c->blob_dirty = false;
	c->sd.in_force = false;          // the tables in force are the host's again (pwn_upload_spheres_device)
	// ... and so is the level (pwn_upload_level_device), whose bake has overwritten the device builder's base copy.  The walk table went
	// up with this very upload: such a call leaves walk_dirty set.
	if(c->ld.in_force) { c->ld.in_force = false; c->sd.base_ok = false; }
	return PWN_OK;
}

extern "C" int pwn_upload_level(pwn_ctx *c, const uint8_t data[4096], const pwn_portal pmap[26])
{
	if(GRP_HEAD(c)) return (data == NULL || pmap == NULL) ? PWN_EINVAL : pwn_group_upload_level(c, data, pmap);
	if(c == NULL || data == NULL || pmap == NULL || !pwn_check_portals(data, pmap)) return PWN_EINVAL;      // (which tables: level_host.c)
	(void)hipSetDevice(c->device);
	memcpy(c->cells, data, 4096);
	memcpy(c->pmap, pmap, sizeof(c->pmap));
	c->have_level = true;
	c->cell_base_ok = false;
	c->walk_dirty = true;
	c->blob_dirty = true;
	return pwn_i_pack_blob(c);
}

extern "C" int pwn_level_load_mem(pwn_ctx *c, const char *text, int len)
{
	if(GRP_HEAD(c)) return (text == NULL || len < 0) ? PWN_EINVAL : pwn_group_level_mem(c, text, len);
	if(c == NULL || text == NULL || len < 0) return PWN_EINVAL;
	(void)hipSetDevice(c->device);
	if(pwn_parse_level(text, len, c->cells, c->pmap, c->spawn) != 0) return PWN_EINVAL;
	c->have_level = true;
	c->cell_base_ok = false;
	c->walk_dirty = true;
	c->blob_dirty = true;
	return pwn_i_pack_blob(c);
}

extern "C" int pwn_level_load(pwn_ctx *c, const char *path)
{
	if(c == NULL || path == NULL) return PWN_EINVAL;
	FILE *fp = fopen(path, "rb");
	if(fp == NULL) { snprintf(c->err, sizeof(c->err), "cannot open %s", path); return PWN_EIO; }
	std::vector<char> buf(1 << 20);
	size_t n = fread(buf.data(), 1, buf.size(), fp);
	fclose(fp);
	return pwn_level_load_mem(c, buf.data(), (int)n);
}

extern "C" int pwn_get_level(pwn_ctx *c, uint8_t data[4096], pwn_portal pmap[26], int32_t spawn[2])
{
	if(GRP_HEAD(c)) return pwn_get_level(GRP_M0(c), data, pmap, spawn);
	if(c == NULL) return PWN_EINVAL;
	if(data) memcpy(data, c->cells, 4096);
	if(pmap) memcpy(pmap, c->pmap, sizeof(c->pmap));
	if(spawn) { spawn[0] = c->spawn[0]; spawn[1] = c->spawn[1]; }
	return PWN_OK;
}

enum { OBJ_INVAL = 0, OBJ_FREE = 1, OBJ_SPHERE = 2 };   // defs.h:55-60

// level_prepare_render's binning + upload for a compact list of live spheres
static int upload_live(pwn_ctx *c, const pwn_sphere *s, int n);

extern "C" int pwn_upload_spheres(pwn_ctx *c, const pwn_sphere *s, int n)
{
	if(GRP_HEAD(c)) return (n < 0 || n > PWN_OBJ_MAX || (n > 0 && s == NULL)) ? PWN_EINVAL : pwn_group_upload_spheres(c, s, n);
	if(c == NULL || n < 0 || n > PWN_OBJ_MAX || (n > 0 && s == NULL)) return PWN_EINVAL;
	int rc = upload_live(c, s, n);
	if(rc == PWN_OK)
	{
		c->objs.assign(s, s + n);
		c->obj_typ.assign((size_t)n, OBJ_SPHERE);
	}
	return rc;
}

extern "C" int pwn_obj_new(pwn_ctx *c)
{
	if(GRP_HEAD(c)) { const int r = pwn_obj_new(GRP_M0(c)); if(r < 0) snprintf(c->err, sizeof(c->err), "%s", GRP_M0(c)->err); return r; }
	if(c == NULL) return PWN_EINVAL;
	for(size_t i = 0; i < c->obj_typ.size(); i++)
		if(c->obj_typ[i] == OBJ_FREE) { c->obj_typ[i] = OBJ_INVAL; return (int)i; }
	if(c->obj_typ.size() >= (size_t)PWN_OBJ_MAX)
	{
		snprintf(c->err, sizeof(c->err), "obj_new: all %d object slots are taken", PWN_OBJ_MAX);
		return PWN_ENOMEM;
	}
	c->objs.push_back(pwn_sphere());
	c->obj_typ.push_back(OBJ_INVAL);
	return (int)c->obj_typ.size() - 1;
}

// A handle is the index of a slot that level_obj_new once handed out.  Like the reference's
// part pointers it stays usable after obj_free: obj_set on a freed slot makes it a sphere again
// (script.h:24 sets pt->typ whatever it was), obj_free on it is a no-op (script.h:48).
static bool obj_ok(pwn_ctx *c, int obj, const char *who)
{
	if(c == NULL) return false;
	if(obj >= 0 && (size_t)obj < c->obj_typ.size()) return true;
	snprintf(c->err, sizeof(c->err), "%s: %d is not an object", who, obj);
	return false;
}

extern "C" int pwn_obj_set_sphere(pwn_ctx *c, int obj, double r, double refl, double x, double y, double z,
	double cb, double cg, double cr)
{
	if(GRP_HEAD(c)) { const int q = pwn_obj_set_sphere(GRP_M0(c), obj, r, refl, x, y, z, cb, cg, cr); if(q < 0) snprintf(c->err, sizeof(c->err), "%s", GRP_M0(c)->err); return q; }
	if(!obj_ok(c, obj, "obj_set")) return PWN_EINVAL;
	pwn_sphere &s = c->objs[(size_t)obj];
	s.r = (float)r; s.refl = (float)refl;
	s.x = (float)x; s.y = (float)y; s.z = (float)z;
	s.cb = (float)cb; s.cg = (float)cg; s.cr = (float)cr;
	c->obj_typ[(size_t)obj] = OBJ_SPHERE;
	return PWN_OK;
}

extern "C" int pwn_obj_free(pwn_ctx *c, int obj)
{
	if(GRP_HEAD(c)) { const int q = pwn_obj_free(GRP_M0(c), obj); if(q < 0) snprintf(c->err, sizeof(c->err), "%s", GRP_M0(c)->err); return q; }
	if(!obj_ok(c, obj, "obj_free")) return PWN_EINVAL;
	c->obj_typ[(size_t)obj] = OBJ_FREE;
	return PWN_OK;
}

extern "C" int pwn_level_get(pwn_ctx *c, int cx, int cz)
{
	if(GRP_HEAD(c)) return pwn_level_get(GRP_M0(c), cx, cz);
	if(c == NULL) return PWN_EINVAL;
	if(!c->have_level) return PWN_ENOLEVEL;
	if(cx < 0 || cx >= 64) cx = 0;
	if(cz < 0 || cz >= 64) cz = 0;
	return c->cells[cz * 64 + cx];
}

static int live_objects(pwn_ctx *c, std::vector<pwn_sphere> &live)
{
	for(size_t i = 0; i < c->obj_typ.size(); i++)
	{
		if(c->obj_typ[i] == OBJ_FREE) continue;
		if(c->obj_typ[i] != OBJ_SPHERE)
		{
			snprintf(c->err, sizeof(c->err), "object %d was created but never set", (int)i);
			return PWN_EINVAL;
		}
		live.push_back(c->objs[i]);
	}
	return PWN_OK;
}

extern "C" int pwn_prepare_render(pwn_ctx *c)
{
	if(GRP_HEAD(c)) return pwn_group_prepare_render(c);
	if(c == NULL) return PWN_EINVAL;
	std::vector<pwn_sphere> live;
	int rc = live_objects(c, live);
	if(rc != PWN_OK) return rc;
	return upload_live(c, live.data(), (int)live.size());
}

extern "C" int pwn_get_objects(pwn_ctx *c, pwn_sphere *out, int cap)
{
	if(GRP_HEAD(c)) { const int q = pwn_get_objects(GRP_M0(c), out, cap); if(q < 0) snprintf(c->err, sizeof(c->err), "%s", GRP_M0(c)->err); return q; }
	if(c == NULL || cap < 0 || (cap > 0 && out == NULL)) return PWN_EINVAL;
	std::vector<pwn_sphere> live;
	int rc = live_objects(c, live);
	if(rc != PWN_OK) return rc;
	for(size_t i = 0; i < live.size() && i < (size_t)cap; i++) out[i] = live[i];
	return (int)live.size();
}

// Which handle each live sphere came from, in live_objects' order: the order of the table the kernels read, so pwn_hit.object indexes it
extern "C" int pwn_get_object_ids(pwn_ctx *c, int *ids, int cap)
{
	if(GRP_HEAD(c)) { const int q = pwn_get_object_ids(GRP_M0(c), ids, cap); if(q < 0) snprintf(c->err, sizeof(c->err), "%s", GRP_M0(c)->err); return q; }
	if(c == NULL || cap < 0 || (cap > 0 && ids == NULL)) return PWN_EINVAL;
	int n = 0;
	for(size_t i = 0; i < c->obj_typ.size(); i++)
	{
		if(c->obj_typ[i] == OBJ_FREE) continue;
		if(c->obj_typ[i] != OBJ_SPHERE)
		{
			snprintf(c->err, sizeof(c->err), "object %d was created but never set", (int)i);
			return PWN_EINVAL;
		}
		if(n < cap) ids[n] = (int)i;
		n++;
	}
	return n;
}

// (a group, pwn_group.cpp: the list is binned once and every member uploads it)
int pwn_i_bin_spheres(const pwn_sphere *s, int n, pwn_binned *out)
{
	out->off.assign(4097, 0);
	const int nb = pwn_bin_spheres(s, n, out->off.data(), NULL, 0);
	if(nb < 0) return PWN_ENOMEM;
	// what pwn_i_pack_blob would refuse (no scheduler or forced form changes that), before the lists themselves are made
	pwn_tables_plan plan;
	if(pwn_i_tables_plan(out->off.data(), (uint32_t)n, PWN_SCHED_DEFAULT, 0, &plan) != PWN_OK) return PWN_ETOOBIG;
	out->idx.assign((size_t)(nb > 0 ? nb : 1), 0);
	if(pwn_bin_spheres(s, n, out->off.data(), out->idx.data(), nb) != nb) return PWN_ENOMEM;
	out->s.assign(s, s + n);
	return PWN_OK;
}

int pwn_i_upload_binned(pwn_ctx *c, const pwn_binned &b)
{
	(void)hipSetDevice(c->device);
	c->spheres = b.s; c->bin_off = b.off; c->bin_idx = b.idx;
	c->blob_dirty = true;
	return pwn_i_pack_blob(c);
}

void pwn_i_set_object_table(pwn_ctx *c, const pwn_sphere *s, int n)
{
	c->objs.assign(s, s + n);
	c->obj_typ.assign((size_t)n, OBJ_SPHERE);
}

static int upload_live(pwn_ctx *c, const pwn_sphere *s, int n)
{
	(void)hipSetDevice(c->device);
	std::vector<int32_t> off(4097, 0);
	int nb = pwn_bin_spheres(s, n, off.data(), NULL, 0);
	if(nb < 0) return PWN_ENOMEM;
	// (tables that no form holds are refused on their size alone: a sphere's box may cover every cell)
	{
		pwn_tables_plan plan;
		const int rc = pwn_i_tables_plan(off.data(), (uint32_t)n, c->scheduler, c->dbg_sphere_lists, &plan);
		if(rc != PWN_OK) return rc;
	}
	std::vector<int32_t> idx((size_t)(nb > 0 ? nb : 1));
	if(pwn_bin_spheres(s, n, off.data(), idx.data(), nb) != nb) return PWN_ENOMEM;
	std::vector<pwn_sphere> keep_s(c->spheres);
	std::vector<int32_t> keep_o(c->bin_off), keep_i(c->bin_idx);
	c->spheres.assign(s, s + n);
	c->bin_off.swap(off);
	c->bin_idx.swap(idx);
	c->blob_dirty = true;
	int rc = pwn_i_pack_blob(c);
	if(rc != PWN_OK)
	{
		// keep the previous, working set
		c->spheres.swap(keep_s); c->bin_off.swap(keep_o); c->bin_idx.swap(keep_i);
		// too big: pwn_i_pack_blob gave up before it changed anything; a failed upload is tried again
		if(rc == PWN_ETOOBIG) c->blob_dirty = false; else (void)pwn_i_pack_blob(c);
	}
	return rc;
}

extern "C" int pwn_get_bins(pwn_ctx *c, uint16_t counts[4096], int32_t *idx, int cap)
{
	if(GRP_HEAD(c)) { const int rc = pwn_group_sync(c); return rc != PWN_OK ? rc : pwn_get_bins(GRP_M0(c), counts, idx, cap); }      // (the lists are the members' threads' work)
	if(c == NULL || counts == NULL) return PWN_EINVAL;
	for(int i = 0; i < 4096; i++) counts[i] = (uint16_t)(c->bin_off[i + 1] - c->bin_off[i]);
	int n = c->bin_off[4096];
	if(idx != NULL)
	{
		if(n > cap) return PWN_EINVAL;
		for(int i = 0; i < n; i++) idx[i] = c->bin_idx[i];
	}
	return n;
}

static void plan_out(const pwn_tables_plan &p, unsigned long long out[6])
{
	out[0] = (unsigned long long)p.form;
	out[1] = (unsigned long long)p.blob_bytes + pwn_trace_lds_extra();
	out[2] = p.big_bytes;
	out[3] = p.nrec; out[4] = p.ncell; out[5] = p.longest;
}

extern "C" int pwn_sphere_tables_plan(const pwn_sphere *s, int n, unsigned long long out[6])
{
	if(out == NULL || n < 0 || n > PWN_OBJ_MAX || s == NULL) return PWN_EINVAL;
	std::vector<int32_t> off(4097, 0);
	if(pwn_bin_spheres(s, n, off.data(), NULL, 0) < 0) return PWN_ENOMEM;
	pwn_tables_plan p;
	const int rc = pwn_i_tables_plan(off.data(), (uint32_t)n, PWN_SCHED_DEFAULT, pwn_i_forced_lists(), &p);
	plan_out(p, out);
	return rc;
}

extern "C" int pwn_sphere_bounds_plan(const pwn_sphere *s, int n, double out[PWN_BOUNDS_MAX][8])
{
	if(out == NULL || n < 0 || n > PWN_OBJ_MAX || s == NULL) return PWN_EINVAL;
	std::vector<int32_t> off(4097, 0);
	const int nb = pwn_bin_spheres(s, n, off.data(), NULL, 0);
	if(nb < 0) return PWN_ENOMEM;
	pwn_tables_plan p;
	const int rc = pwn_i_tables_plan(off.data(), (uint32_t)n, PWN_SCHED_DEFAULT, pwn_i_forced_lists(), &p);
	if(rc != PWN_OK) return rc;
	std::vector<int32_t> idx((size_t)(nb > 0 ? nb : 1));
	if(pwn_bin_spheres(s, n, off.data(), idx.data(), nb) != nb) return PWN_ENOMEM;
	pwn_sphere_bound b[PWN_BOUNDS_MAX];
	const int k = n > 0 ? pwn_sphere_bounds_build(s, off.data(), idx.data(), p.form, b) : 0;
	memset(out, 0, sizeof(double) * PWN_BOUNDS_MAX * 8);
	for(int i = 0; i < k; i++)
	{
		double *o = out[i];
		o[0] = (double)b[i].cell; o[1] = (double)b[i].count; o[2] = (double)b[i].id;
		o[3] = b[i].cx; o[4] = b[i].cy; o[5] = b[i].cz; o[6] = -(double)b[i].neg_r; o[7] = b[i].rr;
	}
	return k;
}

extern "C" int pwn_sphere_tables_state(pwn_ctx *c, unsigned long long out[6])
{
	if(GRP_HEAD(c)) { const int rc = pwn_group_sync(c); return rc != PWN_OK ? rc : pwn_sphere_tables_state(GRP_M0(c), out); }      // (as pwn_get_bins)
	if(c == NULL || out == NULL) return PWN_EINVAL;
	// tables built on the device (pwn_upload_spheres_device): the host knows their capacity, not their lists
	if(c->sd.in_force)
	{
		const uint64_t mp = (uint64_t)c->sd.max_pairs;
		out[0] = PWN_LF_GLOBAL;
		out[1] = (unsigned long long)c->blob.size() + pwn_trace_lds_extra();
		out[2] = pwn_g_total(mp, (uint64_t)c->sd.n);
		out[3] = mp; out[4] = mp < 4096u ? mp : 4096u; out[5] = mp < (uint64_t)PWN_LIST_MAX ? mp : (uint64_t)PWN_LIST_MAX;
		return PWN_OK;
	}
	// (the lists in force are the context's bins: a refused upload has put the previous ones back)
	pwn_tables_plan p;
	const int rc = pwn_i_tables_plan(c->bin_off.data(), (uint32_t)c->spheres.size(), c->scheduler, c->dbg_sphere_lists, &p);
	plan_out(p, out);
	return rc;
}
