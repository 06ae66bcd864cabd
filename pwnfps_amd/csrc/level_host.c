/*
 * level_host.c -- host-side level handling for libpwnhip (plain C).
 *
 *   pwn_parse_level     level_load  (level.h:107-228): the level.txt format
 *   pwn_bin_spheres     level_prepare_render + level_part_add(_bbox)
 *                       (level.h:1-39,64-81): per-cell sphere lists
 *   pwn_check_portals   which hand-made portal tables pwn_upload_level takes
 *   pwn_bake_cells      what the walk's portal arms ask of a cell (trace.h:404-413,
 *                       508-559), decided once per level: cell_bake.h
 *
 *   pwn_sphere_bounds_build   a bounding ball for the longest per-cell lists (sphere_bound.h)
 *
 * All produce flat tables that pwn_tables.cpp packs into the LDS blob.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "level_host.h"

enum { DIR_XP = 0, DIR_ZP, DIR_XN, DIR_ZN };

/* a cell a portal can open onto (util.h:128-138) */
static int is_open(int c)
{
	switch(c)
	{
		case ';': case '$': case '"': case '#': case '&':
		case '>': case '<': case '^': case ',':
			return 1;
	}
	return 0;
}

/* Neighbour lookups go through the flat 4096-byte array exactly like the
   reference's unguarded lv->data[z][x+-1] (util.h:140-149): x = 64 aliases the
   next row.  Reads that would leave the array see a closed cell instead. */
static int flat_cell(const uint8_t *cells, int x, int z)
{
	int i = z * 64 + x;
	return (i >= 0 && i < 4096) ? cells[i] : '.';
}

static const int dir_dx[4] = { 1, 0, -1, 0 };
static const int dir_dz[4] = { 0, 1, 0, -1 };

static int open_dir(const uint8_t *cells, int x, int z)
{
	for(int d = 0; d < 4; d++)
		if(is_open(flat_cell(cells, x + dir_dx[d], z + dir_dz[d])))
			return d;
	return DIR_XP; /* "NOT FREE": the reference falls back to +x (util.h:147-148) */
}

static void endpoint(pwn_portal *pm, int x, int z)
{
	/* level.h:149-160 / 168-177: first two sightings are the endpoints */
	if(pm->x1 == -1) { pm->x1 = x; pm->z1 = z; }
	else if(pm->x2 == -1) { pm->x2 = x; pm->z2 = z; }
}

void pwn_level_clear(uint8_t *cells, pwn_portal *pmap, int32_t *spawn)
{
	/* level_new (level.h:85-105) */
	memset(cells, '.', 4096);
	for(int i = 0; i < 26; i++)
	{
		pmap[i].x1 = pmap[i].z1 = pmap[i].x2 = pmap[i].z2 = -1;
		pmap[i].rot12 = 0;
		pmap[i].c1 = pmap[i].c2 = ';';
	}
	spawn[0] = spawn[1] = 0;
}

int pwn_parse_level(const char *text, int len, uint8_t *cells, pwn_portal *pmap, int32_t *spawn)
{
	if(text == NULL || len < 0) return -1;
	pwn_level_clear(cells, pmap, spawn);

	const unsigned char *p = (const unsigned char *)text, *end = p + len;
	int x = 0, z = 0;
	while(p < end && z < 64)
	{
		int c = *p++;
		if(c == '\r' || c == '\n')
		{
			/* level.h:124-135: a line end at column 0 is swallowed (so CRLF
			   pairs and blank lines vanish); anywhere else it closes the row */
			if(x != 0) { x = 0; z++; }
			continue;
		}
		if(c == '*') { spawn[0] = x; spawn[1] = z; c = ';'; }
		if(c >= 'a' && c < 'z')
		{
			/* level.h:144-161: a lower-case letter is an endpoint of ITS letter
			   and is then stored (and registered again) as the NEXT letter */
			endpoint(&pmap[c - 'a'], x, z);
			c = c - 'a' + 'A' + 1;
		}
		if(c >= 'A' && c <= 'Z') endpoint(&pmap[c - 'A'], x, z);
		cells[z * 64 + x] = (uint8_t)c;
		if(++x == 64) { x = 0; z++; } /* a full row needs no line end (level.h:120) */
	}

	/* level.h:194-221 */
	for(int i = 0; i < 26; i++)
	{
		pwn_portal *pm = &pmap[i];
		if(pm->x2 == -1) continue;
		int d1 = open_dir(cells, pm->x1, pm->z1);
		int d2 = open_dir(cells, pm->x2, pm->z2);
		pm->rot12 = (d2 - d1 + 2) & 3;
		pm->c1 = flat_cell(cells, pm->x1 + dir_dx[d1], pm->z1 + dir_dz[d1]);
		pm->c2 = flat_cell(cells, pm->x2 + dir_dx[d2], pm->z2 + dir_dz[d2]);
	}
	return 0;
}

/* the look-through class of a cell type (trace.h:404-413: '#' and '&' carry on, '"' shifts y) */
static uint32_t look_class(int c)
{
	if(c == '#' || c == '&') return PWN_C_LT2;
	if(c == '"') return PWN_C_LTDQ;
	return 0;
}

/*
 * Which portal tables pwn_upload_level takes (1) and which it refuses (0).  The reference compares a letter's
 * endpoints with the ray's cell as it stands, unclamped (trace.h:404-413, 508-559), while it READS the cell
 * through get_cell's clamp: a ray in cell (-1, 5), outside the grid, reads cell (0, 5) and stands on an endpoint
 * that the table gives as (-1, 5).  -1 is the one coordinate outside the grid that a table can hold: x == -1 says
 * "no endpoint" (level.h:94-99, 149-177), and the z beside it is whatever it was -- level_new sets x1, x2, c1
 * and c2 only, so level_load leaves (x1, z1, -1, 0) or (-1, 0, -1, 0), or a z left over from the level before.
 * The baked table (pwn_bake_cells) gives every cell outside the grid the answers of a non-endpoint.  A table is
 * taken where that is what the reference gives as well:
 *   - every coordinate lies in -1 .. 63 (as before);
 *   - for every cell with a coordinate of -1, (-1, t) and (t, -1), the reference's own tests on the cell it reads
 *     there give what they give for a cell that is no endpoint: looking through sees none of '#', '&', '"'
 *     behind a matching endpoint, and a matching endpoint does not lead anywhere (x2 == -1: a wall either way).
 * level_new and level_load leave c1 = c2 = ';' in every letter without endpoint 2: whatever their z, their tables
 * pass.  What is refused is made by hand: a paired letter with an endpoint at -1 that stands in the row-0 / column-0
 * cell read for it, or a '#', '&', '"' far side behind such an endpoint.
 */
static int outside_cell_differs(const uint8_t *cells, const pwn_portal *pmap, int cx, int cz)
{
	const int c = cells[(cz < 0 ? 0 : cz) * 64 + (cx < 0 ? 0 : cx)];    /* util.h:151-158 */
	if(c < 'A' || c > 'Z') return 0;
	const pwn_portal *pm = &pmap[c - 'A'];
	const int at1 = (pm->x1 == cx && pm->z1 == cz), at2 = (pm->x2 == cx && pm->z2 == cz);
	/* trace.h:404-413: the letter itself is neither 2-high nor a '"' */
	if(at1) { if(look_class(pm->c2 & 0xff) != 0u) return 1; }
	else if(at2) { if(look_class(pm->c1 & 0xff) != 0u) return 1; }
	/* trace.h:514-559: x2 == -1 is a wall before the endpoints are asked */
	return pm->x2 != -1 && (at1 || at2);
}

int pwn_check_portals(const uint8_t *cells, const pwn_portal *pmap)
{
	for(int i = 0; i < 26; i++)
	{
		const int32_t v[4] = { pmap[i].x1, pmap[i].z1, pmap[i].x2, pmap[i].z2 };
		for(int k = 0; k < 4; k++) if(v[k] < -1 || v[k] > 63) return 0;
	}
	/* (no endpoint has a coordinate beyond 63 or below -1: only these cells outside the grid can match one) */
	for(int t = -1; t < 64; t++)
		if(outside_cell_differs(cells, pmap, -1, t) || outside_cell_differs(cells, pmap, t, -1)) return 0;
	return 1;
}

/* a whole number of magnitude <= 64 as a half float; `neg` gives -0.0 for 0 */
static uint32_t half_of_int(int v, int neg)
{
	uint32_t m = (uint32_t)(v < 0 ? -v : v), sign = (v < 0 || neg) ? 0x8000u : 0u;
	if(m == 0) return sign;
	int e = 0;
	while((m >> e) > 1u) e++;
	return sign | ((uint32_t)(e + 15) << 10) | ((m - (1u << e)) << (10 - e));
}

/*
 * The baked bits of every cell word and the endpoint records (cell_bake.h).  bits[65 * 65] in the
 * table's own pitch, row / column 64 included; recs[PWN_EP_MAX].  Returns the number of records
 * used.  The tests on a letter's cell are the reference's, in its order: endpoint 1 before
 * endpoint 2, x2 == -1 only where it goes somewhere.  c1 / c2 are taken as chars (their low byte).
 */
int pwn_bake_cells(const uint8_t *cells, const pwn_portal *pmap, uint16_t *bits, uint32_t *recs)
{
	int nrec = 0;
	memset(bits, 0, 65 * 65 * sizeof(uint16_t));
	memset(recs, 0, PWN_EP_MAX * sizeof(uint32_t));
	for(int z = 0; z < 64; z++)
	for(int x = 0; x < 64; x++)
	{
		const int c = cells[z * 64 + x];
		uint32_t inside = look_class(c), outside = inside;
		if(c >= 'A' && c <= 'Z')
		{
			const pwn_portal *pm = &pmap[c - 'A'];
			const int at1 = (pm->x1 == x && pm->z1 == z), at2 = (pm->x2 == x && pm->z2 == z);
			/* trace.h:404-413 */
			if(at1) inside = look_class(pm->c2 & 0xff);
			else if(at2) inside = look_class(pm->c1 & 0xff);
			/* trace.h:514-559 */
			uint32_t st = pm->x2 == -1 ? PWN_PST_WALL : PWN_PST_MAGENTA;
			outside |= st << PWN_C_PST_SHIFT;
			if(pm->x2 != -1 && (at1 || at2))
			{
				const int dx = pm->x2 - pm->x1, dz = pm->z2 - pm->z1;
				recs[nrec] = at1 ? half_of_int(dx, 0) | (half_of_int(dz, 0) << 16)
				                 : half_of_int(-dx, dx == 0) | (half_of_int(-dz, dz == 0) << 16);
				inside |= ((at1 ? 0u - (uint32_t)pm->rot12 : (uint32_t)pm->rot12) & 3u) << PWN_C_PROT_SHIFT;
				st = PWN_PST_REC0 + (uint32_t)nrec++;
			}
			inside |= st << PWN_C_PST_SHIFT;
		}
		bits[z * 65 + x] = (uint16_t)inside;
		/* what get_cell returns outside the grid on that axis (util.h:151-158): never at an endpoint */
		if(x == 0) bits[z * 65 + 64] = (uint16_t)outside;
		if(z == 0) bits[64 * 65 + x] = (uint16_t)outside;
		if(x == 0 && z == 0) bits[64 * 65 + 64] = (uint16_t)outside;
	}
	return nrec;
}

/*
 * CSR of the per-cell sphere lists.  off[4097]; idx has off[4096] entries.
 * Object order inside a cell = index order, as the reference appends objects
 * in objs[] order (level.h:76-79).  The reference does no bounds check on the
 * bbox cells (level.h:5-17; outside the grid it scribbles over neighbouring
 * memory); cells outside [0,64)^2 are skipped here.
 * Returns the number of entries, or -1 if idx_cap is too small (call with
 * idx = NULL to size).
 */
/* (int)f as the reference's x86 build computes it (cvttss2si: INT_MIN for NaN and anything
   outside int), without the undefined behaviour of the C cast */
static int trunc_to_int(float f)
{
	return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT32_MIN;
}

int pwn_bin_spheres(const pwn_sphere *s, int n, int32_t *off, int32_t *idx, int idx_cap)
{
	int32_t *fill = calloc(4096, sizeof(int32_t));
	if(fill == NULL) return -2;
	memset(off, 0, 4097 * sizeof(int32_t));
	for(int pass = 0; pass < 2; pass++)
	{
		for(int i = 0; i < n; i++)
		{
			/* float subtraction/addition, then truncation toward zero (level.h:27-31) */
			int x1 = trunc_to_int(s[i].x - s[i].r), z1 = trunc_to_int(s[i].z - s[i].r);
			int x2 = trunc_to_int(s[i].x + s[i].r), z2 = trunc_to_int(s[i].z + s[i].r);
			if(x1 < 0) x1 = 0;
			if(z1 < 0) z1 = 0;
			if(x2 > 63) x2 = 63;
			if(z2 > 63) z2 = 63;
			for(int z = z1; z <= z2; z++)
			for(int x = x1; x <= x2; x++)
			{
				int c = z * 64 + x;
				if(pass == 0) off[c + 1]++;
				else idx[off[c] + fill[c]++] = i;
			}
		}
		if(pass == 0)
		{
			for(int c = 0; c < 4096; c++) off[c + 1] += off[c];
			if(idx == NULL) { free(fill); return off[4096]; }
			if(off[4096] > idx_cap) { free(fill); return -1; }
		}
	}
	free(fill);
	return off[4096];
}

/* Bounding balls for the longest per-cell lists (sphere_bound.h has the predicate, the proof and the constants).
   off / idx: the lists as pwn_bin_spheres made them; form: PWN_LF_* of the tables they go into (tables.h: 0 indexed, 1 inline, 2 global), which decides what a list's id is
   (bits 16..30 of its cell's word: tables.h, pwn_i_pack_blob).  The PWN_BOUNDS_MAX lists with the most records are taken, of equally long
   ones the lower cell first, none shorter than PWN_BOUND_MIN_RECORDS; of those a list gets no ball (and no other list takes its
   place) when a member is not finite or far out, or its ball would be large.  Returns how many balls it wrote, longest list first. */
int pwn_sphere_bounds_build(const pwn_sphere *s, const int32_t *off, const int32_t *idx, int form, pwn_sphere_bound *out)
{
	int pick[PWN_BOUNDS_MAX], npick = 0;
	for(int k = 0; k < PWN_BOUNDS_MAX; k++)
	{
		int best = -1, best_n = PWN_BOUND_MIN_RECORDS - 1;
		for(int c = 0; c < 4096; c++)
		{
			const int n = off[c + 1] - off[c];
			if(n <= best_n) continue;
			int taken = 0;
			for(int j = 0; j < npick; j++) taken |= pick[j] == c;
			if(!taken) { best = c; best_n = n; }
		}
		if(best < 0) break;
		pick[npick++] = best;
	}
	int nout = 0;
	for(int k = 0; k < npick; k++)
	{
		const int cell = pick[k], k0 = off[cell], k1 = off[cell + 1], n = k1 - k0;
		/* the list's id in this form: its first entry among the indexed lists (each closed by an end mark), its first record,
		   or its place among the non-empty cells */
		uint32_t id = 0;
		for(int c = 0; c < cell; c++)
		{
			const int m = off[c + 1] - off[c];
			if(m > 0) id += form == 0 ? (uint32_t)m + 1u : (form == 1 ? (uint32_t)m : 1u);
		}
		int ok = 1;
		double mx = 0.0, my = 0.0, mz = 0.0;
		for(int i = k0; i < k1; i++)
		{
			const pwn_sphere *q = &s[idx[i]];
			const double v[4] = { q->x, q->y, q->z, q->r };
			for(int j = 0; j < 4; j++) if(!(fabs(v[j]) <= PWN_SB_COORD_LIMIT)) ok = 0;       /* (NaN and the infinities fail this too) */
			mx += q->x; my += q->y; mz += q->z;
		}
		if(!ok) continue;
		/* the centre the kernel will use: the mean, in fp32 -- the members' distances are taken from THAT point */
		const float cx = (float)(mx / n), cy = (float)(my / n), cz = (float)(mz / n);
		double reff = 0.0;
		for(int i = k0; i < k1; i++)
		{
			const pwn_sphere *q = &s[idx[i]];
			const double dx = (double)q->x - cx, dy = (double)q->y - cy, dz = (double)q->z - cz;
			const double rho = sqrt(dx * dx + dy * dy + dz * dz) * (1.0 + 1e-12), r = fabs((double)q->r);
			if(!(rho + r <= PWN_SB_R_LIMIT)) ok = 0;
			const double a = PWN_SB_D_MAX + rho;
			const double r0 = rho + sqrt(r * r + PWN_SB_EPS_PROOF * a * a + PWN_SB_ETA);
			if(r0 > reff) reff = r0;
		}
		if(!ok) continue;
		/* rounded outwards: R_eff up, RR = R_eff^2 up */
		const float rf = nextafterf((float)(reff * (1.0 + 1.0 / 1048576.0)), INFINITY);
		const float rr = nextafterf((float)((double)rf * (double)rf), INFINITY);
		pwn_sphere_bound *b = &out[nout++];
		b->id = id; b->count = (uint32_t)n; b->cx = cx; b->cy = cy; b->cz = cz; b->rr = rr; b->neg_r = -rf; b->cell = (uint32_t)cell;
	}
	return nout;
}
