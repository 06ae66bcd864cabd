// level_bake.h -- the per-letter and per-cell rules of a level's tables: level_host.c's is_open / flat_cell / open_dir (how
// pwn_parse_level derives a portal table from the cells), the two rules of pwn_check_portals, the look-through class, half_of_int and
// the baked bits of pwn_bake_cells, as code that the host and the device both compile.  The device's level builder (level_bake.hip)
// and its sequential stand-in (tools/sanitize/fake_kernels.cpp) take them from here; tests/test_level_bake.py compiles them with gcc
// and holds them to level_host.c, which stays the ruler.  Plain C; cell_bake.h is the only other header.
//
// Integer work only.  A portal table is 26 x 7 int32 (pwn_portal: x1 z1 x2 z2 rot12 c1 c2), here as a flat array so that a kernel can
// keep it in LDS.  Nothing below uses a table's value as an index, a loop bound or a shift count: coordinates are COMPARED with cell
// coordinates.  The one exception is pwn_lb_cell_bits' record (differences of coordinates, their half floats), which is defined for
// tables that passed pwn_lb_coords_bad only -- callers bake behind the verdict.
#pragma once
#include <stdint.h>
#include "cell_bake.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PWN_LB_FN __host__ __device__ static inline
#else
#define PWN_LB_FN static inline
#endif

#define PWN_LB_PM_WORDS 7            /* int32 per letter */
enum { PWN_LB_X1 = 0, PWN_LB_Z1, PWN_LB_X2, PWN_LB_Z2, PWN_LB_ROT12, PWN_LB_C1, PWN_LB_C2 };
// the verdict on a table (pwn_level_device_state out[2])
enum { PWN_LB_TAKEN = 0, PWN_LB_BAD_COORD = 1, PWN_LB_BAD_OUTSIDE = 2 };

// a cell a portal can open onto (util.h:128-138)
PWN_LB_FN int pwn_lb_is_open(int c)
{
	return c == ';' || c == '$' || c == '"' || c == '#' || c == '&' || c == '>' || c == '<' || c == '^' || c == ',';
}

// the reference's unguarded lv->data[z][x +- 1] (util.h:140-149): through the flat array, x = 64 aliases the next row; a read that
// would leave the array sees a closed cell
PWN_LB_FN int pwn_lb_flat_cell(const uint8_t *cells, int x, int z)
{
	const int i = z * 64 + x;
	return (i >= 0 && i < 4096) ? cells[i] : '.';
}

PWN_LB_FN int pwn_lb_dir_dx(int d) { return d == 0 ? 1 : (d == 2 ? -1 : 0); }
PWN_LB_FN int pwn_lb_dir_dz(int d) { return d == 1 ? 1 : (d == 3 ? -1 : 0); }

// the first open neighbour in the order +x, +z, -x, -z; none: +x (util.h:147-148).  x, z: a cell of the grid.
PWN_LB_FN int pwn_lb_open_dir(const uint8_t *cells, int x, int z)
{
	for(int d = 0; d < 4; d++)
		if(pwn_lb_is_open(pwn_lb_flat_cell(cells, x + pwn_lb_dir_dx(d), z + pwn_lb_dir_dz(d)))) return d;
	return 0;
}

// One letter's row of the table as pwn_parse_level derives it from the cells as stored: first / second = the cell numbers (z * 64 + x)
// of the letter's first two sightings in scan order, each below 4096, or anything else for "none" (a second without a first is none).
PWN_LB_FN void pwn_lb_derive_letter(const uint8_t *cells, uint32_t first, uint32_t second, int32_t *pm)
{
	const int have1 = first < 4096u, have2 = have1 && second < 4096u;
	pm[PWN_LB_X1] = have1 ? (int32_t)(first & 63u) : -1; pm[PWN_LB_Z1] = have1 ? (int32_t)(first >> 6) : -1;
	pm[PWN_LB_X2] = have2 ? (int32_t)(second & 63u) : -1; pm[PWN_LB_Z2] = have2 ? (int32_t)(second >> 6) : -1;
	pm[PWN_LB_ROT12] = 0; pm[PWN_LB_C1] = ';'; pm[PWN_LB_C2] = ';';
	if(!have2) return;
	// level.h:194-221
	const int d1 = pwn_lb_open_dir(cells, pm[PWN_LB_X1], pm[PWN_LB_Z1]), d2 = pwn_lb_open_dir(cells, pm[PWN_LB_X2], pm[PWN_LB_Z2]);
	pm[PWN_LB_ROT12] = (d2 - d1 + 2) & 3;
	pm[PWN_LB_C1] = pwn_lb_flat_cell(cells, pm[PWN_LB_X1] + pwn_lb_dir_dx(d1), pm[PWN_LB_Z1] + pwn_lb_dir_dz(d1));
	pm[PWN_LB_C2] = pwn_lb_flat_cell(cells, pm[PWN_LB_X2] + pwn_lb_dir_dx(d2), pm[PWN_LB_Z2] + pwn_lb_dir_dz(d2));
}

// the look-through class of a cell type (trace.h:404-413: '#' and '&' carry on, '"' shifts y)
PWN_LB_FN uint32_t pwn_lb_look_class(int c)
{
	if(c == '#' || c == '&') return PWN_C_LT2;
	if(c == '"') return PWN_C_LTDQ;
	return 0u;
}

// pwn_check_portals' first rule, for one letter: a coordinate outside -1 .. 63
PWN_LB_FN int pwn_lb_coords_bad(const int32_t *pm)
{
	int bad = 0;
	for(int k = 0; k < 4; k++) bad |= pm[k] < -1 || pm[k] > 63;
	return bad;
}

// ... its second rule, for one cell outside the grid at coordinate -1 -- (cx, cz) is (-1, t) or (t, -1), t = -1 .. 63: the letter
// (0 .. 25) that stands in the cell read for it and would see or do something there as an endpoint, or -1 (level_host.c
// outside_cell_differs).  pmap: the whole table, indexed by the CELL's letter.
PWN_LB_FN int pwn_lb_outside_letter(const uint8_t *cells, const int32_t *pmap, int cx, int cz)
{
	const int c = cells[(cz < 0 ? 0 : cz) * 64 + (cx < 0 ? 0 : cx)];    /* util.h:151-158 */
	if(c < 'A' || c > 'Z') return -1;
	const int32_t *pm = pmap + PWN_LB_PM_WORDS * (c - 'A');
	const int at1 = pm[PWN_LB_X1] == cx && pm[PWN_LB_Z1] == cz, at2 = pm[PWN_LB_X2] == cx && pm[PWN_LB_Z2] == cz;
	int differs = 0;
	if(at1) differs = pwn_lb_look_class(pm[PWN_LB_C2] & 0xff) != 0u;
	else if(at2) differs = pwn_lb_look_class(pm[PWN_LB_C1] & 0xff) != 0u;
	if(pm[PWN_LB_X2] != -1 && (at1 || at2)) differs = 1;
	return differs ? c - 'A' : -1;
}
// the t-th of those 130 cells, t = 0 .. 129: (-1, t - 1) for t < 65, (t - 66, -1) from there
PWN_LB_FN int pwn_lb_outside_letter_nth(const uint8_t *cells, const int32_t *pmap, int t)
{
	return t < 65 ? pwn_lb_outside_letter(cells, pmap, -1, t - 1) : pwn_lb_outside_letter(cells, pmap, t - 66, -1);
}

// a whole number of magnitude <= 64 as a half float; `neg` gives -0.0 for 0 (level_host.c half_of_int).  Anything larger: not
// defined here, and never asked (the verdict stands in front).
PWN_LB_FN uint32_t pwn_lb_half_of_int(int v, int neg)
{
	const uint32_t m = (uint32_t)(v < 0 ? -v : v), sign = (v < 0 || neg) ? 0x8000u : 0u;
	if(m == 0u) return sign;
	int e = 0;
	while(e < 6 && (m >> e) > 1u) e++;
	return sign | ((uint32_t)(e + 15) << 10) | ((m - (1u << e)) << (10 - e));
}

// is cell (x, z) of the grid, holding c, an endpoint that leads somewhere: a letter's cell at one of its endpoints, the letter paired.
// Such cells get the endpoint records, numbered in scan order.
PWN_LB_FN int pwn_lb_is_endpoint(int c, int x, int z, const int32_t *pmap)
{
	if(c < 'A' || c > 'Z') return 0;
	const int32_t *pm = pmap + PWN_LB_PM_WORDS * (c - 'A');
	const int at1 = pm[PWN_LB_X1] == x && pm[PWN_LB_Z1] == z, at2 = pm[PWN_LB_X2] == x && pm[PWN_LB_Z2] == z;
	return pm[PWN_LB_X2] != -1 && (at1 || at2);
}

// The baked bits of cell (x, z) of the grid, which holds c (level_host.c pwn_bake_cells; cell_bake.h).  rank: the cell's number among
// the endpoint cells in scan order (read only where pwn_lb_is_endpoint).  *inside: the bits of the cell's own word; *outside: those
// of the row / column 64 words that repeat it (x == 0, z == 0), the non-endpoint answers; *rec: the endpoint record, where the cell
// has one (else untouched).  Returns 1 if it has.  Only for tables whose coordinates passed pwn_lb_coords_bad.
PWN_LB_FN int pwn_lb_cell_bits(int c, int x, int z, const int32_t *pmap, uint32_t rank, uint32_t *inside, uint32_t *outside, uint32_t *rec)
{
	uint32_t in = pwn_lb_look_class(c), out = in;
	int has = 0;
	if(c >= 'A' && c <= 'Z')
	{
		const int32_t *pm = pmap + PWN_LB_PM_WORDS * (c - 'A');
		const int at1 = pm[PWN_LB_X1] == x && pm[PWN_LB_Z1] == z, at2 = pm[PWN_LB_X2] == x && pm[PWN_LB_Z2] == z;
		/* trace.h:404-413 */
		if(at1) in = pwn_lb_look_class(pm[PWN_LB_C2] & 0xff);
		else if(at2) in = pwn_lb_look_class(pm[PWN_LB_C1] & 0xff);
		/* trace.h:514-559 */
		uint32_t st = pm[PWN_LB_X2] == -1 ? PWN_PST_WALL : PWN_PST_MAGENTA;
		out |= st << PWN_C_PST_SHIFT;
		if(pm[PWN_LB_X2] != -1 && (at1 || at2))
		{
			const int dx = pm[PWN_LB_X2] - pm[PWN_LB_X1], dz = pm[PWN_LB_Z2] - pm[PWN_LB_Z1];
			*rec = at1 ? pwn_lb_half_of_int(dx, 0) | (pwn_lb_half_of_int(dz, 0) << 16)
			           : pwn_lb_half_of_int(-dx, dx == 0) | (pwn_lb_half_of_int(-dz, dz == 0) << 16);
			in |= ((at1 ? 0u - (uint32_t)pm[PWN_LB_ROT12] : (uint32_t)pm[PWN_LB_ROT12]) & 3u) << PWN_C_PROT_SHIFT;
			st = PWN_PST_REC0 + rank;
			has = 1;
		}
		in |= st << PWN_C_PST_SHIFT;
	}
	*inside = in; *outside = out;
	return has;
}
