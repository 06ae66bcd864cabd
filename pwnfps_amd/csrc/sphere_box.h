// sphere_box.h -- which cells a sphere is binned to, and its r*r as the tables hold it: the arithmetic of level_host.c's
// pwn_bin_spheres (level.h:27-31, 64-81) and of pwn_i_pack_blob's sphere records, as code that the host and the device both compile.
// The device's table builder (sphere_bins.hip) takes it from here; tests/test_sphere_box.py compiles it with gcc and holds it to
// pwn_bin_spheres.  Plain C, no other header of the library.
//
// Floating point: one fp32 subtraction or sum per box edge and one fp32 product for r*r, each rounded by itself, denormals KEPT --
// what level_host.c and pwn_tables.cpp compile to on the host (-ffp-contract=off, the default MXCSR).  The flush of r*r is the
// explicit comparison below, not a mode.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PWN_BOX_FN __host__ __device__ static inline
#else
#define PWN_BOX_FN static inline
#endif

// (int)f as the reference's x86 build computes it (cvttss2si: INT_MIN for NaN and anything outside int), without the undefined
// behaviour of the C cast: level_host.c trunc_to_int
PWN_BOX_FN int32_t pwn_box_trunc(float f)
{
	return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN;
}

// The clamped box of a sphere at (x, z) with radius r as one word: x1 | x2 << 8 | z1 << 16 | z2 << 24, every field 0 .. 63, the
// cells x1 .. x2 by z1 .. z2.  A sphere that covers no cell of the grid (an edge pair that crosses after the clamp: wholly outside,
// NaN, a negative radius larger than half a cell) gives PWN_BOX_EMPTY, whose x range is 1 .. 0.
#define PWN_BOX_EMPTY 0x00000001u
PWN_BOX_FN uint32_t pwn_box_pack(float x, float z, float r)
{
	int32_t x1 = pwn_box_trunc(x - r), z1 = pwn_box_trunc(z - r);
	int32_t x2 = pwn_box_trunc(x + r), z2 = pwn_box_trunc(z + r);
	if(x1 < 0) x1 = 0;
	if(z1 < 0) z1 = 0;
	if(x2 > 63) x2 = 63;
	if(z2 > 63) z2 = 63;
	if(x1 > x2 || z1 > z2) return PWN_BOX_EMPTY;
	return (uint32_t)x1 | (uint32_t)x2 << 8 | (uint32_t)z1 << 16 | (uint32_t)z2 << 24;
}

// cell (cx, cz), both 0 .. 63, lies in the box
PWN_BOX_FN int pwn_box_covers(uint32_t box, uint32_t cx, uint32_t cz)
{
	return cx >= (box & 0xffu) && cx <= ((box >> 8) & 0xffu) && cz >= ((box >> 16) & 0xffu) && cz <= (box >> 24);
}

// how many cells the box covers
PWN_BOX_FN uint32_t pwn_box_cells(uint32_t box)
{
	const uint32_t x1 = box & 0xffu, x2 = (box >> 8) & 0xffu, z1 = (box >> 16) & 0xffu, z2 = box >> 24;
	return (x1 > x2 || z1 > z2) ? 0u : (x2 - x1 + 1u) * (z2 - z1 + 1u);
}

// r*r of the tables (trace.h:262 `rad*rad`, one fp32 product), a result below FLT_MIN stored as 0 like the reference build's flush
PWN_BOX_FN float pwn_box_r2(float r)
{
	float r2 = r * r;
	if(r2 < 1.17549435e-38f) r2 = 0.0f;
	return r2;
}
