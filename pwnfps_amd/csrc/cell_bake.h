/* cell_bake.h -- what the host decides once per level about every cell, for the walk's portal arms (plain C: read by
 * level_host.c, which bakes it, and through tables.h by the kernels).
 *
 * The reference asks three things of a cell that holds a letter, each time a ray meets it: what a ray that leaves a 2-high
 * room sees there (trace.h:404-413), whether the cell is one of the letter's endpoints (trace.h:508-559), and where the other
 * endpoint lies.  All three depend on the cell alone -- its coordinates, its letter, the portal table -- so the answers sit
 * in bits of the cell word (tables.h) that the level's class bits leave free and in one 4-byte record per endpoint: the 52
 * records take the room the portal table itself had in the blob, whose size decides how many workgroups a CU holds.
 *
 *   bit 0      PWN_C_LT2    seen from a 2-high room the cell counts as 2-high: '#' or '&', or an endpoint whose far side is
 *   bit 1      PWN_C_LTDQ   ... as '"'.  A cell without a letter: its own class.  Endpoint 1: the class of c2, endpoint 2: of
 *                           c1 (x2 == -1 is not asked on this path).  A letter in a cell that is not its endpoint: neither.
 *   bits 2..7  portal state (cells with PWN_C_PORTAL; 0 elsewhere)
 *                0          unpaired letter (x2 == -1): a wall of BASE_WALL
 *                1          paired letter in a cell that is not one of its endpoints: BASE_MAGENTA
 *                2 + k      an endpoint; record k says where the ray goes.  Endpoint 1 wins where both are the same cell.
 *   bits 13,14 the rotation the ray makes from THIS endpoint: (-rot12) & 3 from endpoint 1, rot12 & 3 from endpoint 2
 *              (PWN_C_RAMPX / PWN_C_RAMPM of a ramp: the walk reads them in a cell with PWN_C_RAMP only, which a letter is not)
 *
 * Record k, 32 bits: what the reference ADDS to the position, as two half floats -- x in the low half, z in the high one:
 * (float)(x2 - x1), (float)(z2 - z1) from endpoint 1, their negations (-0.0 for 0: the reference subtracts) from endpoint 2.
 * Endpoints lie within -1 .. 63, so the differences are whole numbers of at most 64, which a half float holds exactly.  The
 * other endpoint's cell is this cell plus the same two numbers.
 *
 * Row and column 64 of the table (get_cell's clamp, tables.h) are read for cells OUTSIDE the grid, whose coordinates no
 * endpoint has: their words carry what the non-endpoint path gives (state 0 or 1, neither look-through bit for a letter)
 * also where the cell they repeat is an endpoint.  The one coordinate outside the grid that a portal table can hold is -1,
 * where x == -1 says "no endpoint": pwn_check_portals (level_host.c) takes the tables on which the reference's tests give
 * the cells at -1 these same answers.
 */
#ifndef PWN_CELL_BAKE_H
#define PWN_CELL_BAKE_H
#include <stdint.h>

#define PWN_C_LT2        0x01u
#define PWN_C_LTDQ       0x02u
#define PWN_C_PST_MASK   0xfcu
#define PWN_C_PST_SHIFT  2u
#define PWN_PST_WALL     0u
#define PWN_PST_MAGENTA  1u
#define PWN_PST_REC0     2u
#define PWN_EP_MAX       52u    /* two endpoints of 26 letters */

#define PWN_C_PROT_SHIFT 13u

#endif
