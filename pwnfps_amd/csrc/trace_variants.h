// trace_variants.h -- which instantiations of the units kernel (trace_kernel.hip) ship, and in which translation unit: the one table.
// Plain preprocessor and C, no HIP: the four units expand it into their launchers, pwn_launch_trace into the choice of the unit,
// launch_plan.h names a launch's mode with its numbers, and tests/test_trace_variants.py holds it to the symbols of the built library.
//
// A row is (unit, kernel name, MODE, has ORDER variants).  The unit is the file that compiles the row's kernels -- MAIN trace_kernel.hip,
// HIDE trace_hide.hip, HIDE_VP trace_hide_vp.hip, REACH trace_reach.hip -- and the kernel name is what the __global__ is called there
// (the unit file's PWN_TRACE_KERNEL_NAME; trace_kernel.hip's is the default).  MODE is the kernel's template argument of that name:
// what the launch traces (PWN_KM_FRAME .. PWN_KM_VIEWPORT_HITS), or'ed with PWN_KM_HIDE (every view or ray names one sphere it does
// not see) and PWN_KM_REACH (every ray names a distance behind which it stops).
//
// Every row exists for the three forms of the sphere lists (PWN_LF_*) x COUNT x HAS_W with ORDER = false: twelve kernels.  A row with
// ORDER variants has, on top, ORDER = true for the two list forms in LDS (PWN_LF_INDEXED, PWN_LF_INLINE) x COUNT x HAS_W: eight more
// (PWN_TRACE_ROW_FORMS below is that rule).  That makes 92 + 36 + 36 + 24 = 188 kernels.  A (mode, lists, order) outside of this is
// no kernel: the launcher answers hipErrorInvalidValue.  How to add a mode: DESIGN.md, "Kernel variants".
#pragma once

// the (ORDER, LISTS) of a row: X for every row, XO for the rows with ORDER variants alone
#define PWN_TRACE_ROW_FORMS(X, XO) X(false, PWN_LF_INDEXED) X(false, PWN_LF_INLINE) X(false, PWN_LF_GLOBAL) XO(true, PWN_LF_INDEXED) XO(true, PWN_LF_INLINE)

// The numbers are tables.h's, and a file that includes it has them from there (include it first).  A host tool that cannot include
// tables.h -- it names HIP's types -- gets them here; tests/test_trace_variants.py holds the two texts equal.
#ifndef PWN_GRID_PITCH
enum { PWN_LF_INDEXED = 0, PWN_LF_INLINE = 1, PWN_LF_GLOBAL = 2 };
enum { PWN_KM_FRAME = 0, PWN_KM_VIEWS = 1, PWN_KM_RAYS = 2, PWN_KM_HITS = 3, PWN_KM_VIEWPORTS = 4, PWN_KM_VIEW_HITS = 5, PWN_KM_VIEWPORT_HITS = 6 };
enum { PWN_KM_HIDE = 8 };
enum { PWN_KM_REACH = 16 };
#endif

#define PWN_TRACE_VARIANTS_MAIN(X) \
	X(MAIN, pwn_trace_kernel, PWN_KM_FRAME, true) \
	X(MAIN, pwn_trace_kernel, PWN_KM_VIEWS, false) \
	X(MAIN, pwn_trace_kernel, PWN_KM_RAYS, false) \
	X(MAIN, pwn_trace_kernel, PWN_KM_HITS, false) \
	X(MAIN, pwn_trace_kernel, PWN_KM_VIEWPORTS, false) \
	X(MAIN, pwn_trace_kernel, PWN_KM_VIEW_HITS, false) \
	X(MAIN, pwn_trace_kernel, PWN_KM_VIEWPORT_HITS, false)
#define PWN_TRACE_VARIANTS_HIDE(X) \
	X(HIDE, pwn_trace_kernel, PWN_KM_VIEWS | PWN_KM_HIDE, false) \
	X(HIDE, pwn_trace_kernel, PWN_KM_VIEW_HITS | PWN_KM_HIDE, false) \
	X(HIDE, pwn_trace_kernel, PWN_KM_HITS | PWN_KM_HIDE, false)
#define PWN_TRACE_VARIANTS_HIDE_VP(X) \
	X(HIDE_VP, pwn_trace_hide2_kernel, PWN_KM_VIEWPORTS | PWN_KM_HIDE, false) \
	X(HIDE_VP, pwn_trace_hide2_kernel, PWN_KM_VIEWPORT_HITS | PWN_KM_HIDE, false) \
	X(HIDE_VP, pwn_trace_hide2_kernel, PWN_KM_RAYS | PWN_KM_HIDE, false)
#define PWN_TRACE_VARIANTS_REACH(X) \
	X(REACH, pwn_trace_reach_kernel, PWN_KM_HITS | PWN_KM_REACH, false) \
	X(REACH, pwn_trace_reach_kernel, PWN_KM_HITS | PWN_KM_HIDE | PWN_KM_REACH, false)
#define PWN_TRACE_VARIANTS(X) PWN_TRACE_VARIANTS_MAIN(X) PWN_TRACE_VARIANTS_HIDE(X) PWN_TRACE_VARIANTS_HIDE_VP(X) PWN_TRACE_VARIANTS_REACH(X)

// the rows of unit U (a macro's name for one is expanded first), and the function of that unit that launches them (trace_kernel.hip)
#define PWN_TV_CAT_(a, b) a##b
#define PWN_TV_CAT(a, b) PWN_TV_CAT_(a, b)
#define PWN_TRACE_UNIT_VARIANTS(U) PWN_TV_CAT(PWN_TRACE_VARIANTS_, U)
#define PWN_TRACE_UNIT_LAUNCH(U) PWN_TV_CAT(pwn_trace_unit_launch_, U)
