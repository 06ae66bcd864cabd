// The table of kernel variants (pwnfps_amd/csrc/trace_variants.h) and the mode of a launch (launch_plan.h pwn_launch_mode), printed for
// tests/test_trace_variants.py: plain g++, no HIP.
//   N name value                          the mode and list-form numbers as this build sees them
//   V unit kernel order lists mode        one line per (ORDER, LISTS, MODE) the table declares; each stands for COUNT x HAS_W kernels
//   D kind label hide reach mode          the mode of every launch descriptor, or "none" where the table holds no variant of it
#include <stdio.h>
#include "launch_plan.h"

static bool has_variant(int mode)
{
	switch(mode)
	{
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) case (MODE):
	PWN_TRACE_VARIANTS(PWN_ROW)
#undef PWN_ROW
		return true;
	}
	return false;
}

int main(void)
{
#define N(x) printf("N %s %d\n", #x, (int)x);
	N(PWN_LF_INDEXED) N(PWN_LF_INLINE) N(PWN_LF_GLOBAL)
	N(PWN_KM_FRAME) N(PWN_KM_VIEWS) N(PWN_KM_RAYS) N(PWN_KM_HITS) N(PWN_KM_VIEWPORTS) N(PWN_KM_VIEW_HITS) N(PWN_KM_VIEWPORT_HITS) N(PWN_KM_HIDE) N(PWN_KM_REACH)
#undef N
#define PWN_FORM(ORDER, LISTS) printf("V %s %s %d %d %d\n", unit, name, (int)ORDER, (int)LISTS, mode);
#define PWN_FORM_ORDER(ORDER, LISTS) if(has_order) PWN_FORM(ORDER, LISTS)
#define PWN_ROW(UNIT, NAME, MODE, HAS_ORDER) { const char *unit = #UNIT, *name = #NAME; const int mode = (MODE); const bool has_order = HAS_ORDER; PWN_TRACE_ROW_FORMS(PWN_FORM, PWN_FORM_ORDER) }
	PWN_TRACE_VARIANTS(PWN_ROW)
#undef PWN_ROW
	const int kinds[4] = { PWN_LAUNCH_FRAME, PWN_LAUNCH_VIEWS, PWN_LAUNCH_VIEWPORTS, PWN_LAUNCH_RAYS };
	for(int kind : kinds) for(int label = 0; label < 2; label++) for(int hide = 0; hide < 2; hide++) for(int reach = 0; reach <= (kind == PWN_LAUNCH_RAYS ? 1 : 0); reach++)
	{
		const pwn_launch_what W = { kind, label != 0, hide != 0, reach != 0 };
		const int mode = pwn_launch_mode(W);
		if(has_variant(mode)) printf("D %d %d %d %d %d\n", kind, label, hide, reach, mode);
		else printf("D %d %d %d %d none\n", kind, label, hide, reach);
	}
	return 0;
}
