// trace_hide.hip -- the units kernel's HIDE unit (trace_variants.h has its rows): every view or ray names one sphere of the table that
// it does not see (pwn_trace_views_hide_device, pwn_trace_view_hits_hide_device, pwn_trace_hits_hide_device).
//
// The kernel is trace_kernel.hip's, the one text: this unit includes that file as unit HIDE, whose host part then compiles this
// unit's rows alone.  (A unit of its own: in trace_kernel.hip the kernels would add a third to its build time.)  Built with
// trace_kernel.hip's flags (Makefile TRACE_EXTRA).
#define PWN_TRACE_UNIT HIDE
#include "trace_kernel.hip"
