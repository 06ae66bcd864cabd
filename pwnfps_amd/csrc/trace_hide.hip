// trace_hide.hip -- the units kernel's HIDE instantiations (pwn_trace_views_hide_device, pwn_trace_view_hits_hide_device,
// pwn_trace_hits_hide_device: every view or ray names one sphere of the table that it does not see) and pwn_launch_trace_hide.
//
// The kernel is trace_kernel.hip's, the one text: this unit includes that file with PWN_TRACE_HIDE_UNIT set, which swaps its host
// part -- pwn_launch_trace and the occupancy questions -- for the launcher of the thirty-six HIDE kernels.  Templates are
// instantiated where they are used, so neither unit compiles the other's kernels.  Built with trace_kernel.hip's flags (Makefile
// TRACE_EXTRA).
#define PWN_TRACE_HIDE_UNIT
#include "trace_kernel.hip"
