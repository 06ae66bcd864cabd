// trace_reach.hip -- the units kernel's REACH unit (trace_variants.h has its rows): every ray names a distance behind which its walk
// stops, and a ray that stops so gets a PWN_HIT_FREE record (pwn_trace_reach, pwn_trace_reach_device, pwn_trace_reach_hide_device).
//
// The kernel is trace_kernel.hip's, the one text, as in trace_hide.hip and trace_hide_vp.hip, with a name of its own for the
// __global__, so that the set of pwn_trace_kernel's instantiations stays what it was.  Built with trace_kernel.hip's flags (Makefile
// TRACE_EXTRA).
#define PWN_TRACE_UNIT REACH
#define PWN_TRACE_KERNEL_NAME pwn_trace_reach_kernel
#include "trace_kernel.hip"
