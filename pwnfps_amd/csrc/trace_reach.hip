// trace_reach.hip -- the units kernel's REACH instantiations (pwn_trace_reach, pwn_trace_reach_device, pwn_trace_reach_hide_device: every
// ray names a distance behind which its walk stops, and a ray that stops so gets a PWN_HIT_FREE record) and pwn_launch_trace_reach.
//
// The kernel is trace_kernel.hip's, the one text, as in trace_hide.hip and trace_hide_vp.hip: this unit includes that file with
// PWN_TRACE_REACH_UNIT set, which swaps its host part for the launcher of these twenty-four kernels -- PWN_KM_HITS | PWN_KM_REACH with and
// without PWN_KM_HIDE x three list forms x COUNT x HAS_W -- and with a name of its own for the __global__, so that the set of
// pwn_trace_kernel's instantiations stays what it was and none of the other three units compiles one token differently.  Built with
// trace_kernel.hip's flags (Makefile TRACE_EXTRA).
#define PWN_TRACE_REACH_UNIT
#define PWN_TRACE_KERNEL_NAME pwn_trace_reach_kernel
#include "trace_kernel.hip"
