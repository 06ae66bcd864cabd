// trace_hide_vp.hip -- the units kernel's HIDE_VP unit (trace_variants.h has its rows): the hidden sphere for views of their own sizes,
// their first-hit planes and the colours of caller-supplied rays (pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device,
// pwn_trace_rays_hide_device).
//
// The kernel is trace_kernel.hip's, the one text, as in trace_hide.hip, with a name of its own for the __global__: tests pin the
// instantiations of pwn_trace_kernel that carry the HIDE bit to trace_hide.hip's, and a second name changes nothing of what the other
// units compile.  Built with trace_kernel.hip's flags (Makefile TRACE_EXTRA).
#define PWN_TRACE_UNIT HIDE_VP
#define PWN_TRACE_KERNEL_NAME pwn_trace_hide2_kernel
#include "trace_kernel.hip"
