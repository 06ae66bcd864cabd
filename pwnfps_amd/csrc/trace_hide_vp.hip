// trace_hide_vp.hip -- the units kernel's HIDE instantiations for views of their own sizes, their first-hit planes and the colours of
// caller-supplied rays (pwn_trace_viewports_hide_device, pwn_trace_viewport_hits_hide_device, pwn_trace_rays_hide_device) and
// pwn_launch_trace_hide2.
//
// The kernel is trace_kernel.hip's, the one text, as in trace_hide.hip: this unit includes that file with PWN_TRACE_HIDE_VP_UNIT set,
// which swaps its host part for the launcher of these thirty-six kernels, and with a name of its own for the __global__ -- the
// instantiations of pwn_trace_kernel that carry the HIDE bit stay the thirty-six of trace_hide.hip, and neither of the other two units
// compiles one token differently.  Built with trace_kernel.hip's flags (Makefile TRACE_EXTRA).
#define PWN_TRACE_HIDE_VP_UNIT
#define PWN_TRACE_KERNEL_NAME pwn_trace_hide2_kernel
#include "trace_kernel.hip"
