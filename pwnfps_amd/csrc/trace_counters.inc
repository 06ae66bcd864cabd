// trace_counters.inc -- a wave's counters into pwn_stats at the end of a counting kernel: wave reduce, one atomic per
// wave and counter.  Textually included by both trace kernels (as a function it moves spills in the units kernel).
// Names it uses from the including scope:
//   cnt (Counters), lane, P.counters;  PWN_CNT_REGIONS = how many of cnt.rg[] follow the first 16 counters (RG_N in
//   the units kernel, whose regions the issue model maps; 0 in the refill kernel).
{
	unsigned long long v[16 + PWN_CNT_REGIONS] = { cnt.rays, cnt.steps, cnt.portals, cnt.tests, cnt.exhausted, cnt.wsteps,
		cnt.wp[0], cnt.wp[1], cnt.wp[2], cnt.wp[3], cnt.wp[4], cnt.wp[5], cnt.wp[6], cnt.wp[7], cnt.apasses, cnt.apass_lanes };
	for(int i = 0; i < PWN_CNT_REGIONS; i++) v[16 + i] = cnt.rg[i];
	for(int i = 0; i < 16 + PWN_CNT_REGIONS; i++)
	{
		unsigned long long s = v[i];
		for(int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
		if(lane == 0 && s) atomicAdd(&P.counters[i], s);
	}
}
