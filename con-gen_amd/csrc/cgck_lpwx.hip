// cgck_lpwx.hip — lpwx_kernel: lpw_kernel's pipeline (cgck_lpw_kernel.inc, the
// comment in cgck_lane.hip) over a batch that mixes families (CGCK_MIXED), the
// same kernel text compiled with MIXED set.  The windows, the descriptor ring,
// the counted waits and the output staging are lpw_kernel's.  At the end of a
// step each lane holds its packet's sum over [0, len) and its first eight
// header chunks, which is all either finish needs, so the family is a per-lane
// choice (lpwx_headers, lpwx_result in the kernel text):
//
//  * Family.  v = the high nibble of byte q of header chunk 0.  Both header
//    decoders run, each with its own family's lanes as its activity flag
//    (header<8, false>() for v == 4, header6() for v == 6), so every
//    wave-uniform path inside them is chosen from the lanes whose result is
//    used.  Neither forms a load: with eight chunks in registers header<>()
//    never fetches, and header6() only reads registers.  The one place that
//    reads global memory by header fields, result6()'s walk of an extension
//    chain, does so only in lanes with v == 6 (`chain` includes the activity
//    flag, and __any(chain) skips it for a wave without such a lane).
//  * IPv4 finish.  result_t<true>() (cgck_lane.h) with kFlagL4Auto in the
//    flags: ip_p == 1 is in_cksum(ip + hl, len - hl) with its field at +2,
//    every other protocol takes the pseudo-header, as the group kernel does
//    for the RX window.
//  * IPv6 finish.  result6() without CGCK_V_UDP_ZERO_SKIP.
//  * Neither family: out 0, CGCK_NOT_IP; ip_len 0: CGCK_BAD_LEN.
//  * Counters.  lpf_kernel's scheme: two ballots a step into wave-uniform
//    totals, one vector atomic per non-zero total after the final vmcnt(0).
//  * No store into a packet, so lpf's correctness argument is not needed, and
//    no VMEM instruction between a round's issue and the wait for the round
//    before it beyond lpw6_kernel's.
//  * Descriptors.  The ring needs a 16-byte aligned array (DRING true).  For
//    any other 4-byte aligned array (DRING false) the ring's DMA moves zero
//    lines, so the rounds keep their count, and step j + 2's descriptors are
//    read from global memory after the wait for window 0 of step j, where the
//    ring would have been read: a compiler-tracked load, waited for before it
//    is used, which only makes the counted waits cover more.
//
// A module of its own, so lpw_kernel, lpw6_kernel and lpf_kernel keep their
// code.
#include "cgck_lane.h"

namespace cgck {

#define CGCK_LPW_KERNEL lpwx_kernel
#define CGCK_LPW_IP6 false
#define CGCK_LPW_FILL false
#define CGCK_LPW_MIXED true
#include "cgck_lpw_kernel.inc"
#undef CGCK_LPW_KERNEL
#undef CGCK_LPW_IP6
#undef CGCK_LPW_FILL
#undef CGCK_LPW_MIXED

// launch_lpw's shape (lpw_shape, cgck_lane.h) at 8 one-wave workgroups per CU
hipError_t launch_lpwx(const KParams &p, int num_cus, hipStream_t st)
{
	KParams q = p;
	q.contig = 0;
	const LpwShape sh = lpw_shape(p, num_cus, 8, kLpwSlot);
	if (!p.desc) {
		CGCK_NOTE_KERNEL("lpwx_kernel<false, %d, false, true>", kLpwC);
		hipLaunchKernelGGL((lpwx_kernel<false, kLpwC, false, true>), sh.grid, dim3(64), sh.lds, st, q);
	} else if ((reinterpret_cast<uintptr_t>(p.desc) & 15) == 0) {
		CGCK_NOTE_KERNEL("lpwx_kernel<true, %d, false, true>", kLpwC);
		hipLaunchKernelGGL((lpwx_kernel<true, kLpwC, false, true>), sh.grid, dim3(64), sh.lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpwx_kernel<true, %d, false, false>", kLpwC);
		hipLaunchKernelGGL((lpwx_kernel<true, kLpwC, false, false>), sh.grid, dim3(64), sh.lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
