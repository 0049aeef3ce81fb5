// cgck_lpf.hip — lpf_kernel ("lane per packet, fill"): lpw_kernel's pipeline
// (cgck_lpw_kernel.inc, the comment in cgck_lane.hip) with the side effects
// lpw leaves out: the in-place field stores of CGCK_STORE and the running bad
// counters.  IPv4 only.  The windows, the descriptor ring and the output
// staging are lpw_kernel's; the finish is result()'s (cgck_lane.h) with the
// stores and the atomics taken out of it:
//
//  * Field stores.  A step's two fields (lo to a0 + 10 under CGCK_IP, hi to
//    a0 + hl + fo under CGCK_L4 when fo >= 0; nothing for BAD_LEN or RAW; odd
//    addresses bytewise, as store16) are carried in plain scalars and issued
//    right AFTER the next round's DMA, beside the deferred output store, so
//    the wait for the previous round can leave them in flight and they have a
//    whole round to land (stored at the end of their step they sit in front of
//    the next round in the in-order vmcnt, and its wait pays their write
//    acknowledgement).  The loosened count is the number of store
//    instructions really issued after the round waited for: the stores are
//    inline assembly run by all 64 lanes (lpf_store_field), one or two per
//    field, wave-uniform, so the count is exact; anything else stored in
//    between (an end-of-chunk flush) only makes the wait cover more.  A step
//    with no next round (a fallback step, an empty step, the last step) has
//    its fields flushed before the scalars are reused, as `pend` is.
//  * Counters.  Per step the ballots of BAD_IP / BAD_L4 are added to two
//    wave-uniform totals; after the final vmcnt(0) lane 0 adds each non-zero
//    total to p.bad[0] / p.bad[1] with one vector atomic (running: +=).
//
// Why the stores cannot change a result:
//  * A neighbour's store can never change a lane's result: every byte outside
//    a lane's own packet that enters its sum is cancelled from the same copy
//    it was summed from.  In the window path lead_sum / trail_sum read win[],
//    the same DMA'd copy as the prefix sums; in the fallback path they read
//    the same v.  Each chunk of a packet is summed from exactly one copy.  The
//    header words (t8, header<>()'s chunks, the fallback's second ldc pass)
//    are used only for the lane's own bytes, which only that lane writes, and
//    only after its finish.  (So: no second read of a shared chunk that feeds
//    a sum without its correction.)
//  * The frames of a CGCK_STORE batch do not overlap (include/cgck.h): a
//    packet's own stored field is read from the pre-store copy and nothing
//    reads it afterwards.
//  * The hand-counted waits only tighten (above).
//  * Stores stay inside the frame: +10..11 needs len >= 20 (else BAD_LEN, no
//    store), and hl + fo + 2 <= len is the fo >= 0 condition of header().
//
// A module of its own, so lpw_kernel and lpw6_kernel keep their code
// (DESIGN.md §5.6, §5.7).
#include "cgck_lane.h"

namespace cgck {

#define CGCK_LPW_KERNEL lpf_kernel
#define CGCK_LPW_IP6 false
#define CGCK_LPW_FILL true
#define CGCK_LPW_MIXED false
#include "cgck_lpw_kernel.inc"
#undef CGCK_LPW_KERNEL
#undef CGCK_LPW_IP6
#undef CGCK_LPW_FILL
#undef CGCK_LPW_MIXED

// launch_lpw's shape (lpw_shape, cgck_lane.h) at 8 one-wave workgroups per CU
hipError_t launch_lpf(const KParams &p, int num_cus, hipStream_t st)
{
	KParams q = p;
	q.contig = 0;
	const LpwShape sh = lpw_shape(p, num_cus, 8, kLpwSlot);
	if (p.desc) {
		CGCK_NOTE_KERNEL("lpf_kernel<true, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpf_kernel<true, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpf_kernel<false, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpf_kernel<false, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
