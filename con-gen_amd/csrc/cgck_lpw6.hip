// cgck_lpw6.hip — lpw6_kernel: lpw_kernel's pipeline (cgck_lpw_kernel.inc, the
// comment in cgck_lane.hip) over IPv6 records (CGCK_IP6), the same kernel text
// compiled with IP6 set.  The windows, the descriptor ring, the counted waits
// and the output staging are lpw_kernel's; at the end of a step the lane forms
// its packet's result from the sum over [0, len), the sum of the first 8 bytes,
// byte 6 and (ZERO_FIELDS / VERIFY) the stored field, all read from the header
// chunks it gathered (header6, result6: cgck_lane.h), and walks a packet with
// extension headers from global memory.  A module of its own, so lpw_kernel and
// the other lane kernels keep their code.
#include "cgck_lane.h"

namespace cgck {

#define CGCK_LPW_KERNEL lpw6_kernel
#define CGCK_LPW_IP6 true
#define CGCK_LPW_FILL false
#define CGCK_LPW_MIXED false
#include "cgck_lpw_kernel.inc"
#undef CGCK_LPW_KERNEL
#undef CGCK_LPW_IP6
#undef CGCK_LPW_FILL
#undef CGCK_LPW_MIXED

// launch_lpw's shape (lpw_shape, cgck_lane.h) at 8 one-wave workgroups per CU
hipError_t launch_lpw6(const KParams &p, int num_cus, hipStream_t st)
{
	KParams q = p;
	q.contig = 0;
	const LpwShape sh = lpw_shape(p, num_cus, 8, kLpwSlot);
	if (p.desc) {
		CGCK_NOTE_KERNEL("lpw6_kernel<true, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpw6_kernel<true, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpw6_kernel<false, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpw6_kernel<false, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
