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
#include "cgck_lpw_kernel.inc"
#undef CGCK_LPW_KERNEL
#undef CGCK_LPW_IP6
#undef CGCK_LPW_FILL

bool lpw_ok(const KParams &p);

// An IPv6 batch lpw6 takes: what lpw takes (no STORE, no bad counters, no
// internal flags, 16-byte aligned descriptors) with CGCK_IP6 set.
bool lpw6_ok(const KParams &p)
{
	return (p.flags & CGCK_IP6) && lpw_ok(p);
}

// launch_lpw's shape: 8 KiB windows, chunks of 4 steps, 19.3 KiB of LDS per
// workgroup, 8 one-wave workgroups per CU (the product shape only)
hipError_t launch_lpw6(const KParams &p, int num_cus, hipStream_t st)
{
	KParams q = p;
	q.contig = 0;
	constexpr int C = 4;
	const uint64_t want = (p.n + 64 * C - 1) / (64 * C), cap = (uint64_t)num_cus * 8;
	const dim3 g((unsigned)(want < cap ? (want ? want : 1) : cap));
	const size_t lds = 2 * kLpwSlot + 2 * 1024 + C * 64 * (p.verdict ? 5 : 4);
	if (p.desc) {
		CGCK_NOTE_KERNEL("lpw6_kernel<true, %d, false>", C);
		hipLaunchKernelGGL((lpw6_kernel<true, C, false>), g, dim3(64), lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpw6_kernel<false, %d, false>", C);
		hipLaunchKernelGGL((lpw6_kernel<false, C, false>), g, dim3(64), lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
