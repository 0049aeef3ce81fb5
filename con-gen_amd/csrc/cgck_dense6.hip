// cgck_dense6.hip - dstr6_kernel: dstr_kernel (cgck_dense.hip) over IPv6
// frames (CGCK_IP6), the same kernel text compiled with IP6 set.  The
// reducing wave stages each frame's sum, the sum of its first 8 bytes and
// byte 6; the writer wave finishes with the no-extension identity (v6_dense,
// cgck_device.h): L4 sum = sum of bytes [8, ip_len) + htons(ip_len - 40) +
// (nh << 8).  A frame with extension headers is finished by the same lane
// from global memory: exact, only slower.
#include "cgck_device.h"

namespace cgck {

#define CGCK_DSTR_KERNEL dstr6_kernel
#define CGCK_DSTR_IP6 true
#include "cgck_dense_kernel.inc"
#undef CGCK_DSTR_KERNEL
#undef CGCK_DSTR_IP6

// The product shape of launch_dstr (cgck_dense.hip), which sizes the grid.
hipError_t launch_dstr6(const KParams &p, unsigned blocks, hipStream_t st)
{
	CGCK_NOTE_KERNEL("dstr6_kernel<3, 16, true, 0>");
	hipLaunchKernelGGL((dstr6_kernel<3, 16, true, 0>), dim3(blocks), dim3(128), 3 * kDsSlot + 64 * 16, st, p);
	return hipGetLastError();
}

} // namespace cgck
