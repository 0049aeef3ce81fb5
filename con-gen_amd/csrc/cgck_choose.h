// cgck_choose.h — which kernel a batch runs on: a pure function of the batch's
// parameters, its length hint and the context's pin, with no HIP in it, so the
// whole decision table is tested on the CPU (tools/dispatch_table.cpp).
#pragma once
#include "cgck_params.h"

namespace cgck {

// The launcher that runs and, where the choice decides it, the variant: up to
// 15 the Family of that name, above it lpw's other kernels and the lab's first
// stream kernel.  (The launchers fork to cksum6, lpa6, lpd6, dstr6 themselves.)
enum class Kernel : int {
	kGroup = 1, kLpp = 2, kSlot2 = 9, kLpa = 10, kDstr = 11, kLpd = 13, kLpw = 15, kLpw6 = 16, kLpf = 17,
#if CGCK_LAB
	kSlot = 3, kLppp = 4, kLpp1 = 5, kLpp3 = 7, kLpp0 = 8, kSpan = 12, kSlotd = 14, kStream = 18,
#endif
};

struct Choice { Kernel kernel; bool nt; bool contig; }; // nt: nontemporal loads; contig: KParams.contig

// kernel_bits = Family | kNT | kContig | kExplicit | kPacked | kStrOld;
// len_hint = the batch's packet length (strided) or typical length (descriptors).
// Precondition: p.flags has no CGCK_MIXED (launch_cksum sends such a batch to lpwx_kernel first).
Choice choose(const KParams &p, uint32_t len_hint, int kernel_bits);

} // namespace cgck
