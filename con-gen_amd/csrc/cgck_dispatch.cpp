// cgck_dispatch.cpp — launches the kernel and launch shape choose() picks for
// a batch (cgck_choose.cpp; enum Family, cgck_params.h, describes the
// families and says which of them libcgck.so carries).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "cgck_choose.h"
#include "cgck_internal.h"

namespace cgck {

thread_local const char *t_kernel = "";

const char *intern(const char *fmt, ...)
{
	// called once per launch site (function-local static): the strings live
	// for the process
	static std::mutex mu;
	char buf[128];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	std::lock_guard<std::mutex> lk(mu);
	return strdup(buf);
}

hipError_t launch_group(const KParams &p, uint32_t max_len, int num_cus, bool nt, hipStream_t st);
hipError_t launch_lpp(const KParams &p, int num_cus, bool nt, int shape, hipStream_t st);
hipError_t launch_slot2(const KParams &p, int num_cus, bool nt, hipStream_t st);
hipError_t launch_lpa(const KParams &p, int num_cus, bool nt, hipStream_t st);
hipError_t launch_lpd(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_lpw(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_lpw6(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_lpf(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_lpwx(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_dstr(const KParams &p, int num_cus, hipStream_t st);
#if CGCK_LAB
hipError_t launch_span(const KParams &p, int num_cus, bool nt, hipStream_t st);
hipError_t launch_slot(const KParams &p, int num_cus, bool nt, hipStream_t st);
hipError_t launch_lppp(const KParams &p, int num_cus, bool nt, hipStream_t st);
hipError_t launch_stream(const KParams &p, int num_cus, hipStream_t st);
hipError_t launch_slotd(const KParams &p, int num_cus, hipStream_t st);
#endif

// Launches the kernel choose() names (cgck_choose.cpp) for `kernel` = Family |
// bits (cgck_params.h): cgck_ctx_set_kernel pins the family by name; in the
// lab build so does $CGCK_KERNEL.
hipError_t launch_cksum(const KParams &p0, uint32_t len_hint, int num_cus, int kernel, hipStream_t st)
{
	if (p0.n == 0)
		return hipSuccess;
	// a CGCK_MIXED batch has one kernel, whatever is pinned: choose() never sees it
	if (p0.flags & CGCK_MIXED)
		return launch_lpwx(p0, num_cus, st);
	// $CGCK_STR_OLD (lab build): the first stream kernel (cgck_stream.hip) for kDstr
	const Choice c = choose(p0, len_hint, (kernel & ~kStrOld) | (CGCK_ENV("CGCK_STR_OLD") ? kStrOld : 0));
	KParams p = p0;
	p.contig = c.contig;
	switch (c.kernel) {
	case Kernel::kGroup: return launch_group(p, len_hint, num_cus, c.nt, st);
	case Kernel::kLpp: return launch_lpp(p, num_cus, c.nt, kDefaultLppShape, st);
	case Kernel::kSlot2: return launch_slot2(p, num_cus, c.nt, st);
	case Kernel::kLpa: return launch_lpa(p, num_cus, c.nt, st);
	case Kernel::kLpd: return launch_lpd(p, num_cus, st);
	case Kernel::kLpw: return launch_lpw(p, num_cus, st);
	case Kernel::kLpw6: return launch_lpw6(p, num_cus, st);
	case Kernel::kLpf: return launch_lpf(p, num_cus, st);
	case Kernel::kDstr: return launch_dstr(p, num_cus, st);
#if CGCK_LAB
	case Kernel::kStream: return launch_stream(p, num_cus, st);
	case Kernel::kSpan: return launch_span(p, num_cus, c.nt, st);
	case Kernel::kSlot: return launch_slot(p, num_cus, c.nt, st);
	case Kernel::kLppp: return launch_lppp(p, num_cus, c.nt, st);
	case Kernel::kLpp1: return launch_lpp(p, num_cus, c.nt, 1, st);
	case Kernel::kLpp3: return launch_lpp(p, num_cus, c.nt, 3, st);
	case Kernel::kLpp0: return launch_lpp(p, num_cus, c.nt, 0, st);
	case Kernel::kSlotd: return launch_slotd(p, num_cus, st);
#endif
	}
	return hipErrorInvalidValue;
}

} // namespace cgck
