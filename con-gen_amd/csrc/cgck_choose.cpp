// cgck_choose.cpp — the kernel choice: each family's acceptance predicate and
// the rules that pick among them (enum Family, cgck_params.h, says what each
// family is).  Host arithmetic on KParams only.
#include "cgck_choose.h"

namespace cgck {
namespace {

// No internal flag: those are the group kernel's alone.
bool lane_ok(const KParams &p)
{
	return !(p.flags & (kFlagNoLenCheck | kFlagL4Auto | kFlagRx | kFlagGroup));
}

// An IPv6 batch the lane family's variants (lpd6, lpa6) take: at least the
// fixed header, and IP / L4 only: no field zeroing, verify or store, so no
// bad counters either (RAW | IP6 reaches the kernels as RAW).
bool lane6_ok(const KParams &p)
{
	return (p.flags & CGCK_IP6) && !(p.flags & ~(uint32_t)(CGCK_IP6 | CGCK_IP | CGCK_L4)) && p.ip_len >= 40;
}

// aligned fixed-length strided batch of 20..64-byte packets (the 64 B config)
bool lpa_ok(const KParams &p)
{
	return lane_ok(p) && (!(p.flags & CGCK_IP6) || lane6_ok(p)) && !p.desc && p.ip_len >= 20 && p.ip_len <= 64 &&
	       ((reinterpret_cast<uintptr_t>(p.base) | p.stride | p.l3_off) & 15) == 0;
}

bool lpd_ok(const KParams &p)
{
	// an output array, 16-byte aligned: a chunk's outputs leave as 16-byte stores
	return !p.desc && !p.verdict && !p.bad && !(p.flags & CGCK_STORE) && p.out &&
	       (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 && p.ip_len >= 20 && p.ip_len <= 64 &&
	       p.stride <= 64 && p.stride * 63 + p.ip_len <= 4096 &&
	       ((reinterpret_cast<uintptr_t>(p.base) | p.stride | p.l3_off) & 15) == 0;
}

// No side effects, no internal flags, 16-byte aligned descriptors (they travel by DMA).
bool lpw_ok(const KParams &p)
{
	return !p.bad && !(p.flags & (CGCK_STORE | kFlagNoLenCheck | kFlagL4Auto)) &&
	       (reinterpret_cast<uintptr_t>(p.desc) & 15) == 0;
}

// An IPv6 batch lpw6 takes: what lpw takes with CGCK_IP6 set.
bool lpw6_ok(const KParams &p)
{
	return (p.flags & CGCK_IP6) && lpw_ok(p);
}

// A batch lpf takes: IPv4 with a side effect (STORE or the bad counters), no
// internal flags, 16-byte aligned descriptors.  A batch with neither is lpw's.
bool lpf_ok(const KParams &p)
{
	return !(p.flags & CGCK_IP6) && ((p.flags & CGCK_STORE) || p.bad) &&
	       !(p.flags & (kFlagNoLenCheck | kFlagL4Auto)) && (reinterpret_cast<uintptr_t>(p.desc) & 15) == 0;
}

bool dstr_ok(const KParams &p)
{
	// IPv6 (dstr6_kernel): IP and L4 only (RAW | IP6 reaches the kernels as RAW)
	if ((p.flags & CGCK_IP6) && (p.ip_len < 40 || (p.flags & ~(uint32_t)(CGCK_IP6 | CGCK_IP | CGCK_L4))))
		return false;
	const uint32_t fl = p.flags & ~(uint32_t)CGCK_IP6;
	const bool flags_ok = fl == CGCK_RAW || (fl && !(fl & ~(uint32_t)(CGCK_IP | CGCK_L4 | CGCK_L4_NOPSEUDO)));
	return !p.desc && p.n > 0 && p.n < (1ull << 34) && flags_ok && !p.bad && p.out &&
	       (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 && p.ip_len >= 20 && p.ip_len <= 1520 &&
	       p.stride <= 1520 && ((reinterpret_cast<uintptr_t>(p.base) | p.stride | p.l3_off) & 3) == 0;
}

#if CGCK_LAB
bool span_ok(const KParams &p)
{
	return p.desc && !(p.flags & (CGCK_STORE | kFlagNoLenCheck | kFlagL4Auto));
}

bool stream_ok(const KParams &p)
{
	const uint32_t fl = p.flags;
	const bool flags_ok = fl == CGCK_RAW || (fl && !(fl & ~(uint32_t)(CGCK_IP | CGCK_L4 | CGCK_L4_NOPSEUDO)));
	return !p.desc && p.n > 0 && flags_ok && !p.bad && p.ip_len >= 20 && p.ip_len <= 1520 && p.stride <= 1520 &&
	       ((reinterpret_cast<uintptr_t>(p.base) | p.stride | p.l3_off) & 3) == 0;
}
#endif

// The automatic pick.
Family automatic(const KParams &p, uint32_t len_hint, bool packed_hint)
{
	if (!lane_ok(p))
		return kGroup;
	if (lpa_ok(p))
		return lpd_ok(p) ? kLpd : kLpa;
	// Dense strided batches of >= 1 KiB frames take dstr_kernel (cgck_dense.hip,
	// LDS-DMA steps of 4 frames with a writer wave): 80.3-82.0 % vs the group
	// kernel's 78.6-81.5 % in the same process (tools/dstr_sweep.sh,
	// profiles/r02/dense/).  The first LDS-DMA stream kernel (cgck_stream.hip,
	// 76.9 % vs 77.9 %) stays in the lab build.
	if (len_hint >= kGroupFromLen)
		return dstr_ok(p) ? kDstr : kGroup;
	if (len_hint <= kLppUpToLen)
		return kLpp;
	// 256 B <= typical length < 1 KiB: lpw streams 64-frame steps through LDS
	// by DMA, the step's span itself when its frames lie back to back and the
	// frames' chunk runs gathered otherwise, decided per step on the device
	// (tools/family_ab.py, profiles/r03/: 16M IMIX packed without a hint 73.0 %
	// vs slot2 62.8 %, in 2048 B ring slots at +14 62.0 vs 45.7 %; dense strided
	// 256 / 576 / 1000 B 69.6 / 73.1 / 74.7 % vs slot2's 52.1 / 56.6 / 48.4 %,
	// profiles/r02/dma/lpw; 160 B 46.9 vs 59.8 %, 1500 B 75.6 vs group 79.9 %).
	// The layout hint does not change that choice.  A batch with bad counters
	// or CGCK_STORE streams through lpf, the same pipeline with those side
	// effects, instead of falling to slot2 (tools/fill_ab.py, profiles/lpf/,
	// VERIFY with counters 1.07 vs slot2's 1.28 ms packed, 1.37
	// vs 1.49 ms in ring slots; FILL_BOTH in ring slots 2.00 vs 2.14 ms) with
	// one exception: FILL_BOTH on packed frames measured 1.73 vs slot2's 1.70
	// ms, so a descriptor batch with CGCK_STORE under the packed layout hint
	// stays on slot2 (a pinned "lpw" still runs it in lpf).
	const bool packed_fill = (p.flags & CGCK_STORE) && p.desc && packed_hint;
	const bool streams = lpw_ok(p) || (lpf_ok(p) && !packed_fill);
	const bool laid_out = p.desc || p.stride > 0;
	return len_hint >= kLpwFromLen && streams && laid_out ? kLpw : kSlot2;
}

} // namespace

Choice choose(const KParams &p, uint32_t len_hint, int kernel_bits)
{
	const bool ip6 = p.flags & CGCK_IP6;
	int f = kernel_bits & kFamilyMask;
	// a pinned family this build lacks is auto
	bool in_this_build = CGCK_LAB;
	for (const auto &name : kFamilyNames)
		in_this_build |= name.family == f && !name.lab_only;
	if (f == kAuto || !in_this_build)
		f = automatic(p, len_hint, kernel_bits & kPacked);
	// the internal flags go only to group
	if (!lane_ok(p))
		f = kGroup;
	// IPv6 goes only to a family with an IPv6 variant: lpa, lpd, dstr, lpw where
	// lpw6 takes the batch, and group; lpp, slot2, lpf (and the lab's) are IPv4 only
	if (ip6 && f != kLpa && f != kLpd && f != kDstr && !(f == kLpw && lpw6_ok(p)))
		f = kGroup;
	// a family whose precondition fails falls back to lpa, lpp (IPv4), slot2 or group
	if (f == kLpa && !lpa_ok(p))
		f = ip6 ? kGroup : kLpp;
	if (f == kLpd && !(lpa_ok(p) && lpd_ok(p)))
		f = lpa_ok(p) ? kLpa : ip6 ? kGroup : kLpp;
#if CGCK_LAB
	if (f == kSpan && !span_ok(p))
		f = kGroup;
#endif
	if (f == kDstr && !dstr_ok(p))
		f = kGroup;
	if (f == kLpw && !lpw_ok(p) && !lpf_ok(p))
		f = kSlot2;
	// the family's kernel: lpw's by the batch, lpp shape 2 is the product's lpp
	Kernel k = f == kLpw ? (ip6 ? Kernel::kLpw6 : lpf_ok(p) ? Kernel::kLpf : Kernel::kLpw)
			     : f == kLpp2 ? Kernel::kLpp : static_cast<Kernel>(f);
#if CGCK_LAB
	if (k == Kernel::kDstr && (kernel_bits & kStrOld) && stream_ok(p))
		k = Kernel::kStream;
#endif
	// nontemporal loads and contiguous block ranges: as given, or the family's measured defaults
	if (kernel_bits & kExplicit)
		return {k, (kernel_bits & kNT) != 0, (kernel_bits & kContig) != 0};
	return {k, f == kGroup ? kDefaultGroupNT : kDefaultLaneNT, f == kGroup ? kDefaultGroupContig : kDefaultLaneContig};
}

} // namespace cgck
