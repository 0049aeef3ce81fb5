// cgck_route.cpp — the route a host-resident request takes through the burst
// server, from the predicates of cgck_route.h that desc_host_impl /
// cgck_burst_request (cgck_api.cpp, cgck_burst.cpp) and burst_server_kernel (cgck_group.hip)
// themselves call.  Host arithmetic only.  It assumes the product's settings:
// no lab opts bits, the default caps (kServerPktsDefault, kServerCopyDefault,
// kBurstPerWG) and a device of at least kBurstMaxWG CUs.
#include "cgck_route.h"

#include <stdio.h>

#include "cgck_params.h"

namespace cgck {

// The flag sets burst_body_spec (cgck_group.hip) compiles a one-workgroup body
// for.  Its switch instantiates templates, so the list is restated here: a set
// added there or here is added to the other.
static bool route_spec(uint32_t flags, bool ldsp)
{
	switch (flags) {
	case kRxFlags:
	case kTxFlags:
	case kTxFlags | kFlagL4Auto:
	case CGCK_VERIFY_BSD:
	case CGCK_FILL_BOTH:
		return true;
	}
	// (the drop-in symbols' one region, staged)
	return ldsp && (flags == CGCK_RAW || flags == (CGCK_L4 | kFlagNoLenCheck));
}

// burst_body's parts of packets [lo, hi): either side of n1 runs on its own.
static int part_mask(bool g4, uint32_t lo, uint32_t hi, uint32_t n1)
{
	if (n1 > lo && n1 < hi)
		return (burst_u1(g4, n1 - lo) ? 1 : 2) | (burst_u1(g4, hi - n1) ? 1 : 2);
	return burst_u1(g4, hi - lo) ? 1 : 2;
}

Route burst_route(const RouteIn &in)
{
	Route r = {RouteLoc::kLaunch, false, 0, RouteBody::kStaged, 0, 0, 1, false};
	const bool request = in.mem == kRouteRequest;
	if (in.n == 0 || in.max_pkts == 0 || in.max_bytes == 0)
		return r;
	if (request && (in.flags & (CGCK_IP6 | CGCK_MIXED))) {
		r.loc = RouteLoc::kRefused;
		return r;
	}
	// the host: in place or staged, server or launch
	const bool in_place = request || burst_in_place(in.mem == kRouteRegistered, in.flags & CGCK_STORE, in.posted,
							in.pkt_bytes, in.n, kServerCopyDefault);
	const size_t cap = burst_stage_cap(in.max_pkts, in.max_bytes);
	const bool fits = burst_fits_caps(in.max_pkts, kServerPktsDefault, cap, in.max_bytes, in.n,
					  in_place ? 0 : in.pkt_bytes, request ? 0 : in.pkt_bytes);
	if (!burst_flags_ok(in.flags, in_place) || !fits) {
		r.loc = request ? RouteLoc::kRefused : RouteLoc::kLaunch;
		return r;
	}
	// the server
	const uint32_t n = (uint32_t)in.n;
	const uint32_t n1 = in.n1 < n ? in.n1 : 0;
	const uint32_t K = burst_wgs(in.max_pkts, kBurstMaxWG, kBurstPerWG);
	const bool g4 = burst_g4(in.max_len);
	r.in_place = in_place;
	r.W = burst_wgs(n, K, kBurstPerWG);
	r.G = g4 ? 4 : 16;
	if (r.W == 1) {
		const uint32_t bytes = (uint32_t)burst_layout(in_place ? 0 : in.pkt_bytes, n).bytes;
		const bool in_lds = burst_in_lds(bytes);
		const bool sys = in_place && burst_sys_ok(in.max_len, n);
		r.loc = in_lds ? RouteLoc::kLds : RouteLoc::kScratch;
		r.body = sys ? RouteBody::kSys : in_place ? RouteBody::kInPlace : in_lds ? RouteBody::kLdsp : RouteBody::kStaged;
		// the LDS block's system-coherent and LDS-resident bodies go through
		// burst_body_spec; the others take the run-time flags.  (The scratch
		// copy's sys and in-place bodies exist, burst_body<false, true> and
		// burst_body<false> over h.base, but no product request reaches them:
		// an in-place block is 64 + 12 n bytes, at most 832 for n <= 64.)
		const bool spec = in_lds && (sys || !in_place);
		r.fl = spec && !n1 && route_spec(in.flags, r.body == RouteBody::kLdsp);
		r.u_mask = (r.body == RouteBody::kSys || r.body == RouteBody::kLdsp) ? 1 : part_mask(g4, 0, n, n1);
		return r;
	}
	r.loc = RouteLoc::kSlice;
	r.body = in_place ? RouteBody::kInPlace : RouteBody::kStaged;
	for (uint32_t j = 0; j < r.W; j++) {
		const uint32_t lo = burst_slice_at(n, j, r.W), hi = burst_slice_at(n, j + 1, r.W);
		uint32_t passes = 0;
		for (uint32_t c0 = lo; c0 < hi; c0 += kSliceLds, passes++)
			r.u_mask |= part_mask(g4, c0, burst_pass_end(c0, hi), n1);
		r.passes = passes > r.passes ? passes : r.passes;
	}
	return r;
}

int route_name(const Route &r, char *name, size_t cap)
{
	int k;
	if (r.loc == RouteLoc::kLaunch || r.loc == RouteLoc::kRefused) {
		k = snprintf(name, cap, "%s", r.loc == RouteLoc::kLaunch ? "launch" : "refused");
		return k >= 0 && (size_t)k < cap ? k : -1;
	}
	static const char *const body[] = {"sys", "ldsp", "staged", "inplace"};
	static const char *const us[] = {"", "u1", "u4", "u4+u1"};
	char head[16], tail[24] = "";
	if (r.loc == RouteLoc::kSlice)
		snprintf(head, sizeof head, "wide%u/slice", r.W);
	else
		snprintf(head, sizeof head, "one/%s", r.loc == RouteLoc::kLds ? "lds" : "scratch");
	if (r.passes > 1)
		snprintf(tail, sizeof tail, "/%upasses", r.passes);
	k = snprintf(name, cap, "%s/%s/g%d%s/%s%s", head, body[(int)r.body], r.G, us[r.u_mask & 3], r.fl ? "fl" : "rt", tail);
	return k >= 0 && (size_t)k < cap ? k : -1;
}

// cksum_body instantiations behind the kinds ("Burst server", has the table):
// sys <G, S, 1, true, false, true, true, true, false, FL>, ldsp <..., true,
// false, true, true, FL>, the plain ones <G, S, U, true, false, LDSD, false,
// WT, false, 0> with LDSD = the block in LDS or a slice, WT = one workgroup.
const RouteKind kRouteKinds[] = {
	{"one/lds/sys/g4u1/fl", true},         {"one/lds/sys/g4u1/rt", true},
	{"one/lds/sys/g16u1/fl", true},        {"one/lds/sys/g16u1/rt", true},
	{"one/lds/ldsp/g4u1/fl", true},        {"one/lds/ldsp/g4u1/rt", true},
	{"one/lds/ldsp/g16u1/fl", true},       {"one/lds/ldsp/g16u1/rt", true},
	{"one/lds/inplace/g16u1/rt", true},    {"one/lds/inplace/g16u4/rt", true},
	{"one/scratch/staged/g16u1/rt", true}, {"one/scratch/staged/g16u4/rt", true},
	{"wide/slice/staged/g4u1/rt", true},   {"wide/slice/staged/g4u4/rt", true},
	{"wide/slice/staged/g16u1/rt", true},  {"wide/slice/staged/g16u4/rt", true},
	{"wide/slice/staged/passes", true},
	{"wide/slice/inplace/g4u1/rt", true},  {"wide/slice/inplace/g4u4/rt", true},
	{"wide/slice/inplace/g16u1/rt", true}, {"wide/slice/inplace/g16u4/rt", true},
	{"wide/slice/inplace/passes", true},
	// No product request reaches these.  In place with max_len <= 80 and
	// n <= 64 is always burst_sys_ok, and a staged block of 64 frames of 80
	// bytes is 5952 bytes: the plain G = 4 one-workgroup bodies run only
	// under the lab's opts bits 256 / 4096.  The scratch copy's sys and
	// in-place bodies (burst_body<false, true>, burst_body<false> over
	// h.base) would need an in-place block above 8 KiB; it is 64 + 12 n.
	{"one/lds/inplace/g4u1/rt", false},    {"one/scratch/staged/g4u1/rt", false},
	{"one/scratch/sys/g4u1/rt", false},    {"one/scratch/sys/g16u1/rt", false},
	{"one/scratch/inplace/g4u1/rt", false}, {"one/scratch/inplace/g16u1/rt", false},
	{"one/scratch/inplace/g16u4/rt", false},
};
const size_t kRouteKindCount = sizeof kRouteKinds / sizeof kRouteKinds[0];

} // namespace cgck

extern "C" int cgck_test_burst_route(uint32_t max_pkts, size_t max_bytes, int mem, int posted, uint64_t n,
				     uint32_t max_len, uint64_t pkt_bytes, uint32_t flags, uint32_t n1, char *name,
				     size_t cap)
{
	if (!name || mem < cgck::kRoutePageable || mem > cgck::kRouteRequest)
		return -22; // -EINVAL
	const cgck::RouteIn in = {max_pkts, max_bytes, mem, posted != 0, n, max_len, (size_t)pkt_bytes, flags, n1};
	return cgck::route_name(cgck::burst_route(in), name, cap) < 0 ? -22 : 0;
}

extern "C" int cgck_test_burst_route_kind(uint32_t i, char *kind, size_t cap)
{
	if (i >= cgck::kRouteKindCount)
		return -2; // -ENOENT
	if (!kind || snprintf(kind, cap, "%s", cgck::kRouteKinds[i].kind) >= (int)cap)
		return -22;
	return cgck::kRouteKinds[i].product ? 1 : 0;
}
