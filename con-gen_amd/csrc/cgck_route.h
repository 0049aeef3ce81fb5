// cgck_route.h — which body of the burst server serves a host-resident
// request: the constants and predicates the host (cgck_api.cpp, cgck_burst.cpp) and the server
// kernel (cgck_group.hip) decide by, each written once here, and burst_route(),
// which names the route from the same text.  No HIP: <stdint.h>, <stddef.h>
// and the public header, so the whole table is tested on the CPU
// (cgck_route.cpp, cgck_test_burst_route, tests/test_server_routes_cpu.py).
// Part of cgck_internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cgck.h"

// CGCK_HD: callable from the kernels; CGCK_HDI: and always inlined there, as
// the expressions these predicates replaced were (the server kernel's
// instruction stream is the one it had with them written out).
#ifdef __HIP__
#define CGCK_HD __host__ __device__
#define CGCK_HDI __host__ __device__ __attribute__((always_inline))
#else
#define CGCK_HD
#define CGCK_HDI
#endif

namespace cgck {

constexpr uint32_t kBurstMaxWG = 32; // workgroups of a server (K)
constexpr uint32_t kBurstOneWG = 64; // packets one workgroup serves alone (one wide read of the block)
constexpr uint32_t kBurstPerWG = 64; // packets per workgroup of a wider request (default)

// Workgroups that serve a request of n packets on a server of K with `per`
// packets per workgroup: one up to kBurstOneWG packets (it reads the whole
// small block in one round trip), then one per `per` packets, at most K.
// A wide request's packet reads over the fabric are bound by the device's
// aggregate host-read rate, not by one CU: 2048 x 64 B in place took 25.3 /
// 31.2 / 44.4 / 43.9 us at 64 / 32 / 16 / 8 packets per workgroup
// (tools/srvlat, profiles/r03/burst/srvlat_per_wg.log), so 64 it is.
CGCK_HD constexpr uint32_t burst_wgs(uint32_t n, uint32_t K, uint32_t per)
{
	return n <= kBurstOneWG ? 1u : ((n + per - 1) / per < K ? (n + per - 1) / per : K);
}

constexpr uint32_t kBurstReqBytes = 64; // sizeof(BurstReq), cgck_internal.h
// A one-workgroup request's first read, and the largest block that stays in LDS.
constexpr uint32_t kBurstFirst = 8192;
// Descriptors of one slice pass staged in LDS (12 KiB): a slice of more
// packets runs in passes.
constexpr uint32_t kSliceLds = 1024;

// ---- the server kernel's choices (burst_server_kernel, burst_part)

// A one-workgroup request's block stays in LDS (descriptors and staged bytes
// are read from there); a larger one is copied into device scratch.
CGCK_HDI constexpr bool burst_in_lds(uint32_t block_bytes) { return block_bytes <= kBurstFirst; }

// The lane shape: 4 lanes a packet up to 80 bytes (<= 6 chunks at any
// alignment: two steps of 4 lanes), 16 lanes above.
CGCK_HDI constexpr bool burst_g4(uint32_t max_len) { return max_len <= 80; }

// A part the block covers in one pass with one packet per group (64 groups
// of 4 lanes, 16 of 16) runs unrolled once, else four packets per group.
CGCK_HDI constexpr bool burst_u1(bool g4, uint32_t count) { return g4 ? count <= 64 : count <= 16; }

// Can a one-workgroup request of n packets read its packet bytes in place
// with the system-coherent body?  One packet per lane group must cover each
// part in one pass (64 groups of 4 lanes up to 80 bytes, 16 of 16 lanes
// above), with every packet within the body's S * G chunks (1536 bytes).
CGCK_HDI constexpr bool burst_sys_ok(uint32_t max_len, uint32_t n)
{
	return max_len <= 80 ? n <= 64 : (n <= 16 && max_len <= 1520);
}

// Workgroup j of W serves packets [burst_slice_at(n, j, W), burst_slice_at(n, j + 1, W)).
CGCK_HDI constexpr uint32_t burst_slice_at(uint32_t n, uint32_t j, uint32_t W) { return (uint32_t)((uint64_t)n * j / W); }

// The end of the slice pass that starts at c0.
CGCK_HDI constexpr uint32_t burst_pass_end(uint32_t c0, uint32_t hi) { return hi - c0 < kSliceLds ? hi : c0 + kSliceLds; }

// ---- the host's choices (desc_host_impl, cgck_burst_request, cgck_burst_open)

constexpr uint64_t kServerPktsDefault = 1u << 20; // packets a request may hold
constexpr size_t kServerCopyDefault = 32 << 10;    // registered packets are copied into the block up to here

// Offsets in the request block of n descriptors and `staged` packet bytes
// copied into it (0: read in place).
struct BurstLayout {
	size_t d_off, p_off, bytes;
};

inline BurstLayout burst_layout(size_t staged, uint64_t n)
{
	BurstLayout L;
	L.d_off = kBurstReqBytes;
	L.p_off = (L.d_off + 12 * n + 15) & ~(size_t)15;
	L.bytes = L.p_off + staged;
	return L;
}

// Bytes of one request slot of a server opened for max_pkts packets and
// max_bytes packet bytes: the header, the descriptors and the packet bytes,
// each packet padded to 16; the server's first read fetches kBurstFirst bytes
// whatever the request.
inline size_t burst_stage_cap(uint32_t max_pkts, size_t max_bytes)
{
	size_t cap = burst_layout(((max_bytes + 15) & ~(size_t)15) + 16 * (size_t)max_pkts, max_pkts).bytes;
	return (cap < kBurstFirst ? kBurstFirst : cap + 15) & ~(size_t)15;
}

// Does cgck_desc_host read the packets where they lie?  Only registered
// memory (dev: it has a device view), and then when the request stores in
// place, is posted, or its block would exceed one wide read (server_copy).
inline bool burst_in_place(bool dev, bool store, bool posted, size_t pkt_bytes, uint64_t n, size_t server_copy)
{
	return dev && (store || posted || burst_layout(pkt_bytes, n).bytes > server_copy);
}

// The server's bodies are IPv4, and its copy of staged bytes is not written back.
inline bool burst_flags_ok(uint32_t flags, bool in_place)
{
	return !(flags & (CGCK_IP6 | CGCK_MIXED)) && (in_place || !(flags & CGCK_STORE));
}

// Does a request of n packets, `data` packet bytes of which `staged` are
// copied into the block (0 when read in place), fit a server of bmax packets,
// bmax_bytes packet bytes and stage_cap bytes a slot?
inline bool burst_fits_caps(uint64_t bmax, uint64_t server_pkts, size_t stage_cap, size_t bmax_bytes, uint64_t n,
			    size_t staged, size_t data)
{
	return n <= bmax && n <= server_pkts && burst_layout(staged, n).bytes <= stage_cap && data <= bmax_bytes;
}

// ---- the route

enum RouteMem : int {
	kRoutePageable = 0,   // cgck_desc_host on memory without a device view
	kRouteRegistered = 1, // cgck_desc_host on registered memory
	kRouteRequest = 2,    // cgck_burst_request over a device view: always in place
};

struct RouteIn {
	uint32_t max_pkts; // cgck_burst_open's caps
	size_t max_bytes;
	int mem;           // RouteMem
	bool posted;       // a posted request (the pipelined windows)
	uint64_t n;
	uint32_t max_len;   // the longest ip_len
	size_t pkt_bytes;   // the packets' bytes, each padded to 16 (what a staged block holds)
	uint32_t flags;     // as the library posts them (BurstReq.flags)
	uint32_t n1;        // 0 < n1 < n: a two-part request (BurstReq.n1)
};

enum class RouteLoc : int { kLaunch, kRefused, kLds, kScratch, kSlice };
enum class RouteBody : int { kSys, kLdsp, kStaged, kInPlace };

struct Route {
	RouteLoc loc;   // kLaunch: the launch path; kRefused: cgck_burst_request fails; else where the block is read
	bool in_place;  // the packet bytes are read where they lie
	uint32_t W;     // workgroups that serve the request
	RouteBody body;
	int G;          // lanes a packet: 4 or 16
	int u_mask;     // 1: a part ran unrolled once (U = 1), 2: four times (U = 4)
	uint32_t passes; // the most slice passes of one workgroup (1 outside slices)
	bool fl;        // the body compiled for the request's flag set runs (burst_body_spec)
};

Route burst_route(const RouteIn &in);
// "launch", "refused", "one/lds/sys/g16u1/fl", "wide32/slice/inplace/g4u4+u1/rt/2passes"; the
// bytes written (without the NUL), or -1 when `cap` is too small.
int route_name(const Route &r, char *name, size_t cap);

// Every body a route name can stand for, by its kind: the name with W and the
// pass count left out and one U a kind ("wide/slice/staged/g16u4/rt"; a slice
// that ran in passes also "wide/slice/staged/passes").  product: a request to
// the product library reaches it.
struct RouteKind { const char *kind; bool product; };
extern const RouteKind kRouteKinds[];
extern const size_t kRouteKindCount;

} // namespace cgck
