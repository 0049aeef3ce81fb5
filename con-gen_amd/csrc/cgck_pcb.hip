// cgck_pcb.hip — per-frame connection lookup (cgck_pcb_build, cgck_pcb_lookup:
// include/cgck.h section 3): in_pcblookup (bsd44/in_pcb.c:167-192; ip_socket_get,
// subr.c:580-596) over a tuple table the caller owns.  cgck_l4_desc's records and
// the frames' addresses go in, the connection index and the flow index that
// cgck_l4_build takes come out.  The table, the hash and every probe rule are
// cgck_pcb_probe.h's, which a CPU program compiles too; here are the two kernels
// and the accessor of global loads and atomics they probe through.
//
// pcbb_kernel: a lane per connection.  The lane reads its entry and its flow
// record, hashes the key and walks the slots from its home with
// pcb_insert_step: a plain (atomic, relaxed) read of the slot, a 64-bit
// compare-and-swap on a slot seen empty, an atomic min where the occupant has its
// key.  No lane waits for another: there is no spin loop and no flag, every loop
// ends after the table's slot count, and a workgroup never depends on another
// being resident.  The four counters of `stat` are sums over lanes of what each
// lane alone decides (it took a slot, it met its key, proto 0, a bad flow), so they
// do not depend on the order.  The kernel boundary on the stream is all the lookup
// needs to see the table.
//
// pcbl_kernel: cgck_frame.h's shape, a lane per frame, FrameCursor<4>: the 48
// frame-relative bytes the four chunks cover hold b[8..40) at any alignment.  The
// seg record's port dword and the class byte are fetched a step ahead with the
// chunks.  The probe loop runs behind a wave-wide __any: a step is the slot, on a
// tag match conn[j], then flow[conn[j].flow]'s flags and 32 address bytes.  idx,
// fidx and kind leave as a lane's own dword and byte stores (consecutive across
// the wave), the counters through the LDS histogram.
//
// TAG false is the A/B's other shape: 4-byte slots, a
// key fetch per occupied slot probed.
#include "cgck_frame.h"
#include "cgck_pcb_probe.h"

namespace cgck {

constexpr uint32_t kPcbBins = CGCK_PCB_NCOUNT;
constexpr int kPcbbThreads = 256;

// The accessor of cgck_pcb_probe.h over device memory.  RO: the lookup's, whose
// slot reads are plain loads of a table no one writes while it runs; the build
// reads a slot others may be taking with a relaxed atomic load.
template <bool RO>
struct PcbDev {
	const CGCK_GLOBAL uint32_t *conn_;
	const CGCK_GLOBAL u32x4_t *flow_;
	CGCK_GLOBAL uint64_t *t64;
	CGCK_GLOBAL uint32_t *t32;
	uint32_t nconn, nflow;

	__device__ __forceinline__ explicit PcbDev(const PcbTable &t)
		: conn_((const CGCK_GLOBAL uint32_t *)t.conn), flow_((const CGCK_GLOBAL u32x4_t *)t.flow),
		  t64((CGCK_GLOBAL uint64_t *)t.table), t32((CGCK_GLOBAL uint32_t *)t.table), nconn(t.nconn), nflow(t.nflow)
	{
	}
	__device__ __forceinline__ void conn(uint32_t j, uint32_t &flow, uint32_t &ports, uint32_t &w2) const
	{
		const CGCK_GLOBAL uint32_t *g = conn_ + 3 * (uint64_t)j;
		flow = g[0];
		ports = g[1];
		w2 = g[2];
	}
	__device__ __forceinline__ void flow_key(uint32_t f, uint32_t &flags, uint32_t (&a)[8]) const
	{
		const CGCK_GLOBAL u32x4_t *g = flow_ + 3 * (uint64_t)f;
		const uint32_t w3 = ((const CGCK_GLOBAL uint32_t *)g)[3];
		const u32x4_t l = g[1], r = g[2];
		flags = (w3 >> 16) & 255u;
		a[0] = l[0], a[1] = l[1], a[2] = l[2], a[3] = l[3];
		a[4] = r[0], a[5] = r[1], a[6] = r[2], a[7] = r[3];
	}
	__device__ __forceinline__ uint64_t slot64(uint32_t s) const
	{
		return RO ? t64[s] : __hip_atomic_load(t64 + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ uint32_t slot32(uint32_t s) const
	{
		return RO ? t32[s] : __hip_atomic_load(t32 + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ uint64_t cas64(uint32_t s, uint64_t v)
	{
		uint64_t seen = kPcbEmpty64;
		__hip_atomic_compare_exchange_strong(t64 + s, &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
						     __HIP_MEMORY_SCOPE_AGENT);
		return seen;
	}
	__device__ __forceinline__ uint32_t cas32(uint32_t s, uint32_t v)
	{
		uint32_t seen = kPcbNone;
		__hip_atomic_compare_exchange_strong(t32 + s, &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
						     __HIP_MEMORY_SCOPE_AGENT);
		return seen;
	}
	__device__ __forceinline__ void min64(uint32_t s, uint64_t v)
	{
		__hip_atomic_fetch_min(t64 + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ void min32(uint32_t s, uint32_t v)
	{
		__hip_atomic_fetch_min(t32 + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
};

template <bool TAG>
__global__ __launch_bounds__(kPcbbThreads) void pcbb_kernel(PcbbParams p)
{
	__shared__ uint32_t hist[4];
	frame_hist_zero(hist, 4);
	__syncthreads();
	const uint64_t i = (uint64_t)blockIdx.x * kPcbbThreads + threadIdx.x;
	if (i < p.t.nconn) {
		PcbDev<false> a(p.t);
		PcbKey key;
		uint32_t flow;
		const int st = pcb_conn_key(a, (uint32_t)i, key, flow);
		uint32_t bin = st == kPcbUnused ? 2u : 3u;
		if (st == kPcbValid) {
			const uint32_t h = pcb_hash(key), mask = p.t.mask;
			uint32_t s = pcb_home(h, mask, p.t.chain != 0);
			bin = 4; // no slot: impossible in a table of 2 nconn slots that this call initialised
			for (uint32_t it = 0; it <= mask; ++it) {
				const int r = pcb_insert_step<TAG>(a, (uint32_t)i, key, h, s);
				if (r != kPcbGo) {
					bin = r == kPcbPlaced ? 0u : 1u;
					break;
				}
				s = (s + 1) & mask;
			}
		}
		if (bin < 4)
			__hip_atomic_fetch_add(hist + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	}
	frame_hist_flush(hist, 4, p.stat);
}

// I: idx and / or fidx are written; X: kind and / or the counters.
template <bool I, bool X, bool TAG>
__global__ __launch_bounds__(kFrameThreads) void pcbl_kernel(PcblParams p)
{
	__shared__ uint32_t hist[kPcbBins];
	const bool count = X && p.count != nullptr;
	if (X) {
		frame_hist_zero(hist, kPcbBins);
		__syncthreads();
	}
	const FrameDescs src = {p.base, p.desc, p.n};
	FrameCursor<4, FrameDescs> cur(src, p.n, p.zero);
	const PcbDev<true> a(p.t);
	const uint32_t mask = p.t.mask;
	const CGCK_GLOBAL uint32_t *segw = (const CGCK_GLOBAL uint32_t *)p.seg;
	const CGCK_GLOBAL uint8_t *clsb = (const CGCK_GLOBAL uint8_t *)p.cls;
	// the record's ports (sport | dport << 16) and the class nibble of frame k, index clamped as frame_desc's
	auto fetch = [&](uint64_t k, uint32_t &sp, uint32_t &cb) {
		const uint64_t kk = k < p.n ? k : p.n - 1;
		sp = segw[8 * kk + 4];
		cb = clsb ? clsb[kk] & 15u : (uint32_t)CGCK_SEG_TCP;
	};
	if (cur.more()) {
		uint32_t sp, cb, spn, cbn;
		cur.start();
		fetch(cur.k(), sp, cb);
		for (; cur.more(); cur.advance(), sp = spn, cb = cbn) {
			cur.ahead();
			fetch((cur.s + cur.W) * 64 + cur.lane, spn, cbn);
			const uint64_t k = cur.k();
			const bool ok = k < p.n;
			const uint32_t len = cur.len;
			uint32_t R[12]; // the frame's bytes [0, 48)
			frame_realign(cur.c.c, (uint32_t)(cur.a0 & 15), R);

			// rules 1 and 2
			const uint32_t v = (R[0] & 255u) >> 4;
			const bool l4 = cb == CGCK_SEG_TCP || cb == CGCK_SEG_UDP, six = v == 6;
			const bool ip = len != 0 && ((v == 4 && len >= 20) || (six && len >= 40));
			uint32_t kind = !l4 ? (uint32_t)CGCK_PCB_SKIP : !ip ? (uint32_t)CGCK_PCB_NONE : (uint32_t)CGCK_PCB_MISS;

			// rule 3: in_pcblookup(proto, ip_dst, dport, ip_src, sport)
			PcbKey key;
			key.a[0] = six ? R[6] : R[4];
			key.a[4] = six ? R[2] : R[3];
#pragma unroll
			for (int i = 1; i < 4; ++i) {
				key.a[i] = six ? R[6 + i] : 0u;
				key.a[4 + i] = six ? R[2 + i] : 0u;
			}
			key.ports = sp >> 16 | sp << 16;
			key.fp = (six ? 1u : 0u) | (cb == CGCK_SEG_UDP ? 17u : 6u) << 8;
			const uint32_t h = pcb_hash(key);
			uint32_t s = pcb_home(h, mask, p.t.chain != 0);
			uint32_t idx = kPcbNone, flow = kPcbNone;
			bool active = ok && kind == CGCK_PCB_MISS && p.t.nconn != 0;
			for (uint32_t it = 0; __any(active); ++it) {
				if (active) {
					const int r = pcb_probe_step<TAG>(a, key, h, s, idx, flow);
					if (r == kPcbHit)
						kind = CGCK_PCB_HIT;
					s = (s + 1) & mask;
					active = r == kPcbGo && it < mask; // at most mask + 1 steps
				}
			}
			// rule 4: a listening socket on a port below EPHEMERAL_MIN (in_pcb.c:186-188)
			if (kind == CGCK_PCB_MISS && p.bound != nullptr) {
				const uint32_t port = bswap16(sp >> 16);
				if (port < (uint32_t)CGCK_PCB_NBOUND) {
					const uint32_t b = ((const CGCK_GLOBAL uint32_t *)p.bound)[port];
					if (b != kPcbNone) {
						kind = CGCK_PCB_BOUND;
						idx = b;
					}
				}
			}
			const bool hit = kind == CGCK_PCB_HIT;
			if (I && ok) {
				if (p.idx)
					((CGCK_GLOBAL uint32_t *)p.idx)[k] = idx;
				if (p.fidx)
					((CGCK_GLOBAL uint32_t *)p.fidx)[k] = hit ? flow : kPcbNone;
			}
			if (X && ok) {
				if (p.kind)
					((CGCK_GLOBAL uint8_t *)p.kind)[k] = (uint8_t)kind;
				if (count) {
					__hip_atomic_fetch_add(hist + kind, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					if (hit && six)
						__hip_atomic_fetch_add(hist + 5, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
		}
	}
	if (X)
		frame_hist_flush(hist, kPcbBins, p.count);
}

hipError_t launch_pcbb(const PcbbParams &p, bool tagged, hipStream_t st)
{
	const size_t bytes = ((size_t)p.t.mask + 1) * (tagged ? 8 : 4);
	hipError_t e = hipMemsetAsync(p.t.table, 0xFF, bytes, st);
	if (e == hipSuccess && p.stat != nullptr)
		e = hipMemsetAsync(p.stat, 0, 4 * sizeof(uint32_t), st);
	if (e != hipSuccess || p.t.nconn == 0)
		return e;
	const dim3 g((p.t.nconn + kPcbbThreads - 1) / kPcbbThreads), b(kPcbbThreads);
	if (tagged) {
		CGCK_NOTE_KERNEL("pcbb_kernel<true>");
		hipLaunchKernelGGL((pcbb_kernel<true>), g, b, 0, st, p);
	} else {
		CGCK_NOTE_KERNEL("pcbb_kernel<false>");
		hipLaunchKernelGGL((pcbb_kernel<false>), g, b, 0, st, p);
	}
	return hipGetLastError();
}

hipError_t launch_pcbl(const PcblParams &p, bool tagged, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool i = p.idx != nullptr || p.fidx != nullptr, x = p.kind != nullptr || p.count != nullptr;
#define CGCK_PCBL(Ii, Xx)                                                                  \
	do {                                                                               \
		if (tagged) {                                                              \
			CGCK_NOTE_KERNEL("pcbl_kernel<%s, %s, true>", tf(Ii), tf(Xx));     \
			hipLaunchKernelGGL((pcbl_kernel<Ii, Xx, true>), g, b, 0, st, p);   \
		} else {                                                                   \
			CGCK_NOTE_KERNEL("pcbl_kernel<%s, %s, false>", tf(Ii), tf(Xx));    \
			hipLaunchKernelGGL((pcbl_kernel<Ii, Xx, false>), g, b, 0, st, p);  \
		}                                                                          \
	} while (0)
	if (i && x)
		CGCK_PCBL(true, true);
	else if (i)
		CGCK_PCBL(true, false);
	else
		CGCK_PCBL(false, true);
#undef CGCK_PCBL
	return hipGetLastError();
}

} // namespace cgck
