// cgck_lane.hip — kernels whose per-packet work runs on ONE lane.
//
// The streaming rate of this path is VALU-issue-bound long before it is
// HBM-bound (tools/probe.py: ~300 extra VALU per 4 KiB halves a 64 B-packet
// stream), so per-packet work must run once per packet, not once per lane of
// a group, and must be cheap in the common cases.  The families, in order (the
// kernels that lost their A/B are in cgck_lane_lab.inc, for libcgck_lab.so only):
//
//  * lpp_kernel   — one lane per packet (small packets: every lane is a head).
//  * lpa_kernel, lpd_kernel (cgck_lane_kernels.inc; lpa6 / lpd6 for IPv6) — the
//    same for aligned fixed-length strided batches, by register or LDS-DMA ring.
//  * slot2_kernel — one lane per 128-byte SLOT: a packet of L bytes spans
//    ceil(chunks/8) consecutive lanes of a wave, so mixed sizes (IMIX) keep
//    every lane loading 8 chunks at once, large packets load coalesced
//    across lanes, and the per-packet work (header, finish) runs on the
//    packet's head lane only.  Slot partial sums are joined by a segmented
//    suffix reduction towards the head lane.
//  * lpw_kernel   — one lane per packet over DMA'd windows of a packed batch
//    (cgck_lpw_kernel.inc; cgck_lpw6.hip compiles it as lpw6_kernel for IPv6,
//    cgck_lpf.hip as lpf_kernel with the in-place stores and the bad counters,
//    cgck_lpwx.hip as lpwx_kernel with the family chosen per lane, CGCK_MIXED).
//
// Shared per-packet pieces:
//  * header(): the first 6 chunks realigned to packet-relative dwords
//    (v_bfi selects + v_alignbyte) — IP header sum, pseudo src/dst, ip_p and
//    both stored checksum fields, with wave-uniform fast paths (all packets
//    16-byte aligned / dword aligned / ip_hl == 5);
//  * edges: the bytes of the first/last chunk outside the packet are taken
//    out of the raw chunk sum (each chunk is read exactly once — a STORE batch
//    may rewrite a neighbour's header inside our last chunk);
//  * finish(): zero-field semantics by one's-complement subtraction, the
//    pseudo-header, reduce() (subr.c:137-156), verdicts, stores, outputs.
#include "cgck_lane.h"

#include <stdlib.h>
#include <optional>

namespace cgck {

// --------------------------------------------------------------------------
// Lane per packet
// --------------------------------------------------------------------------

template <bool DESC, bool NT, int S0, bool CLAMP>
__global__ __launch_bounds__(256) void lpp_kernel(KParams p)
{
	const bool raw = p.flags & CGCK_RAW;
	const Sched sc = sched((p.n + 255) / 256, p.contig);
	for (uint64_t it = sc.it; it < sc.end; it += sc.step) {
		const uint64_t k = it * 256 + threadIdx.x;
		const Pkt pk = get_pkt<DESC>(p, k);
		const uint64_t a0 = pk.a0;
		const int len = (int)pk.len, q = (int)(a0 & 15), nch = nchunks(a0, pk.len);
		const uint4 *c0 = reinterpret_cast<const uint4 *>(a0 & ~(uint64_t)15);
		// first S0 chunks: clamped and branch-free (precise vmcnt) or
		// predicated per lane (no duplicate loads)
		uint4 v[S0];
#pragma unroll
		for (int i = 0; i < S0; ++i)
			v[i] = CLAMP ? ldc<NT>(c0, i, nch, p.zero) : (i < nch ? ld<NT>(c0 + i) : make_uint4(0, 0, 0, 0));
		const bool more = __any(nch > S0);
		uint4 last = make_uint4(0, 0, 0, 0);
		if (CLAMP) {
			if (more)
				last = ldc<NT>(c0, nch - 1, nch, p.zero);
		} else {
			last = nch > S0 ? ld<NT>(c0 + nch - 1) : make_uint4(0, 0, 0, 0);
		}

		uint32_t tot = 0;
#pragma unroll
		for (int i = 0; i < S0; ++i)
			tot = i < nch ? sum4(v[i], tot) : tot;
		Hdr h{};
		if (!raw)
			h = header<S0, NT>(v, c0, nch, q, len, p.flags, pk.ok);
		if (more) {
			// chunks S0 .. nch-2 (the last one is `last`), 8 per step
			for (int t = S0; __any(t < nch - 1); t += 8) {
				uint4 w[8];
#pragma unroll
				for (int i = 0; i < 8; ++i)
					w[i] = t + i < nch - 1 ? ld<NT>(c0 + t + i) : make_uint4(0, 0, 0, 0);
				uint32_t s = 0;
#pragma unroll
				for (int i = 0; i < 8; ++i)
					s = sum4(w[i], s);
				tot = fold16(tot) + fold16(s);
			}
		}
		const bool dw = !__any(((q | len) & 3) != 0);
		if (__any(q != 0))
			tot = fold16(tot) + (0xffffu - fold16(lead_sum(v[0], q, dw)));
		const int e = q + len - 16 * (nch - 1); // bytes of the last chunk inside
		if (more)
			tot = fold16(tot) + fold16(nch > S0 ? sum4(last, 0) - trail_sum(last, e, dw) : 0u);
		if (__any(nch > 0 && nch <= S0 && e != 16)) {
			uint4 lc = make_uint4(0, 0, 0, 0);
#pragma unroll
			for (int i = 0; i < S0; ++i)
				if (i == nch - 1)
					lc = v[i];
			tot = fold16(tot) + (0xffffu - fold16(nch > 0 && nch <= S0 ? trail_sum(lc, e, dw) : 0u));
		}
		if (pk.ok)
			finish(p, k, a0, len, fold16(tot), h);
	}
}

// --------------------------------------------------------------------------
// Lane per packet, aligned fixed-length strided batches (the 64 B config)
// --------------------------------------------------------------------------
//
// Strided batch, base/stride/l3_off all multiples of 16 and one ip_len in
// [20, 64]: every packet is nch = ceil(len/16) whole chunks from a 16-byte
// boundary, the same for every lane.  Chunk loads are unconditional (index
// clamped to the last chunk, idle lanes to packet n-1), so no load sits in
// a branch and every wait is a counted vmcnt.  Two packet groups per lane
// are in flight (explicit A/B registers, no loop-carried copies): the
// chunks of group i+1 are issued before group i is reduced and its output
// stored, so each output store trails the next group's loads (vmcnt retires
// in order on gfx9).
struct Quad {
	uint4 c[4];
};

template <bool NT>
__device__ __forceinline__ void lpa_load(const KParams &p, uint64_t k, bool live, int nch, Quad &q)
{
	k = k < p.n ? k : p.n - 1;
	// past the block's last group: a zero line of the context, one of 64 by
	// block, instead of re-reading packet bytes that have left the L2
	const uint4 *c0 = live ? reinterpret_cast<const uint4 *>(p.base + k * p.stride + p.l3_off)
			       : reinterpret_cast<const uint4 *>((const uint8_t *)p.zero + (blockIdx.x & 63) * 64);
#pragma unroll
	for (int i = 0; i < 4; ++i)
		q.c[i] = ld<NT>(c0 + (i < nch ? i : nch - 1));
}

// Reduce packet k's quad and store its u32 output.  The store carries the
// nontemporal policy: +3 points of HBM peak in the slower of the two states a
// process lands in, +1.5 in the faster (tools/ab_lib.sh; the same policy on
// the group, slot and hash kernels' stores lost up to 13 points).  (A staged
// form — four results per lane leaving as one 16-byte store after an LDS
// transpose — measured 66.7 % vs 69.5 % of HBM peak on one box.)
// IP6 (lpa6_kernel, lpd6_kernel: CGCK_IP6 with IP / L4 only, lane6_ok): the
// frame's sum, the sum of its first 8 bytes and byte 6 go to v6_dense
// (cgck_device.h), the no-extension identity; a packet with extension headers
// is finished exactly by its lane from global memory.
template <bool NT, bool STAGE = false, bool IP6 = false>
__device__ __forceinline__ void lpa_reduce(const KParams &p, uint64_t k, int len, int nch, const Quad &q,
					   uint32_t *so = nullptr)
{
	const bool ok = k < p.n;
	if constexpr (IP6) {
		uint32_t T = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			// wave-uniform: whole chunks, then the last one's first len - 16 i bytes
			if (i < nch - 1 || (i == nch - 1 && (len & 15) == 0))
				T = sum4(q.c[i], T);
			else if (i == nch - 1)
				T = msum(q.c[i], 0, 0, len - 16 * i, T);
		}
		const uint32_t h8 = fold16(hsum(q.c[0].y, hsum(q.c[0].x, 0))), nh0 = (q.c[0].y >> 16) & 0xffu;
		// Fast path (wave-uniform): no packet of the wave has an extension or
		// Fragment header, so the identity applies as it stands and the finish
		// is straight-line code (v6_dense's walk and its loops cost the 64 B
		// reduce, which is issue-bound, 3-6 % against IPv4's fast path).
		const bool plain = len >= 40 && !__any(ok && (v6_is_ext(nh0) || nh0 == 44));
		if (ok) {
			const uint64_t a0 = reinterpret_cast<uint64_t>(p.base) + k * p.stride + p.l3_off;
			uint32_t bl = 0, out = 0;
			if (plain) {
				const int fo = v6_field(nh0);
				if (!(p.flags & CGCK_L4)) {
					// CGCK_IP alone: inert, 0
				} else if (fo >= 0 && 40 + fo + 2 > len) {
					bl = CGCK_BAD_LEN; // the checksum field does not fit
				} else {
					const uint32_t L = fold16(ocsub(fold16(T), h8) + (nh0 << 8) + bswap16((uint32_t)(len - 40)));
					out = finish(L) << 16;
				}
			} else {
				out = v6_dense(a0, len, fold16(T), h8, nh0, p.flags, &bl);
			}
			if (STAGE) {
				*so = out;
			} else if (p.out) {
				uint32_t *o = p.out + k;
				asm volatile("global_store_dword %0, %1, off nt" ::"v"(o), "v"(out) : "memory");
			}
			if (p.verdict)
				gbl(p.verdict)[k] = (uint8_t)bl;
		}
		return;
	}
	// Fast path (wave-uniform): ip_cksum + tcp_cksum only, whole chunks, and
	// every packet of the wave with ip_hl = 5 — the 64 B config.  IP header =
	// dwords 0..4, pseudo src/dst = dwords 3..4, ip_p = byte 9; the same
	// arithmetic as result() with no field, verdict or store work.
	if (p.flags == (CGCK_IP | CGCK_L4) && (len & 15) == 0 && !__any(ok && (q.c[0].x & 15u) != 5u)) {
		uint32_t T = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			if (i < nch)
				T = sum4(q.c[i], T);
		const uint32_t IPs = fold16(hsum(q.c[1].x, sum4(q.c[0], 0)));
		const uint32_t PS = fold16(hsum(q.c[1].x, hsum(q.c[0].w, 0)));
		const uint32_t proto = (q.c[0].z >> 8) & 0xffu;
		uint32_t L = ocsub(fold16(T), IPs);
		L = fold16(L + PS + (proto << 8) + bswap16((uint32_t)(len - 20)));
		if (ok) {
			const uint32_t out = finish(IPs) | (finish(L) << 16);
			if (STAGE) {
				*so = out;
			} else if (p.out) {
				uint32_t *o = p.out + k;
				asm volatile("global_store_dword %0, %1, off nt" ::"v"(o), "v"(out) : "memory");
			}
			if (p.verdict)
				gbl(p.verdict)[k] = 0;
		}
		return;
	}
	// chunks 4, 5 are zero: len <= 64 puts every header and L4-field dword
	// header() may read below dword 16, so it never loads more
	uint4 v[6];
	v[4] = v[5] = make_uint4(0, 0, 0, 0);
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		// wave-uniform: chunks past the packet drop out, the last one keeps
		// its first len - 16 i bytes
		const int r1 = i < nch - 1 ? 16 : (i == nch - 1 ? len - 16 * i : 0);
		v[i] = make_uint4(q.c[i].x & dmask(0, 0, 0, r1), q.c[i].y & dmask(0, 1, 0, r1),
				  q.c[i].z & dmask(0, 2, 0, r1), q.c[i].w & dmask(0, 3, 0, r1));
	}
	uint32_t tot = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i)
		tot = sum4(v[i], tot);
	const uint64_t a0 = reinterpret_cast<uint64_t>(p.base) + (ok ? k : 0) * p.stride + p.l3_off;
	Hdr h{};
	if (!(p.flags & CGCK_RAW))
		h = header<6, NT>(v, reinterpret_cast<const uint4 *>(a0), nch, 0, len, p.flags, ok);
	if (ok) {
		const Res r = result(p, a0, len, fold16(tot), h);
		if (p.out) {
			// The u32 output through inline asm: the compiler then does not
			// hold the next group's address/data registers (which it tends to
			// allocate onto this store's data VGPR) behind a vmcnt(0) for the
			// store.  Every vmcnt the compiler computes stays conservative: the
			// hidden store only makes in-order waits include it.
			if (STAGE) {
				*so = r.out;
			} else {
				uint32_t *o = p.out + k;
				asm volatile("global_store_dword %0, %1, off nt" ::"v"(o), "v"(r.out) : "memory");
			}
		}
		if (p.verdict)
			gbl(p.verdict)[k] = (uint8_t)r.verdict;
	}
}

#define CGCK_LPA_KERNEL lpa_kernel
#define CGCK_LPD_KERNEL lpd_kernel
#define CGCK_LANE_IP6 false
#include "cgck_lane_kernels.inc"
#undef CGCK_LPA_KERNEL
#undef CGCK_LPD_KERNEL
#undef CGCK_LANE_IP6
#define CGCK_LPA_KERNEL lpa6_kernel
#define CGCK_LPD_KERNEL lpd6_kernel
#define CGCK_LANE_IP6 true
#include "cgck_lane_kernels.inc"
#undef CGCK_LPA_KERNEL
#undef CGCK_LPD_KERNEL
#undef CGCK_LANE_IP6

// --------------------------------------------------------------------------
// Lane per 128-byte slot, software-pipelined two deep
// --------------------------------------------------------------------------
//
// The header's slot mapping, with TWO iterations of chunk loads in flight: while
// iteration i is reduced, the chunks of i+1 are loading and the descriptors of
// i+2 too.  In-order vmcnt retirement shapes the issue order of each phase:
//
//   map(i+1) [waits only for desc(i+1), issued before chunks(i)]
//   issue desc(i+2); issue chunks(i+1)
//   reduce(i) [waits for chunks(i): desc(i+2) + chunks(i+1) stay in flight]
//
// The A/B buffers are explicit (the loop body is unrolled twice) so no
// register holding an in-flight load is ever copied — a copy would force a
// vmcnt(0) at the back edge.  Every load is branch-free (clamped to the
// packet's chunks or the context's zero chunk) so vmcnt counting stays exact.

// One iteration's lane -> (packet, slot) mapping.
struct SMap {
	uint64_t a0;   // owner packet's IPv4 header (jumbo: lane 0's packet)
	int len, nch;  // owner packet
	int s;         // slot index inside the owner packet
	int st, ns;    // owner's first slot (lane) and slot count
	int owner;     // owner's packet index relative to the iteration
	int m;         // packets placed this iteration (0: jumbo or empty)
	bool act;      // lane holds a slot
};

template <bool DESC>
__device__ __forceinline__ SMap smap(const KParams &p, uint64_t cur, uint64_t r1, const DescW &d,
				     uint32_t (&mark)[64])
{
	const int l = threadIdx.x & 63;
	const Pkt pk = decode<DESC>(p, cur + l, r1, d);
	const int nch_l = nchunks(pk.a0, pk.len);
	const uint32_t ns = pk.ok ? (uint32_t)max(1, (nch_l + 7) >> 3) : 0u;
	const uint32_t P = wave_scan_dpp(ns);
	const uint64_t fit = __ballot(pk.ok && P <= 64);
	SMap M;
	M.m = __popcll(fit);
	const int T = M.m ? (int)__builtin_amdgcn_readlane(P, M.m - 1) : 0; // slots in use
	mark[l] = 0;
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
	if (l < M.m)
		mark[P - ns] = 1;
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
	const uint64_t heads = __ballot(mark[l] != 0 && l < T);
	const uint64_t le = l == 63 ? ~0ull : ((2ull << l) - 1);
	const uint64_t below = heads & le, above = heads & ~le;
	M.act = l < T;
	M.owner = below ? __popcll(below) - 1 : 0;
	M.st = below ? 63 - __clzll(below) : 0;
	M.ns = (above ? __ffsll((long long)above) - 1 : T) - M.st;
	M.s = l - M.st;
	M.a0 = shfl64(pk.a0, M.owner);
	M.len = __shfl((int)pk.len, M.owner, 64);
	M.nch = nchunks(M.a0, (uint32_t)M.len);
	return M;
}

template <bool NT>
__device__ __forceinline__ void slot_issue(const KParams &p, const SMap &M, uint4 (&w)[8])
{
	// Idle lanes (past the slots in use) clamp into the last placed packet's
	// final chunk, a line its own tail lane reads anyway: pointing them all
	// at the context's one zero chunk made every wave of the grid hit the
	// same address (one L2 channel).  Their chunks are excluded from sums.
	const uint4 *c0 = reinterpret_cast<const uint4 *>(M.a0 & ~(uint64_t)15);
#pragma unroll
	for (int i = 0; i < 8; ++i)
		w[i] = ldc<NT>(c0, 8 * M.s + i, M.nch, p.zero);
}

template <bool NT>
__device__ __forceinline__ void slot_reduce(const KParams &p, uint64_t cur, const SMap &M, uint4 (&w)[8],
					    WaveStage &ws)
{
	const int l = threadIdx.x & 63;
	const bool raw = p.flags & CGCK_RAW;
	const uint64_t a0 = M.a0;
	const int len = M.len, nch = M.nch, s = M.s;
	const int q = (int)(a0 & 15);
	const uint4 *c0 = reinterpret_cast<const uint4 *>(a0 & ~(uint64_t)15);
	// All of w[] counts as consumed here, on every path: a chunk whose use
	// sits in a skippable branch (or the jumbo path, which ignores w[]) would
	// leave its load "maybe pending" and degrade later waits to vmcnt(0).
#pragma unroll
	for (int i = 0; i < 8; ++i)
		asm volatile("" ::"v"(w[i].x), "v"(w[i].y), "v"(w[i].z), "v"(w[i].w));
	if (M.m == 0) {
		// jumbo packet (> 64 slots): windows of 64 slots, whole-wave sums
		const int nsj = (nch + 7) >> 3;
		uint32_t acc = 0;
		Hdr h{};
		for (int wbase = 0; wbase < nsj; wbase += 64) {
			const int sj = wbase + l;
			// the window reuses w[] (dead here) with clamped, branch-free loads
			uint4 (&v)[8] = w;
#pragma unroll
			for (int i = 0; i < 8; ++i)
				v[i] = ldc<NT>(c0, 8 * sj + i, nch, p.zero);
			uint32_t r = 0;
#pragma unroll
			for (int i = 0; i < 8; ++i)
				r = 8 * sj + i < nch ? sum4(v[i], r) : r;
			if (wbase == 0 && !raw)
				h = header<8, NT>(v, c0, nch, q, len, p.flags, l == 0);
			const int j = (nch - 1) - 8 * sj;
			const int e = q + len - 16 * (nch - 1);
			uint32_t corr = 0;
			if (sj == 0 && q != 0)
				corr += lead_sum(v[0], q, false);
			if (j >= 0 && j < 8 && e != 16)
				corr += trail_sum(pick8(v, j), e, false);
			r = fold16(r) + (0xffffu - fold16(corr));
			acc = fold16(acc) + fold16(gsum<64>(r));
		}
		wave_stage_reserve(p, ws, cur, 1);
		if (l == 0)
			wave_stage_put(ws, cur, result(p, a0, len, fold16(acc), h));
		// drain this rare path completely so the wait state merged after it
		// holds no "maybe pending" loads (they would cost a vmcnt(0) later)
		__builtin_amdgcn_s_waitcnt(0);
		return;
	}
	const bool act = M.act;
	uint32_t r = 0;
#pragma unroll
	for (int i = 0; i < 8; ++i)
		r = act && 8 * s + i < nch ? sum4(w[i], r) : r;
	const bool head = act && s == 0;
	Hdr h{};
	if (!raw)
		h = header<8, NT>(w, c0, nch, q, len, p.flags, head);
	const bool dw = !__any(act && ((q | len) & 3) != 0);
	uint32_t corr = 0;
	if (__any(head && q != 0))
		corr = head && q != 0 ? lead_sum(w[0], q, dw) : 0u;
	const int j = (nch - 1) - 8 * s;
	const int e = q + len - 16 * (nch - 1);
	const bool tail = act && nch > 0 && j >= 0 && j < 8 && e != 16;
	if (__any(tail))
		corr += tail ? trail_sum(pick8(w, j), e, dw) : 0u;
	r = fold16(r) + (0xffffu - fold16(corr));
	// segmented suffix sum towards the head lane
	uint32_t nso = 0; // wave-uniform bound on segment length (OR >= max)
#pragma unroll
	for (int b = 0; b < 7; ++b)
		nso |= __any(act && ((M.ns >> b) & 1)) ? (1u << b) : 0u;
	const int send = M.st + M.ns;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		if ((uint32_t)d >= nso)
			break;
		const uint32_t y = __shfl_down(r, d, 64);
		if (l + d < send)
			r += y;
	}
	wave_stage_reserve(p, ws, cur, M.m);
	if (head)
		wave_stage_put(ws, cur + M.owner, result(p, a0, len, fold16(r), h));
}

#if !CGCK_LAB || !defined(CGCK_SLOT2_CHUNK) // compile-time A/B knob of the lab build only
#undef CGCK_SLOT2_CHUNK
#define CGCK_SLOT2_CHUNK 0
#endif
template <bool DESC, bool NT>
__global__ __launch_bounds__(256) void slot2_kernel(KParams p)
{
	__shared__ uint32_t mark[4][64];
	__shared__ uint32_t so[4][kWaveStage];
	__shared__ uint8_t sv[4][kWaveStage];
	const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63; // wave-uniform (SGPR)
	const uint64_t nwaves = (uint64_t)gridDim.x * 4;
	const uint64_t wid = (uint64_t)blockIdx.x * 4 + wv;
#if CGCK_SLOT2_CHUNK
	// chunks of CGCK_SLOT2_CHUNK packets, grid-interleaved (A/B builds)
	for (uint64_t ck = wid; ck * CGCK_SLOT2_CHUNK < p.n; ck += nwaves) {
	const uint64_t r0 = ck * CGCK_SLOT2_CHUNK;
	const uint64_t r1 = r0 + CGCK_SLOT2_CHUNK < p.n ? r0 + CGCK_SLOT2_CHUNK : p.n;
#else
	const uint64_t per = (p.n + nwaves - 1) / nwaves;
	const uint64_t r0 = wid * per;
	const uint64_t r1 = r0 + per < p.n ? r0 + per : p.n;
	if (r0 >= r1)
		return;
#endif
	WaveStage ws{so[wv], sv[wv], r0};

	// prologue: map A, desc of B, chunks of A
	uint64_t curA = r0;
	SMap mA = smap<DESC>(p, curA, r1, load_desc<DESC>(p, curA + l, r1), mark[wv]);
	uint64_t curB = curA + (mA.m ? mA.m : 1);
	DescW dB = load_desc<DESC>(p, curB + l, r1);
	uint4 wA[8], wB[8];
	slot_issue<NT>(p, mA, wA);
	for (;;) {
		// phase A: map B, prefetch desc C, issue chunks B, reduce A
		const SMap mB = smap<DESC>(p, curB, r1, dB, mark[wv]);
		const uint64_t curC = curB + (mB.m ? mB.m : 1);
		const DescW dC = load_desc<DESC>(p, curC + l, r1);
		slot_issue<NT>(p, mB, wB);
		slot_reduce<NT>(p, curA, mA, wA, ws);
		if (curB >= r1)
			break;
		// phase B: map C, prefetch desc D, issue chunks C (into A), reduce B
		const SMap mC = smap<DESC>(p, curC, r1, dC, mark[wv]);
		const uint64_t curD = curC + (mC.m ? mC.m : 1);
		dB = load_desc<DESC>(p, curD + l, r1);
		slot_issue<NT>(p, mC, wA);
		slot_reduce<NT>(p, curB, mB, wB, ws);
		if (curC >= r1)
			break;
		curA = curC;
		mA = mC;
		curB = curD;
	}
	wave_stage_flush(p, ws, r1);
#if CGCK_SLOT2_CHUNK
	}
#endif
}

// --------------------------------------------------------------------------
// Lane per packet over DMA'd windows of the batch's own span (lpw: packed
// descriptor batches, the IMIX config under CGCK_LAYOUT_PACKED)
// --------------------------------------------------------------------------
//
// A step is 64 consecutive descriptors, one per lane.  When their chunk
// ranges chain (each packet starts at or after the starts before it and at
// or before the furthest end so far: frames back to back, as a burst copied
// into one buffer or the IMIX set), every chunk of the step's span [S, E)
// belongs to one of them.  The span is then streamed with contiguous DMA in
// windows of kLpwWin chunks through a 2-deep LDS ring; per window, a lane per
// chunk sums every chunk (conflict-free 16-byte LDS reads) and prefix-sums
// them in lane order, and a lane per packet takes its chunks' sum as a
// difference of two prefixes, minus the bytes of its edge chunks outside it;
// its header chunks are gathered in registers from whichever windows hold
// them and read once per step.  No slot map: a step's descriptors do not
// depend on the previous step, and they travel by DMA with the data (768 B,
// one instruction, into a 2-deep descriptor ring) two steps ahead, so no wait
// in the loop is on a compiler-tracked load; every round issues kLpwDma + 1
// DMA instructions (zero lines where there is nothing to move), so the waits
// are counted.  Steps that do not chain are computed from global memory by
// the same lanes (exact, slow): the layout hint says which batches chain.
// In one process on the 16M IMIX batch (tools/sweep.py,
// profiles/r02/dma/lpw/): 69.9 % of 8 TB/s against slot2's 63.8 %; windows of
// 7 / 9 / 10+ DMA instructions, fewer waves per CU, or the lane-per-packet walk
// of each window (21-23 %) lose.
// The kernel's text is cgck_lpw_kernel.inc, compiled here as lpw_kernel and in
// cgck_lpw6.hip as lpw6_kernel (CGCK_IP6: the same pipeline, an IPv6 finish)
// and in cgck_lpf.hip as lpf_kernel (CGCK_STORE and the bad counters) and in
// cgck_lpwx.hip as lpwx_kernel (CGCK_MIXED: the family chosen per lane).
#define CGCK_LPW_KERNEL lpw_kernel
#define CGCK_LPW_IP6 false
#define CGCK_LPW_FILL false
#define CGCK_LPW_MIXED false
#include "cgck_lpw_kernel.inc"
#undef CGCK_LPW_KERNEL
#undef CGCK_LPW_IP6
#undef CGCK_LPW_FILL
#undef CGCK_LPW_MIXED

// --------------------------------------------------------------------------
// Launchers
// --------------------------------------------------------------------------

template <bool DESC, int S0, bool CLAMP>
static hipError_t launch_lpp_t(const KParams &p, int max_blocks, bool nt, hipStream_t st)
{
	const unsigned blocks = grid_blocks(p.n, 256, max_blocks);
	if (nt) {
		CGCK_NOTE_KERNEL("lpp_kernel<%s, true, %d, %s>", tf(DESC), S0, tf(CLAMP));
		hipLaunchKernelGGL((lpp_kernel<DESC, true, S0, CLAMP>), dim3(blocks), dim3(256), 0, st, p);
	} else {
		CGCK_NOTE_KERNEL("lpp_kernel<%s, false, %d, %s>", tf(DESC), S0, tf(CLAMP));
		hipLaunchKernelGGL((lpp_kernel<DESC, false, S0, CLAMP>), dim3(blocks), dim3(256), 0, st, p);
	}
	return hipGetLastError();
}

#if CGCK_LAB // the A/B-only kernels, their launchers, the lab halves of the launchers below
#include "cgck_lane_lab.inc"
#endif

// shape: 0 = 4 chunks up front, clamped; 1 = 6 clamped; 2 = 6 predicated
// (the default, kDefaultLppShape; the only one in libcgck.so); 3 = 4 predicated
hipError_t launch_lpp(const KParams &p, int num_cus, bool nt, int shape, hipStream_t st)
{
	const int mb = num_cus * 8;
#if CGCK_LAB
	if (const auto lab = launch_lpp_lab(p, mb, nt, shape, st)) // shapes 0, 1, 3
		return *lab;
#endif
	return p.desc ? launch_lpp_t<true, 6, false>(p, mb, nt, st) : launch_lpp_t<false, 6, false>(p, mb, nt, st);
}

hipError_t launch_lpd(const KParams &p, int num_cus, hipStream_t st)
{
	static const int wpc = [] { // $CGCK_LPD_WPC: waves per CU
		const char *e = CGCK_ENV("CGCK_LPD_WPC");
		return e && atoi(e) > 0 ? atoi(e) : 8;
	}();
	const dim3 g(grid_blocks(p.n, 64 * 16, (uint64_t)num_cus * wpc)); // >= 16 steps per wave
	if (p.flags & CGCK_IP6) { // the product shape only
		CGCK_NOTE_KERNEL("lpd6_kernel<2, 32, 2>");
		hipLaunchKernelGGL((lpd6_kernel<2, 32, 2>), g, dim3(64), 2 * 4096 + 32 * 256, st, p);
		return hipGetLastError();
	}
#if CGCK_LAB
	if (const auto lab = launch_lpd_lab(p, g, num_cus, st)) // $CGCK_LPD_*: lpd_lc, lpdw, other lpd_kernel<D, C, SP>
		return *lab;
#endif
	CGCK_NOTE_KERNEL("lpd_kernel<2, 32, 2>");
	hipLaunchKernelGGL((lpd_kernel<2, 32, 2>), g, dim3(64), 2 * 4096 + 32 * 256, st, p);
	return hipGetLastError();
}

hipError_t launch_lpa(const KParams &p, int num_cus, bool nt, hipStream_t st)
{
	// One block per CU (one wave per SIMD) with four packet groups per lane in
	// flight: 68.8-69.1 % of HBM peak vs 66.2-66.4 % for two groups at 3 blocks
	// per CU and 67.9-68.7 % for three groups (tools/lpa_depth.sh, one box).
	// The per-packet reduce is short, so fewer waves with deeper register
	// rings keep more bytes in flight per instruction issued.
	static const int bpc = [] { // $CGCK_LPA_BPC: blocks per CU (A/B runs)
		const char *e = CGCK_ENV("CGCK_LPA_BPC");
		return e && atoi(e) > 0 ? atoi(e) : 1;
	}();
	static const int depth = [] { // $CGCK_LPA_DEPTH: packet groups per lane in flight, 2..4
		const char *e = CGCK_ENV("CGCK_LPA_DEPTH");
		const int d = e ? atoi(e) : 0;
		return d >= 2 && d <= 4 ? d : 4;
	}();
	uint64_t want = (p.n + 255) / 256, mb = (uint64_t)num_cus * bpc;
	const dim3 g((unsigned)(want < mb ? want : mb));
	if (p.flags & CGCK_IP6) { // the default depth only
		if (nt) {
			CGCK_NOTE_KERNEL("lpa6_kernel<true, 4>");
			hipLaunchKernelGGL((lpa6_kernel<true, 4>), g, dim3(256), 0, st, p);
		} else {
			CGCK_NOTE_KERNEL("lpa6_kernel<false, 4>");
			hipLaunchKernelGGL((lpa6_kernel<false, 4>), g, dim3(256), 0, st, p);
		}
		return hipGetLastError();
	}
#define CGCK_LPA(D)                                                                            \
	do {                                                                                   \
		if (nt) {                                                                      \
			CGCK_NOTE_KERNEL("lpa_kernel<true, %d>", D);                           \
			hipLaunchKernelGGL((lpa_kernel<true, D>), g, dim3(256), 0, st, p);      \
		} else {                                                                       \
			CGCK_NOTE_KERNEL("lpa_kernel<false, %d>", D);                          \
			hipLaunchKernelGGL((lpa_kernel<false, D>), g, dim3(256), 0, st, p);     \
		}                                                                              \
	} while (0)
	if (depth == 4)
		CGCK_LPA(4);
	else if (depth == 3)
		CGCK_LPA(3);
	else
		CGCK_LPA(2);
#undef CGCK_LPA
	return hipGetLastError();
}

template <bool DESC>
static hipError_t launch_slot2_t(const KParams &p, int max_blocks, bool nt, hipStream_t st)
{
	const unsigned blocks = grid_blocks(p.n, 4 * 64, max_blocks);
	if (nt) {
		CGCK_NOTE_KERNEL("slot2_kernel<%s, true>", tf(DESC));
		hipLaunchKernelGGL((slot2_kernel<DESC, true>), dim3(blocks), dim3(256), 0, st, p);
	} else {
		CGCK_NOTE_KERNEL("slot2_kernel<%s, false>", tf(DESC));
		hipLaunchKernelGGL((slot2_kernel<DESC, false>), dim3(blocks), dim3(256), 0, st, p);
	}
	return hipGetLastError();
}

hipError_t launch_slot2(const KParams &p, int num_cus, bool nt, hipStream_t st)
{
	// 8 blocks per CU requested; 41 KiB of LDS per block (the 2048-packet
	// output windows) keeps 3 resident per CU — 1984-packet windows (4
	// resident) and 3072 (2) measured the same.  $CGCK_BPC overrides the
	// blocks per CU for A/B runs.
	static const int bpc = [] {
		const char *e = CGCK_ENV("CGCK_BPC");
		return e && atoi(e) > 0 ? atoi(e) : 8;
	}();
	const int mb = num_cus * bpc;
	return p.desc ? launch_slot2_t<true>(p, mb, nt, st) : launch_slot2_t<false>(p, mb, nt, st);
}

hipError_t launch_lpw(const KParams &p, int num_cus, hipStream_t st)
{
	static const int wpc = [] { // $CGCK_LPW_WPC: waves per CU
		const char *e = CGCK_ENV("CGCK_LPW_WPC");
		return e && atoi(e) > 0 ? atoi(e) : 8;
	}();
	KParams q = p;
	q.contig = 0;
	const LpwShape sh = lpw_shape(p, num_cus, wpc, kLpwSlot);
#if CGCK_LAB
	if (const auto lab = launch_lpw_lab(p, q, sh.grid, sh.lds, num_cus, wpc, st)) // $CGCK_LPW_*: q.contig, C = 8, lpx, writer
		return *lab;
#endif
	if (p.desc) {
		CGCK_NOTE_KERNEL("lpw_kernel<true, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpw_kernel<true, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpw_kernel<false, %d, false>", kLpwC);
		hipLaunchKernelGGL((lpw_kernel<false, kLpwC, false>), sh.grid, dim3(64), sh.lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
