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
//  * lpw_kernel   — one lane per packet over DMA'd windows of a packed batch.
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
#if !CGCK_LAB || !defined(CGCK_LPW_DMA) // compile-time A/B knobs of the lab build only
#undef CGCK_LPW_DMA
#define CGCK_LPW_DMA 8
#endif
// 0: instruction i moves chunks [64 i, 64 i + 64) of the window (1 KiB
// contiguous); 1: lane l moves chunks [8 l, 8 l + 8) over the 8 instructions,
// so its own run lands in conflict-free LDS places (A/B builds)
#if !CGCK_LAB || !defined(CGCK_LPW_SLOTMAJOR)
#undef CGCK_LPW_SLOTMAJOR
#define CGCK_LPW_SLOTMAJOR 0
#endif
// 1: the window's prefix with a lane per pair of chunks (4 wave scans a
// window), 0: a lane per chunk (8) — the A/B builds' knob
#if !CGCK_LAB || !defined(CGCK_LPW_PAIR)
#undef CGCK_LPW_PAIR
#define CGCK_LPW_PAIR 1
#endif
// LDS index (in 16-byte units) of window chunk idx
__device__ __forceinline__ int lpw_at(int idx)
{
#if CGCK_LPW_SLOTMAJOR
	return ((idx & 7) << 6) | (idx >> 3);
#else
	return idx;
#endif
}
constexpr int kLpwDma = CGCK_LPW_DMA;            // data DMA instructions per window
constexpr int kLpwWin = kLpwDma * 64;            // chunks a window owns (no overlap: a header
						 // split over two windows is gathered from both)
constexpr int kLpwSlot = kLpwDma * 1024;         // bytes per ring slot

struct LpwStep {
	uint64_t a0;
	int len, q, nch, e;
	bool ok;
	uint64_t cs, ce; // the lane's packet in window coordinates: absolute chunks (chained) or list positions
	uint64_t dl;     // gathered: (a0 >> 4) - cs, the chunk address of list position x is dl + x
	uint64_t S, E;   // wave: span
	uint32_t nwin;   // wave: windows (0: computed from global memory)
	bool gather;     // wave: the windows are the packets' chunk runs concatenated in lane order
};

template <bool DESC>
__device__ __forceinline__ LpwStep lpw_step(const KParams &p, uint64_t first, const DescW &d)
{
	const int l = threadIdx.x & 63;
	const Pkt pk = decode<DESC>(p, first + l, p.n, d);
	LpwStep s;
	s.a0 = pk.a0;
	s.len = (int)pk.len;
	s.ok = pk.ok;
	s.q = (int)(pk.a0 & 15);
	s.nch = nchunks(pk.a0, pk.len);
	s.e = s.q + s.len - 16 * (s.nch - 1);
	s.cs = pk.a0 >> 4;
	s.ce = s.cs + (uint64_t)s.nch;
	// Over the non-empty packets in lane order: running maxima of the starts
	// and of the ends (inclusive DPP scans of 32-bit offsets from the first
	// non-empty packet, then shifted by one lane).  The step chains when every
	// start is >= the starts before it and <= the furthest end before it: then
	// [S, E) is exactly the union of the packets' chunks.
	const bool ne = s.ok && s.nch > 0;
	const uint64_t nonempty = __ballot(ne);
	const int f = nonempty ? __ffsll((long long)nonempty) - 1 : 0; // first non-empty lane
	// the wave's values (base, span, windows) by readlane: scalar, so the
	// window loop and the round bookkeeping (pre, pend, sage) stay uniform
	// branches instead of exec-masked ones
	const uint64_t base = readlane64(s.cs, f);
	const uint64_t ds = s.cs - base, de = s.ce - base;
	const bool far = ne && (s.cs < base || de > 0x7fffffffull); // before the first, or too far for 32 bits
	const uint32_t rs = ne && !far ? (uint32_t)ds : 0u, re = ne && !far ? (uint32_t)de : 0u;
	const uint32_t mS = wave_max_scan_dpp(rs), mE = wave_max_scan_dpp(re);
	const uint32_t prev_s = (uint32_t)__shfl_up((int)mS, 1, 64), prev_e = (uint32_t)__shfl_up((int)mE, 1, 64);
	const bool brk = far || (ne && l > f && (rs < prev_s || rs > prev_e));
	s.S = nonempty ? base : 0;
	s.E = nonempty ? base + (uint64_t)__builtin_amdgcn_readlane(mE, 63) : 0;
	s.dl = 0;
	s.gather = false;
	const uint64_t span = s.E - s.S;
	if (!__any(brk) && span <= 16 * kLpwWin) {
		s.nwin = span ? (uint32_t)((span + kLpwWin - 1) / kLpwWin) : 1u; // (empty packets: one window, nothing moved)
	} else {
		// Not back to back (ring slots, gaps, reordered frames): the windows
		// walk the list of the packets' chunk runs concatenated in lane order,
		// packet p at list positions [P_p, P_p + nch_p) (an exclusive scan of
		// the chunk counts), gathered by the same DMA (lpw_issue).  The
		// per-window work is unchanged in list coordinates.
		const uint32_t nc = ne ? (uint32_t)s.nch : 0u;
		const uint32_t incl = wave_scan_dpp(nc);
		const uint32_t T = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
		s.cs = incl - nc;
		s.ce = incl;
		s.dl = (pk.a0 >> 4) - s.cs;
		s.S = 0;
		s.E = T;
		s.gather = true;
		s.nwin = T > 16 * kLpwWin ? 0u : T ? (T + kLpwWin - 1) / kLpwWin : 1u;
	}
	s.nwin = __builtin_amdgcn_readfirstlane(s.nwin);
	return s;
}

// One round: window t of step s (live) or zero lines, plus the descriptors
// of step dstep (when dlive) into the descriptor slot.  A gathered step
// (gather) maps each list position of the window to its packet's chunk: the
// packets starting in the window mark their position in an owner table built
// in the target slot itself (free until this round's DMA lands; every row's
// address is computed before the first DMA is issued), a max-scan per row of 64
// positions fills the table forward, the row's carry is the last packet that
// started before it (a ballot), and the chunk address is that packet's dl
// (staged next to the table) plus the position.
template <bool DESC>
__device__ __forceinline__ void lpw_issue(const KParams &p, uint64_t wb, uint64_t E, bool live, bool gather,
					  uint64_t cs, uint64_t ce, uint64_t dl, uint8_t *slot, uint32_t lds_slot,
					  uint64_t dfirst, bool dlive, uint32_t lds_dslot, const uint8_t *zero)
{
	// window [wb, wb + 512) of a span ending at E (values, not a step
	// reference: selecting between two steps' structs put them in scratch)
	const int l = threadIdx.x & 63;
	const uint32_t base = __builtin_amdgcn_readfirstlane(lds_slot); // wave-uniform: M0
	if (gather && live) {
		uint32_t *own = reinterpret_cast<uint32_t *>(slot);       // kLpwWin entries: owner lane + 1, 0 none
		uint64_t *dls = reinterpret_cast<uint64_t *>(slot + 4 * kLpwWin); // 64 lanes' dl
		// one element type for the table, and memory clobbers between the
		// phases: the reads must not move above the zeroing or the marks (the
		// slot holds the last window's packet bytes until it is cleared)
#pragma unroll
		for (int r = 0; r < kLpwDma; ++r)
			own[64 * r + l] = 0u;
		asm volatile("" ::: "memory");
		const bool ne = ce > cs;
		if (ne && cs >= wb && cs < wb + kLpwWin)
			own[cs - wb] = (uint32_t)l + 1;
		dls[l] = dl;
		asm volatile("" ::: "memory");
		// every row's address first: row i's DMA lands on bytes [1024 i, 1024 i
		// + 1024) of the slot, over the table the later rows read
		const void *src[kLpwDma];
#pragma unroll
		for (int i = 0; i < kLpwDma; ++i) {
			const uint64_t x = wb + 64 * i + l;
			const uint64_t before = __ballot(ne && cs < wb + 64 * i); // packets started before this row
			const int carry = before ? 64 - __builtin_clzll(before) : 0; // last such lane + 1
			const uint32_t m = wave_max_scan_dpp(own[64 * i + l]);
			const int o = (int)(m > (uint32_t)carry ? m : (uint32_t)carry) - 1;
			const uint64_t d = dls[o > 0 ? o : 0];
			src[i] = x < E ? reinterpret_cast<const void *>((d + x) << 4) : zero;
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the table is read: the slot may be refilled
#pragma unroll
		for (int i = 0; i < kLpwDma; ++i)
			glds16_nt(src[i], base + 1024 * i);
	} else {
#pragma unroll
		for (int i = 0; i < kLpwDma; ++i) {
#if CGCK_LPW_SLOTMAJOR
			const uint64_t c = wb + 8 * l + i; // lane l's 8 chunks land at +16 l of each KiB
#else
			const uint64_t c = wb + 64 * i + l;
#endif
			glds16_nt(live && c < E ? reinterpret_cast<const void *>(c << 4) : zero, base + 1024 * i);
		}
	}
	const uint64_t doff = 12 * dfirst + 16 * (uint64_t)l;
	const bool dok = DESC && dlive && l < 48 && doff < 12 * p.n;
	glds16_nt(dok ? reinterpret_cast<const void *>(reinterpret_cast<const uint8_t *>(p.desc) + doff) : zero,
		  __builtin_amdgcn_readfirstlane(lds_dslot));
}

template <bool DESC>
__device__ __forceinline__ DescW lpw_desc_lds(const uint8_t *dslot)
{
	DescW d{0, 0, 0};
	if (DESC) {
		const uint32_t *q = reinterpret_cast<const uint32_t *>(dslot) + 3 * (threadIdx.x & 63);
		d.lo = q[0];
		d.hi = q[1];
		d.w2 = q[2];
	}
	return d;
}

template <bool DESC, int C, bool W>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(W ? 4 : 1))) void lpw_kernel(KParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	uint8_t *dring = smem + 2 * kLpwSlot; // 2 x 1 KiB descriptor slots (64 lanes x 16 B; 768 B used)
	uint32_t *so = reinterpret_cast<uint32_t *>(dring + 2 * 1024);
	uint8_t *sv = reinterpret_cast<uint8_t *>(so + C * 64);
	const int l = threadIdx.x & 63;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	const uint32_t ldsd = lds0 + 2 * kLpwSlot;
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t NS = (p.n + 63) / 64, NC = (NS + C - 1) / C, G = gridDim.x, b = blockIdx.x;
	if (b >= NC)
		return;
	const uint64_t nsteps = (NC - b + G - 1) / G * C;
	auto gstep = [&](uint64_t j) { return (b + (j / C) * G) * C + j % C; };
	auto first_of = [&](uint64_t j) { return j < nsteps ? gstep(j) * 64 : p.n; };

	if (W && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 1) {
		// The writer wave (as dstr_kernel's): wave 0 stages a chunk's outputs
		// and verdicts and hands them over at barrier H; this wave reads them
		// into registers, releases the staging at barrier R (wave 0 meets it
		// just before its first staging write of the next chunk) and stores
		// them, so no output store sits in wave 0's in-order vmcnt (IMIX: the
		// flush alone cost 3-7 points, profiles/r02/imix/README.md).
		const uint64_t KD = nsteps / C;
		for (uint64_t k = 0; k < KD; ++k) {
			wg_barrier(); // H_k
			const uint64_t f0 = gstep(k * C) * 64;
			const uint64_t cntp = f0 < p.n ? (p.n - f0 < (uint64_t)C * 64 ? p.n - f0 : (uint64_t)C * 64) : 0;
			uint32_t vo[C];
			uint8_t vv[C];
#pragma unroll
			for (int i = 0; i < C; ++i) {
				vo[i] = so[64 * i + l];
				vv[i] = p.verdict ? sv[64 * i + l] : 0;
			}
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			if (k + 1 < KD)
				wg_barrier(); // R_k: the staging is free
#pragma unroll
			for (int i = 0; i < C; ++i) {
				if ((uint64_t)(64 * i + l) < cntp) {
					if (p.out)
						gbl(p.out)[f0 + 64 * i + l] = vo[i];
					if (p.verdict)
						gbl(p.verdict)[f0 + 64 * i + l] = vv[i];
				}
			}
		}
		return;
	}

	LpwStep cur = lpw_step<DESC>(p, first_of(0), load_desc<DESC>(p, first_of(0) + l, p.n));
	LpwStep nxt = lpw_step<DESC>(p, first_of(1), load_desc<DESC>(p, first_of(1) + l, p.n));
	LpwStep nn = nxt;
	uint32_t kiss = 0;      // rounds issued (round k uses data slot k & 1)
	// A full chunk's outputs leave as one 16-byte store per lane (C = 4: 256
	// outputs) issued right AFTER the next DMA round, whose wait then leaves
	// it in flight (vmcnt + 1): the store has a whole round to complete before
	// a wait must cover it.  Stored at the end of its chunk instead (in front
	// of the next round in the in-order vmcnt), the flush cost IMIX 3-7 points
	// (profiles/r02/imix/README.md).  Lab mode 6: the end-of-chunk flush.
	static_assert(C % 4 == 0, "C / 4 16-byte stores per lane per chunk");
	const bool defer_ok = !W && p.out && !p.verdict && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 &&
			      p.contig != 6 && p.contig != 5;
	bool pend = false; // a chunk's outputs wait in the staging for the next round
	int sage = 0;      // waits left that may leave the chunk store in flight
	uint64_t pf0 = 0;  // its first packet
	bool pre = false;       // cur's window 0 (with step j + 2's descriptors) already issued
	for (uint64_t j = 0; j < nsteps; ++j) {
		const uint64_t first = first_of(j);
		uint32_t acc = 0, corr = 0;
		Hdr h{};
		if (first < p.n && cur.nwin > 0) {
			// the header's chunks, loop-carried in native vectors (an array of
			// uint4, a union type, was put in scratch)
			u32x4_t t8[8];
#pragma unroll
			for (int u = 0; u < 8; ++u)
				t8[u] = u32x4_t{0, 0, 0, 0};
			if (!pre) {
				lpw_issue<DESC>(p, cur.S, cur.E, true, cur.gather, cur.cs, cur.ce, cur.dl, smem + (kiss & 1) * kLpwSlot,
						lds0 + (kiss & 1) * kLpwSlot, first_of(j + 2), first_of(j + 2) < p.n,
						ldsd + (uint32_t)((j + 2) & 1) * 1024, zero);
				++kiss;
			}
			for (uint32_t t = 0; t < cur.nwin; ++t) {
				// the next round: this step's next window, or the next step's first
				// (carrying the descriptors of step j + 3)
				const bool more = t + 1 < cur.nwin;
				const bool nx = !more && first_of(j + 1) < p.n && nxt.nwin > 0;
				const uint64_t iwb = more ? cur.S + (uint64_t)(t + 1) * kLpwWin : nxt.S;
				const uint64_t iE = more ? cur.E : nxt.E;
				lpw_issue<DESC>(p, iwb, iE, more || nx, more ? cur.gather : nxt.gather, more ? cur.cs : nxt.cs,
						more ? cur.ce : nxt.ce, more ? cur.dl : nxt.dl, smem + (kiss & 1) * kLpwSlot,
						lds0 + (kiss & 1) * kLpwSlot, first_of(j + 3), !more && first_of(j + 3) < p.n,
						ldsd + (uint32_t)((j + 3) & 1) * 1024, zero);
				++kiss;
				pre = nx;
				if (pend) {
					const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + pf0, C * 256);
#pragma unroll
					for (int i = 0; i < C / 4; ++i)
						bstore16<kSc1>(rs, 16 * (64 * i + l), reinterpret_cast<const u32x4_t *>(so)[64 * i + l]);
					pend = false;
					sage = 2;
				}
				// The wait for the previous round.  A store issued after this
				// round (sage 2) or after the previous one (sage 1) may stay in
				// flight: it sits between the two rounds in the in-order count.
				if (sage > 0) {
					--sage;
					asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1 + C / 4) : "memory");
				} else {
					asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1) : "memory");
				}
				// (the covering vmcnt alone orders this wave's reads behind its
				// DMA; the barrier is kept in the one-wave form as measured)
				if (!W)
					__builtin_amdgcn_s_barrier();
				if (t == 0) // step j + 2's descriptors came with window 0 of this step
					nn = lpw_step<DESC>(p, first_of(j + 2), lpw_desc_lds<DESC>(dring + ((j + 2) & 1) * 1024));
				if (p.contig == 4) // lab $CGCK_LPW_NOCONS: rounds without the per-window work
					continue;
				const uint4 *win = reinterpret_cast<const uint4 *>(smem + (kiss & 1) * kLpwSlot); // round kiss - 2
				const uint64_t wb = cur.S + (uint64_t)t * kLpwWin;
				const uint64_t we = wb + kLpwWin;
				// 1. reads of single chunks: the packet's edge chunks and its
				// header chunks cs .. cs + 7 that fall in this window (kept in
				// registers across windows; the header is read once per step)
				const bool head = cur.ok && cur.nch > 0 && cur.cs >= wb && cur.cs < we;
				const bool tail = cur.ok && cur.nch > 0 && cur.ce - 1 >= wb && cur.ce - 1 < we;
				const bool dw = !__any(cur.ok && ((cur.q | cur.len) & 3) != 0);
				if (__any(head && cur.q != 0))
					corr += head && cur.q != 0 ? lead_sum(win[lpw_at((int)(cur.cs - wb))], cur.q, dw) : 0u;
				if (__any(tail && cur.e != 16))
					corr += tail && cur.e != 16 ? trail_sum(win[lpw_at((int)(cur.ce - 1 - wb))], cur.e, dw) : 0u;
				const bool hwin = cur.ok && cur.cs + 8 > wb && cur.cs < we;
				if (!(p.flags & CGCK_RAW) && __any(hwin)) {
					const u32x4_t *win4 = reinterpret_cast<const u32x4_t *>(win);
#pragma unroll
					for (int u = 0; u < 8; ++u) {
						const uint64_t c = cur.cs + u;
						const bool in = hwin && c >= wb && c < we;
						const u32x4_t c8 = win4[in ? lpw_at((int)(c - wb)) : 0];
						t8[u] = in ? c8 : t8[u];
					}
				}
				// 2. lane per chunk: every owned chunk's sum (conflict-free 16-byte
				// reads), prefix-summed over the window in lane order; the rows'
				// scans are independent, their carries added after.  The prefix is
				// written over the slot's first rows, already read.
#if CGCK_LPW_SLOTMAJOR
				static_assert(kLpwDma == 8, "slot-major windows are 64 lanes x 8 chunks");
				// lane l owns chunks [8 l, 8 l + 8): local prefix, one wave scan
				uint32_t xs[8];
				uint32_t run = 0;
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const uint4 v = win[64 * i + l];
					run += wb + 8 * l + i < cur.E ? sum4(v, 0u) : 0u;
					xs[i] = run;
				}
				const uint32_t before = wave_scan_dpp(run) - run;
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				{
					typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
					u32x4v *p4 = reinterpret_cast<u32x4v *>(pfx + 8 * l);
					p4[0] = u32x4v{before + xs[0], before + xs[1], before + xs[2], before + xs[3]};
					p4[1] = u32x4v{before + xs[4], before + xs[5], before + xs[6], before + xs[7]};
				}
#elif CGCK_LPW_PAIR
				// A lane per PAIR of chunks (2 l, 2 l + 1 of each 2 KiB row
				// pair): half the wave scans of a lane per chunk (4 a window
				// instead of 8: the scans' DPP chain was the window's largest
				// issue cost, lpw being issue-bound on the packed layout —
				// SQ_ACTIVE_INST_ANY 0.49 of its wave cycles against dstr's
				// 0.20, profiles/r06/lpwpmc/).  The two 16-byte reads of a
				// lane go first / second by bit 3 of the lane, so lanes l and
				// l + 8 (32 bytes apart x 8) never hit the same banks.
				uint32_t ya[kLpwDma / 2], yb[kLpwDma / 2];
				const int sw = (l >> 3) & 1;
#pragma unroll
				for (int r = 0; r < kLpwDma / 2; ++r) {
					const int c = 128 * r + 2 * l;
					const uint4 va = win[c + sw], vb = win[c + 1 - sw];
					const uint32_t sa = wb + (uint64_t)(c + sw) < cur.E ? sum4(va, 0u) : 0u;
					const uint32_t sb = wb + (uint64_t)(c + 1 - sw) < cur.E ? sum4(vb, 0u) : 0u;
					const uint32_t s1 = sw ? sa : sb; // chunk c + 1's sum
					const uint32_t inc = wave_scan_dpp(sa + sb);
					yb[r] = inc;
					ya[r] = inc - s1;
				}
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				uint32_t carry = 0;
#pragma unroll
				for (int r = 0; r < kLpwDma / 2; ++r) {
					typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
					*reinterpret_cast<u32x2v *>(pfx + 128 * r + 2 * l) = u32x2v{ya[r] + carry, yb[r] + carry};
					carry += __builtin_amdgcn_readlane(yb[r], 63);
				}
#else
				uint32_t xs[kLpwDma];
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					const uint4 v = win[64 * r + l];
					xs[r] = wave_scan_dpp(wb + 64 * r + l < cur.E ? sum4(v, 0u) : 0u);
				}
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				uint32_t carry = 0;
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					pfx[64 * r + l] = xs[r] + carry;
					carry += __builtin_amdgcn_readlane(xs[r], 63);
				}
#endif
				// 3. lane per packet: its chunks in this window as a prefix difference
				const uint64_t lo = cur.cs > wb ? cur.cs : wb;
				const uint64_t hi = cur.ce < we ? cur.ce : we;
				if (cur.ok && hi > lo)
					acc += pfx[(int)(hi - 1 - wb)] - (lo > wb ? pfx[(int)(lo - 1 - wb)] : 0u);
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slots are refilled next round
			}
			if (!(p.flags & CGCK_RAW)) {
				uint4 w8[8];
#pragma unroll
				for (int u = 0; u < 8; ++u)
					w8[u] = make_uint4(t8[u].x, t8[u].y, t8[u].z, t8[u].w);
				h = header<8, false>(w8, reinterpret_cast<const uint4 *>(cur.a0 & ~(uint64_t)15), cur.nch, cur.q,
						     cur.len, p.flags, cur.ok);
			}
			if (!pre) { // the last round was a zero round: drained before the next issue or a fallback
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				sage = 0; // (a looser count would no longer cover a round)
			}
		} else if (first < p.n) {
			// not chained: the lane's packet straight from global memory
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			sage = 0;
			pre = false;
			nn = lpw_step<DESC>(p, first_of(j + 2), load_desc<DESC>(p, first_of(j + 2) + l, p.n));
			const uint4 *c0 = reinterpret_cast<const uint4 *>(cur.a0 & ~(uint64_t)15);
			const int cnt = cur.ok ? cur.nch : 0;
			for (int i = 0; __any(i < cnt); ++i) {
				const uint4 v = ldc<false>(c0, i, cnt, p.zero);
				acc = i < cnt ? sum4(v, acc) : acc;
				if (i == 0 && cnt > 0 && cur.q != 0)
					corr += lead_sum(v, cur.q, false);
				if (i == cnt - 1 && cur.e != 16)
					corr += trail_sum(v, cur.e, false);
			}
			if (!(p.flags & CGCK_RAW)) {
				uint4 w8[8];
#pragma unroll
				for (int u = 0; u < 8; ++u)
					w8[u] = ldc<false>(c0, u, cnt, p.zero);
				h = header<8, false>(w8, c0, cur.nch, cur.q, cur.len, p.flags, cur.ok);
			}
		}
		if (W && j % C == 0 && j > 0)
			wg_barrier(); // R: the writer has read the last chunk's staging
		if (pend) { // no round came (a fallback or an empty step): flush before the staging is reused
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			for (int i = l; i < C * 64; i += 64)
				gbl(p.out)[pf0 + i] = so[i];
			pend = false;
		}
		if (first < p.n) {
			const uint32_t r = fold16(acc) + (0xffffu - fold16(corr));
			const Res res = result(p, cur.a0, cur.len, fold16(r), h);
			const int slot = (int)(j % C) * 64 + l;
			so[slot] = res.out;
			if (p.verdict) // (the verdict staging is allocated only with verdicts)
				sv[slot] = (uint8_t)res.verdict;
		}
		if (W && (j + 1) % C == 0) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the chunk's outputs are in LDS
			wg_barrier();                                      // H: hand them to the writer
		} else if (!W && ((j + 1) % C == 0 || j + 1 == nsteps) && p.contig != 5) { // lab mode 5: no flush
			// flush the chunk's outputs (packets [f0, f0 + 64 C) of the batch)
			const uint64_t f0 = gstep(j - j % C) * 64;
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			const uint64_t cntp = f0 < p.n ? (p.n - f0 < (uint64_t)C * 64 ? p.n - f0 : (uint64_t)C * 64) : 0;
			if (defer_ok && cntp == (uint64_t)C * 64 && j + 1 < nsteps) {
				pend = true; // stored after the next round's issue
				pf0 = f0;
			} else {
				for (uint64_t i = l; i < cntp; i += 64) {
					if (p.out)
						gbl(p.out)[f0 + i] = so[i];
					if (p.verdict)
						gbl(p.verdict)[f0 + i] = sv[i];
				}
			}
		}
		cur = nxt;
		nxt = nn;
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// --------------------------------------------------------------------------
// Launchers
// --------------------------------------------------------------------------

// blocks for n packets at `per` a block: at most cap, at least one (an empty batch still launches)
static unsigned grid_blocks(uint64_t n, uint64_t per, uint64_t cap)
{
	const uint64_t want = (n + per - 1) / per, g = want < cap ? want : cap;
	return (unsigned)(g ? g : 1);
}

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

// An IPv6 batch the lane family's variants (lpd6, lpa6) take: at least the
// fixed header, and IP / L4 only: no field zeroing, verify or store, so no
// bad counters either (RAW | IP6 reaches the kernels as RAW).
bool lane6_ok(const KParams &p)
{
	return (p.flags & CGCK_IP6) && !(p.flags & ~(uint32_t)(CGCK_IP6 | CGCK_IP | CGCK_L4)) && p.ip_len >= 40;
}

bool lpd_ok(const KParams &p)
{
	// an output array, 16-byte aligned: a chunk's outputs leave as 16-byte stores
	return !p.desc && !p.verdict && !p.bad && !(p.flags & CGCK_STORE) && p.out &&
	       (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 && p.ip_len >= 20 && p.ip_len <= 64 &&
	       p.stride <= 64 && p.stride * 63 + p.ip_len <= 4096 &&
	       ((reinterpret_cast<uintptr_t>(p.base) | p.stride | p.l3_off) & 15) == 0;
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

bool lpw_ok(const KParams &p)
{
	return !p.bad && !(p.flags & (CGCK_STORE | kFlagNoLenCheck | kFlagL4Auto)) &&
	       (reinterpret_cast<uintptr_t>(p.desc) & 15) == 0;
}

hipError_t launch_lpw(const KParams &p, int num_cus, hipStream_t st)
{
	static const int wpc = [] { // $CGCK_LPW_WPC: waves per CU
		const char *e = CGCK_ENV("CGCK_LPW_WPC");
		return e && atoi(e) > 0 ? atoi(e) : 8;
	}();
	KParams q = p;
	q.contig = 0;
	constexpr int C = 4; // 8 KiB windows: 19.3 KiB of LDS per workgroup, 8 per CU
	const dim3 g(grid_blocks(p.n, 64 * C, (uint64_t)num_cus * wpc));
	const size_t lds = 2 * kLpwSlot + 2 * 1024 + C * 64 * (p.verdict ? 5 : 4);
#if CGCK_LAB
	if (const auto lab = launch_lpw_lab(p, q, g, lds, num_cus, wpc, st)) // $CGCK_LPW_*: q.contig, C = 8, lpx, writer
		return *lab;
#endif
	if (p.desc) {
		CGCK_NOTE_KERNEL("lpw_kernel<true, %d, false>", C);
		hipLaunchKernelGGL((lpw_kernel<true, C, false>), g, dim3(64), lds, st, q);
	} else {
		CGCK_NOTE_KERNEL("lpw_kernel<false, %d, false>", C);
		hipLaunchKernelGGL((lpw_kernel<false, C, false>), g, dim3(64), lds, st, q);
	}
	return hipGetLastError();
}

} // namespace cgck
