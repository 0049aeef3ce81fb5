// cgck_l4b.hip — frames from segment records (cgck_l4_build, include/cgck.h section
// 3): the inverse of cgck_l2_desc + cgck_l4_desc.  Ethernet + IPv4 / IPv6 + TCP / UDP
// headers of a burst (tcp_output.c:253-304,359-418; tcp_subr.c:52-123;
// ip_output.c:42-68; gbtcp/tcp.c:381-450) are written into ring slots from flow
// records and cgck_seg_t records, both checksums final for a segment without
// payload.
//
// Shape is cgck_frame.h's: a lane per frame, 64 frames a wave-step, waves
// grid-stride over the steps, frame_grid's four 256-thread workgroups a CU.  The
// kernel reads no frame bytes, so it has its own loop instead of FrameCursor
// (whose prefetch is of frame chunks): a step loads the slot descriptor, the seg
// record (two 16-byte loads), the class byte and the flow index, then the flow
// record (three 16-byte loads), and the 16 waves a CU hide the two dependent
// rounds.
//
// The header in registers.  A header is 42 to 98 bytes whose parts start at
// lane-variant offsets (h 14 / 18, iph 20 / 40, the options present), and l4d's
// precedent for lane-variant positions is an LDS row.  Here no
// position needs a variable index: the header is laid out in a 25-dword register
// row R with the IP header always at row byte 20, so the Ethernet header ends
// there and starts at row byte s = 20 - h (6, or 2 with a tag), the transport
// header starts at row dword 10 or 15, and the options are packed by selects on
// the count of those in front.  Every R[i] is a v_cndmask between at most three
// statically named values: no LDS row, no scratch, and the sums are taken from the
// same registers (v_dot2_u32_u16).
//
// Stores, the inverse of frame_realign.  The row leaves for an address of any byte
// alignment: with q = (s - a0) & 3, the aligned destination dword j holds the row
// bytes [4j + q, 4j + q + 4) = v_alignbyte(R[j + 1], R[j], q); a lane stores the
// dwords that lie wholly inside [s, e), and the up to three bytes in front (always
// eth_dst's first) and behind (the header's last dword, named by the options) as
// byte and short stores.  Nothing is read, nothing outside the header is written,
// and no store is wider than the bytes it owns, so neighbours may share a dword.
//
// TURN is the other store shape, kept for the A/B of DESIGN.md section 5.14 and the
// tests: each lane also puts its shifted dwords into its own 33-dword LDS block in
// destination coordinates (the 128-byte window from the 16-byte boundary below the
// frame), stores only the dwords and bytes of granules the header does not cover
// whole, and the wave stores the whole granules eight lanes a frame as 16-byte
// pieces.  It measured no faster than the direct shape (1.02 times its time, inside
// the margins), so the product launches TURN = false.
//
// The two descriptor outputs leave through wave_turn_store as 12-byte records, the
// counters through the LDS histogram.  LDS: 3 KiB of turned records and 32 bytes
// of counters per workgroup (TURN: 33 KiB of blocks and 3 KiB of window words more).
#include "cgck_frame.h"

namespace cgck {

constexpr uint32_t kL4bBins = CGCK_BLD_NCOUNT;
constexpr int kL4bRow = 25; // dwords: 20 bytes up to the IP header, 40 of IPv6, 40 of TCP

// The 16-bit word the two bytes of `v` big-endian read as little-endian.
__device__ __forceinline__ uint32_t be16(uint32_t v)
{
	return bswap16(v);
}

constexpr int kL4bBlk = 33; // dwords of a lane's turned block: one in front, the 128-byte window, an odd stride

// D: raw_out and / or desc_out are written; X: cls and / or the counters; T: the
// whole 16-byte granules of a header are turned through LDS and leave as 16-byte
// stores, eight lanes a frame (false: every dword leaves from its own lane).
template <bool D, bool X, bool TURN>
__global__ __launch_bounds__(kFrameThreads) void l4b_kernel(L4bParams p)
{
	__shared__ uint32_t hist[kL4bBins];
	__shared__ uint32_t xpose[D ? kFrameWaves : 1][192]; // a wave-step's descriptors on their way out
	__shared__ uint32_t turn[TURN ? kFrameWaves : 1][TURN ? 64 * kL4bBlk : 1]; // a wave-step's headers in destination coordinates
	__shared__ uint32_t tmeta[TURN ? kFrameWaves : 1][TURN ? 64 * 3 : 1];       // per frame: the window's address, lead | end << 8
	const bool count = X && p.count != nullptr;
	if (X) {
		frame_hist_zero(hist, kL4bBins);
		__syncthreads();
	}
	const int lane = threadIdx.x & 63;
	const uint64_t nsteps = (p.n + 63) / 64, W = (uint64_t)gridDim.x * kFrameWaves;

	for (uint64_t step = (uint64_t)blockIdx.x * kFrameWaves + (threadIdx.x >> 6); step < nsteps; step += W) {
		const uint64_t k = step * 64 + lane;
		const bool ok = k < p.n;
		const uint64_t kk = ok ? k : p.n - 1;
		const FDesc d = frame_desc(p.slot, p.n, k);
		const CGCK_GLOBAL u32x4_t *sg = (const CGCK_GLOBAL u32x4_t *)p.seg + 2 * kk;
		const u32x4_t s0 = sg[0], s1 = sg[1];
		const uint32_t c = p.cls ? ((const CGCK_GLOBAL uint8_t *)p.cls)[kk] & 15u : (uint32_t)CGCK_SEG_TCP;
		const uint64_t f = p.fidx ? (uint64_t)((const CGCK_GLOBAL uint32_t *)p.fidx)[kk] : kk;
		const bool l4 = c == CGCK_SEG_TCP || c == CGCK_SEG_UDP, udp = c == CGCK_SEG_UDP;
		const bool fin = l4 && f < p.nflow;
		u32x4_t f0 = {0, 0, 0, 0}, f1 = f0, f2 = f0;
		if (fin) {
			const CGCK_GLOBAL u32x4_t *fl = (const CGCK_GLOBAL u32x4_t *)p.flow + 3 * f;
			f0 = fl[0];
			f1 = fl[1];
			f2 = fl[2];
		}
		uint64_t a0;
		uint32_t cap;
		frame_at(p.base, d, ok, a0, cap);
		const uint32_t l3 = d.w2 & 0xffffu;

		// the record
		const uint32_t seq = s0[0], ack = s0[1], tsv = s0[2], tse = s0[3];
		const uint32_t ports = s1[0], win = s1[1] & 0xffffu, mss = s1[1] >> 16, pay = s1[2] >> 16;
		const uint32_t thf = s1[3] & 255u, wsc = (s1[3] >> 16) & 255u, opt = s1[3] >> 24;
		const uint32_t tci = f0[3] & 0xffffu, fflags = (f0[3] >> 16) & 255u, ttl = f0[3] >> 24;
		const bool six = (fflags & CGCK_FLOW_IP6) != 0, vlan = (fflags & CGCK_FLOW_VLAN) != 0;
		const bool hm = (opt & CGCK_SEG_MSS) != 0, hw = (opt & CGCK_SEG_WS) != 0, ht = (opt & CGCK_SEG_TS) != 0;

		// rules 1 to 5
		const uint32_t h = vlan ? 18u : 14u, iph = six ? 40u : 20u;
		const uint32_t l4h = udp ? 8u : 20u + (hm ? 4u : 0u) + (hw ? 4u : 0u) + (ht ? 12u : 0u);
		const uint32_t l4len = l4h + pay, total = iph + l4len, L = h + total;
		uint32_t cls;
		if (!l4)
			cls = CGCK_BLD_SKIP;
		else if (!fin || (fflags & ~(uint32_t)(CGCK_FLOW_IP6 | CGCK_FLOW_VLAN)) != 0)
			cls = CGCK_BLD_BADFLOW;
		else if (udp ? pay > 65527u : ((opt & ~(uint32_t)(CGCK_SEG_MSS | CGCK_SEG_WS | CGCK_SEG_TS)) != 0 || (hw && wsc > 14u)))
			cls = CGCK_BLD_BADSEG;
		else if (L > cap || l3 + h > 65535u)
			cls = CGCK_BLD_NOROOM;
		else
			cls = udp ? CGCK_BLD_UDP : CGCK_BLD_TCP;
		const bool built = ok && cls <= CGCK_BLD_UDP;
		const bool fam = six && cls != CGCK_BLD_BADFLOW, paid = built && pay != 0;
		const bool built6 = built && six;
		// the 128-byte window from the 16-byte boundary at or below the frame: the header is its bytes [lead, wend)
		const uint32_t lead = (uint32_t)a0 & 15u, wend = built ? lead + h + iph + l4h : 0u;

		if (built) {
			const uint32_t proto = udp ? 17u : 6u;
			// the transport header, its sum field zero
			uint32_t T[10];
			const uint32_t mssd = 0x0402u | be16(mss) << 16, wsd = 0x030301u | wsc << 24, ts0 = 0x0A080101u;
			const uint32_t ts1 = __builtin_bswap32(tsv), ts2 = __builtin_bswap32(tse);
			if (udp) {
				T[0] = ports;
				T[1] = be16(8u + pay);
#pragma unroll
				for (int i = 2; i < 10; ++i)
					T[i] = 0;
			} else {
				T[0] = ports;
				T[1] = __builtin_bswap32(seq);
				T[2] = __builtin_bswap32(ack);
				T[3] = (l4h >> 2) << 4 | thf << 8 | be16(win) << 16;
				T[4] = 0;
				// the options, packed: `pre` of MSS and WS in front of the timestamps
				const uint32_t pre = (hm ? 1u : 0u) + (hw ? 1u : 0u);
				const uint32_t P[2] = {hm ? mssd : wsd, wsd};
				const uint32_t TS[3] = {ht ? ts0 : 0u, ht ? ts1 : 0u, ht ? ts2 : 0u};
#pragma unroll
				for (int j = 0; j < 5; ++j) {
					const uint32_t a = j < 3 ? TS[j] : 0u;                            // pre 0
					const uint32_t b = j == 0 ? P[0] : (j - 1 < 3 ? TS[j - 1] : 0u);  // pre 1
					const uint32_t cc = j < 2 ? P[j] : TS[j - 2];                      // pre 2
					T[5 + j] = pre == 0 ? a : pre == 1 ? b : cc;
				}
			}
			// the IP header and the address words of the pseudo-header
			uint32_t I[10];
			uint32_t acc = 0;
			if (six) {
				I[0] = 0x60u;
				I[1] = be16(l4len) | proto << 16 | ttl << 24;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					I[2 + i] = f1[i];
					I[6 + i] = f2[i];
					acc = hsum(f1[i], hsum(f2[i], acc));
				}
			} else {
				const uint32_t id = (p.ip_id0 + (uint32_t)k) & 0xffffu;
				I[0] = 0x45u | be16(total) << 16;
				I[1] = be16(id) | be16(p.ip_off) << 16;
				I[2] = ttl | proto << 8;
				I[3] = f1[0];
				I[4] = f2[0];
				acc = hsum(I[3], hsum(I[4], 0));
				const uint32_t ipsum = finish(fold16(hsum(I[0], hsum(I[1], hsum(I[2], acc)))));
				I[2] |= ipsum << 16;
#pragma unroll
				for (int i = 5; i < 10; ++i)
					I[i] = 0;
			}
			// the transport sum: final without payload, zero with (the fill's to write)
			uint32_t l4sum = 0;
			if (pay == 0) {
				acc += (proto << 8) + be16(l4len);
#pragma unroll
				for (int i = 0; i < 10; ++i)
					acc = hsum(T[i], acc);
				l4sum = finish(fold16(acc));
			}
			if (udp)
				T[1] |= l4sum << 16;
			else
				T[4] = l4sum;
			// the header's last dword: what the bytes behind the last whole dword come from
			const uint32_t Z = udp ? T[1] : ht ? ts2 : hw ? wsd : hm ? mssd : T[4];

			// the row: Ethernet up to byte 20, IP from there, the transport header behind it
			uint32_t R[kL4bRow + 1];
			const uint32_t M0 = f0[0], M1 = f0[1], M2 = f0[2];
			const uint32_t A = M0 << 16, B = __builtin_amdgcn_alignbyte(M1, M0, 2),
				       C = __builtin_amdgcn_alignbyte(M2, M1, 2);
			const uint32_t et = six ? 0xDD86u : 0x0008u;
			R[0] = vlan ? A : 0u;
			R[1] = vlan ? B : A;
			R[2] = vlan ? C : B;
			R[3] = vlan ? (M2 >> 16 | 0x0081u << 16) : C;
			R[4] = vlan ? (be16(tci) | et << 16) : (M2 >> 16 | et << 16);
#pragma unroll
			for (int j = 0; j < 5; ++j) {
				R[5 + j] = I[j];
				R[10 + j] = six ? I[5 + j] : T[j];
				R[15 + j] = six ? T[j] : T[5 + j];
				R[20 + j] = six ? T[5 + j] : 0u;
			}
			R[kL4bRow] = 0;

			const uint32_t s = 20u - h, e = 20u + iph + l4h;
			const uint32_t q = (s - (uint32_t)a0) & 3u;
			const uint64_t Q = a0 - s + q; // where row dword 0, shifted by q bytes, would go: 4-byte aligned
			// TURN: window byte of row dword 0 shifted by q: a multiple of 4 in [-4, 16]
			const int wq = (int)lead - (int)s + (int)q;
			uint32_t *blk = turn[TURN ? threadIdx.x >> 6 : 0] + (TURN ? kL4bBlk * lane + 1 + (wq >> 2) : 0);
#pragma unroll
			for (int j = 0; j < kL4bRow; ++j) {
				const uint32_t lo = 4u * j + q;
				if (lo >= s && lo + 4 <= e) {
					const uint32_t w = __builtin_amdgcn_alignbyte(R[j + 1], R[j], q);
					bool mine = true;
					if (TURN) {
						// a dword of a granule that lies wholly inside the header leaves in the second phase
						const uint32_t g = (uint32_t)(wq + 4 * j) & ~15u;
						blk[j] = w;
						mine = g < lead || g + 16 > wend;
					}
					if (mine)
						*gbl_at<uint32_t>(Q + 4u * j) = w;
				}
			}
			// in front: eth_dst's first bytes up to the first aligned address
			const uint32_t hb = (0u - (uint32_t)a0) & 3u;
			if (hb & 1u)
				*gbl_at<uint8_t>(a0) = (uint8_t)M0;
			if (hb & 2u)
				*gbl_at<uint16_t>(a0 + (hb & 1u)) = (uint16_t)(M0 >> (8u * (hb & 1u)));
			// behind: the last tb bytes of Z from the last aligned address on
			const uint64_t E = a0 + h + iph + l4h;
			const uint32_t tb = (uint32_t)E & 3u;
			if (tb & 2u)
				*gbl_at<uint16_t>(E - tb) = (uint16_t)(Z >> (8u * (4u - tb)));
			if (tb & 1u)
				*gbl_at<uint8_t>(E - 1) = (uint8_t)(Z >> 24);
		}

		if (TURN) {
			// second phase: eight lanes a frame, a 16-byte granule each, eight frames an instruction
			uint32_t *tw = turn[threadIdx.x >> 6], *tm = tmeta[threadIdx.x >> 6];
			tm[3 * lane + 0] = (uint32_t)(a0 & ~(uint64_t)15);
			tm[3 * lane + 1] = (uint32_t)(a0 >> 32);
			tm[3 * lane + 2] = lead | wend << 8;
			__builtin_amdgcn_wave_barrier();
			asm volatile("" ::: "memory");
			const uint32_t g = 16u * (lane & 7);
#pragma unroll
			for (int t = 0; t < 8; ++t) {
				const int fr = 8 * t + (lane >> 3);
				const uint32_t m = tm[3 * fr + 2];
				if (g >= (m & 255u) && g + 16 <= m >> 8) {
					const uint32_t *b = tw + kL4bBlk * fr + 1 + (g >> 2);
					const u32x4_t v = {b[0], b[1], b[2], b[3]};
					*gbl_at<u32x4_t>((((uint64_t)tm[3 * fr + 1] << 32) | tm[3 * fr]) + g) = v;
				}
			}
			__builtin_amdgcn_wave_barrier();
			asm volatile("" ::: "memory");
		}

		if (D) {
			uint32_t *xs = xpose[threadIdx.x >> 6];
			const uint64_t left = p.n - step * 64;
			const bool b = cls <= CGCK_BLD_UDP;
			if (p.raw_out) {
				const uint32_t mine[3] = {d.lo, d.hi, l3 | (b ? L : 0u) << 16};
				wave_turn_store(xs, mine, (CGCK_GLOBAL uint32_t *)p.raw_out + 192 * step, left, lane);
			}
			if (p.desc_out) {
				const uint32_t mine[3] = {d.lo, d.hi, b ? (l3 + h) | total << 16 : l3};
				wave_turn_store(xs, mine, (CGCK_GLOBAL uint32_t *)p.desc_out + 192 * step, left, lane);
			}
		}
		if (X && ok) {
			if (p.cls_out)
				((CGCK_GLOBAL uint8_t *)p.cls_out)[k] =
					(uint8_t)(cls | (fam ? (uint32_t)CGCK_BLD_IP6 : 0u) | (paid ? (uint32_t)CGCK_BLD_PAYLOAD : 0u));
			if (count) {
				__hip_atomic_fetch_add(hist + cls, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				if (built6)
					__hip_atomic_fetch_add(hist + 6, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				if (paid)
					__hip_atomic_fetch_add(hist + 7, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
		}
	}
	if (X)
		frame_hist_flush(hist, kL4bBins, p.count);
}

hipError_t launch_l4b(const L4bParams &p, bool turned, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool d = p.raw_out != nullptr || p.desc_out != nullptr, x = p.cls_out != nullptr || p.count != nullptr;
#define CGCK_L4B(Dd, Xx)                                                                  \
	do {                                                                              \
		if (turned) {                                                             \
			CGCK_NOTE_KERNEL("l4b_kernel<%s, %s, true>", tf(Dd), tf(Xx));     \
			hipLaunchKernelGGL((l4b_kernel<Dd, Xx, true>), g, b, 0, st, p);   \
		} else {                                                                  \
			CGCK_NOTE_KERNEL("l4b_kernel<%s, %s, false>", tf(Dd), tf(Xx));    \
			hipLaunchKernelGGL((l4b_kernel<Dd, Xx, false>), g, b, 0, st, p);  \
		}                                                                         \
	} while (0)
	if (d && x)
		CGCK_L4B(true, true);
	else if (d)
		CGCK_L4B(true, false);
	else if (x)
		CGCK_L4B(false, true);
	else
		CGCK_L4B(false, false);
#undef CGCK_L4B
	return hipGetLastError();
}

} // namespace cgck
