// cgck_l2d.hip — classify and trim a raw Ethernet burst (cgck_l2_desc,
// include/cgck.h section 3): ether_input's demultiplex (bsd44/if_ether.c:152-183)
// and ip_input's length rules (ip_input.c:28-44, 63-79) over a device-resident
// burst.  It turns the transport's {frame offset, delivered bytes} into the
// descriptors every other call takes: the IP header found behind up to two VLAN
// tags, Ethernet padding cut off by the header's own length field.
//
// Shape and memory are cgck_frame.h's, with three chunks a frame.  Everything
// the rules consult lies in the frame's first 28 bytes: the destination address,
// the ethertype, two tags, and the first six bytes of the IP header behind them
// (14 + 8 + 6); three chunks cover [0, 32).  There is no second load round.
//
// Stores.  A wave-step's 64 output descriptors are 768 consecutive bytes, three
// dwords a lane through wave_turn_store; three stores at a 12-byte lane stride
// took 0.525 ms where these take 0.484 on the 16M-frame set (profiles/l2d/).
// Any 4-byte alignment of desc_out.
//
// LDS.  The kernel has no tables: 3 KiB for the turned rows and 48 bytes for the
// 12 counters.
#include "cgck_frame.h"

namespace cgck {

constexpr uint32_t kL2dBins = CGCK_L2_NCOUNT;

__device__ __forceinline__ bool is_tpid(uint32_t et)
{
	return et == 0x8100u || et == 0x88A8u;
}

// D: desc_out is written; C: cls and / or the counters.
template <bool D, bool C>
__global__ __launch_bounds__(kFrameThreads) void l2d_kernel(L2dParams p)
{
	__shared__ uint32_t hist[kL2dBins];
	__shared__ uint32_t xpose[D ? kFrameWaves : 1][192]; // a wave-step's descriptors on their way out
	const bool count = C && p.count != nullptr;
	if (C) {
		frame_hist_zero(hist, kL2dBins);
		__syncthreads();
	}

	const FrameDescs frames = {p.base, p.raw, p.n};
	FrameCursor<3, FrameDescs> cur(frames, p.n, p.zero);

	if (cur.more()) {
		for (cur.start(); cur.more(); cur.advance()) {
			cur.ahead();
			const FDesc dc = cur.d;
			const uint64_t k = cur.k();
			const bool ok = k < p.n;
			// frame-relative dwords R0 .. R6 = bytes [0, 28)
			uint32_t R[7];
			frame_realign(cur.c.c, (uint32_t)(cur.a0 & 15), R);

			const uint32_t L = cur.len;
			const uint32_t l3 = dc.w2 & 0xffffu;
			// rule 2: the tag walk (bytes 12-13, 16-17, 20-21)
			uint32_t et = bswap16(R[3]), off = 14, tags = 0;
			bool runt = L < 14;
			if (!runt && is_tpid(et)) {
				if (L < 18) {
					runt = true;
				} else {
					et = bswap16(R[4]);
					off = 18;
					tags = 1;
					if (is_tpid(et)) {
						if (L < 22) {
							runt = true;
						} else {
							et = bswap16(R[5]);
							off = 22;
							tags = 2;
						}
					}
				}
			}
			// rule 3: the flags
			uint32_t flags = 0;
			if (L >= 14) {
				const bool bc = R[0] == 0xffffffffu && (R[1] & 0xffffu) == 0xffffu;
				flags = bc ? (uint32_t)CGCK_L2_BCAST : (R[0] & 1u) ? (uint32_t)CGCK_L2_MCAST : 0u;
				if (tags)
					flags |= CGCK_L2_VLAN;
			}
			// rule 4: b[0..3] and b[4..7], the bytes from off on
			const uint32_t X0 = __builtin_amdgcn_alignbyte(R[4], R[3], 2), X1 = __builtin_amdgcn_alignbyte(R[5], R[4], 2),
				       X2 = __builtin_amdgcn_alignbyte(R[6], R[5], 2), X3 = R[6] >> 16;
			const uint32_t B0 = tags == 0 ? X0 : tags == 1 ? X1 : X2;
			const uint32_t B1 = tags == 0 ? X1 : tags == 1 ? X2 : X3;
			const uint32_t avail = L - off; // consulted only when !runt: L >= off
			uint32_t cls, ip_len = 0;
			if (runt || l3 + off > 65535u) {
				cls = CGCK_L2_RUNT; // rules 1, 2 and 8
			} else if (is_tpid(et)) {
				cls = CGCK_L2_OTHER; // a third tag
			} else if (et == 0x0800u) {
				const uint32_t hl = (B0 & 15u) * 4, total = bswap16(B0 >> 16);
				if (avail < 20)
					cls = CGCK_L2_TOOSMALL;
				else if (((B0 >> 4) & 15u) != 4)
					cls = CGCK_L2_BADVERS;
				else if (hl < 20 || hl > avail)
					cls = CGCK_L2_BADHLEN;
				else if (total < hl)
					cls = CGCK_L2_BADLEN;
				else if (avail < total)
					cls = CGCK_L2_TOOSHORT;
				else {
					cls = CGCK_L2_IP4;
					ip_len = total;
				}
			} else if (et == 0x86DDu) {
				const uint32_t total = 40 + bswap16(B1);
				if (avail < 40)
					cls = CGCK_L2_TOOSMALL;
				else if (((B0 >> 4) & 15u) != 6)
					cls = CGCK_L2_BADVERS;
				else if (avail < total)
					cls = CGCK_L2_TOOSHORT;
				else {
					cls = CGCK_L2_IP6;
					ip_len = total;
				}
			} else {
				cls = et == 0x0806u ? (uint32_t)CGCK_L2_ARP : (uint32_t)CGCK_L2_OTHER;
			}

			if (D) {
				// 192 consecutive dwords a step (a lane stride of 3 in the wave's
				// LDS row: no bank conflict)
				const uint32_t mine[3] = {dc.lo, dc.hi, (ip_len << 16) | (cls == CGCK_L2_RUNT ? l3 : l3 + off)};
				wave_turn_store(xpose[threadIdx.x >> 6], mine, (CGCK_GLOBAL uint32_t *)p.desc_out + 192 * cur.s,
						p.n - cur.s * 64, cur.lane);
			}
			if (ok) {
				if (C) {
					if (p.cls)
						((CGCK_GLOBAL uint8_t *)p.cls)[k] = (uint8_t)(cls | flags);
					if (count) {
						__hip_atomic_fetch_add(hist + cls, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
						if (flags & (CGCK_L2_BCAST | CGCK_L2_MCAST))
							__hip_atomic_fetch_add(hist + 10, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
						if (flags & CGCK_L2_VLAN)
							__hip_atomic_fetch_add(hist + 11, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					}
				}
			}
		}
	}
	if (C)
		frame_hist_flush(hist, kL2dBins, p.count);
}

hipError_t launch_l2d(const L2dParams &p, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool d = p.desc_out != nullptr, c = p.cls != nullptr || p.count != nullptr;
#define CGCK_L2D(Dd, Cc)                                                          \
	do {                                                                      \
		CGCK_NOTE_KERNEL("l2d_kernel<%s, %s>", tf(Dd), tf(Cc));           \
		hipLaunchKernelGGL((l2d_kernel<Dd, Cc>), g, b, 0, st, p);         \
	} while (0)
	if (d && c)
		CGCK_L2D(true, true);
	else if (d)
		CGCK_L2D(true, false);
	else
		CGCK_L2D(false, true);
#undef CGCK_L2D
	return hipGetLastError();
}

} // namespace cgck
