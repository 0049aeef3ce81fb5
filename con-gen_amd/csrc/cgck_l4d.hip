// cgck_l4d.hip — per-frame TCP / UDP segment records of a verified burst
// (cgck_l4_desc, include/cgck.h section 3): the front half of tcp_input / udp_input
// (bsd44/tcp_input.c:67-110, 925-996; bsd44/udp_usrreq.c:65-79; gbtcp/inet.c:123-156)
// over a device-resident burst: the segment length rules, the header fields in
// host order, the option walk and the PCB hash, so that a worker goes from a
// descriptor to its hash bucket without reading the frame.
//
// Shape and memory are cgck_frame.h's, with six chunks a frame: they give the
// frame-relative bytes [0, 80) at any start alignment, an IPv4 header without
// options and a whole 60-byte TCP header, or an IPv6 header and a TCP header
// with timestamps (72).  In a 2048-byte ring slot the six chunks lie in the
// frame's first 128-byte line, so they cost no more memory traffic than rssf's
// four.
//
// Window.  The transport header starts at a lane-variant offset and the option
// walk indexes bytes at a lane-variant position; a register array indexed that
// way would go to scratch.  Each lane therefore puts its 80 bytes into its own
// LDS row (21 dwords: an odd stride, so the lanes of a wave start on distinct
// banks) and reads the transport header from there, dwords for the fixed fields
// (l4_off is a multiple of 4 under both families), bytes for the options.  Only
// the lane itself reads its row: no barrier.
//
// Second round.  A transport header that does not end inside [0, 80) — IPv4 with
// IP options, an IPv6 extension chain, IPv6 with a TCP option area past 40 bytes —
// is loaded again from l4_off on (five chunks: 64 bytes at any alignment) into
// the lane's row, only in the lanes that need it, behind a wave-wide __any; the
// headers of an IPv6 extension chain likewise, as rssf walks them.
//
// Stores.  A wave-step's 64 records are 2 KiB consecutive, two 16-byte halves a
// lane through wave_turn_store (l2d's finding, DESIGN.md §5.11: stores at a lane
// stride cost 8 % there).
//
// LDS.  21 KiB of rows, 8 KiB of turned records and 48 bytes of counters per
// workgroup.
#include "cgck_frame.h"

namespace cgck {

constexpr uint32_t kL4dBins = CGCK_SEG_NCOUNT;
constexpr int kL4dChunks = 6;                        // first round: bytes [0, 80)
constexpr uint32_t kL4dWin = 16u * kL4dChunks - 16u; // 80
constexpr int kL4dChunks2 = 5;                       // second round: bytes [l4_off, l4_off + 64)
constexpr int kL4dRow = 21;                          // dwords per lane: 80 bytes, odd stride

// The 64 bytes from frame byte `off` on (off < len) into the lane's row: the five
// granules from the one that holds it, clamped to the frame's last.
__device__ __forceinline__ void l4d_second(uint64_t a0, uint32_t len, uint32_t off, uint32_t *row)
{
	const int nch = frame_granules(a0, len);
	const uint32_t at = (uint32_t)(a0 & 15) + off;
	const int j = (int)(at >> 4);
	const uint64_t A = a0 & ~(uint64_t)15;
	u32x4_t c[kL4dChunks2];
#pragma unroll
	for (int i = 0; i < kL4dChunks2; ++i)
		c[i] = *gbl_at<const u32x4_t>(A + 16u * (uint32_t)min(j + i, nch - 1));
	uint32_t R[4 * kL4dChunks2 - 4];
	frame_realign(c, at & 15u, R);
#pragma unroll
	for (int i = 0; i < 4 * kL4dChunks2 - 4; ++i)
		row[i] = R[i];
}

// SG: seg is written (the fields and the option walk); X: cls, hash and / or the
// counters.
template <bool SG, bool X>
__global__ __launch_bounds__(kFrameThreads) void l4d_kernel(L4dParams p)
{
	__shared__ uint32_t hist[kL4dBins];
	__shared__ uint32_t rows[kFrameThreads * kL4dRow];
	__shared__ __attribute__((aligned(16))) u32x4_t xpose[SG ? kFrameWaves : 1][128]; // a wave-step's records on their way out
	const bool count = X && p.count != nullptr;
	if (X) {
		frame_hist_zero(hist, kL4dBins);
		__syncthreads();
	}

	uint32_t *row = rows + kL4dRow * threadIdx.x;
	const uint8_t *rowb = reinterpret_cast<const uint8_t *>(row);
	const FrameDescs frames = {p.base, p.desc, p.n};
	FrameCursor<kL4dChunks, FrameDescs> cur(frames, p.n, p.zero);

	if (cur.more()) {
		for (cur.start(); cur.more(); cur.advance()) {
			cur.ahead();
			const uint64_t a0 = cur.a0, k = cur.k();
			const uint32_t len = cur.len;
			const bool ok = k < p.n;
			// frame-relative dwords R0 .. R19 = bytes [0, 80)
			uint32_t R[4 * kL4dChunks - 4];
			frame_realign(cur.c.c, (uint32_t)(a0 & 15), R);

			// step 1, the IP layer (rssf's rules): st 0 NONE, 1 FRAG, 2 proto known
			const uint32_t b0 = R[0] & 255u, v = b0 >> 4;
			const bool six = len != 0 && v == 6;
			uint32_t st = 0, off = 0, proto = 0, F = 0, nh = 0, seen = 0;
			bool walk = false;
			if (len == 0) {
			} else if (v == 4) {
				const uint32_t hl = (b0 & 15u) * 4;
				if (!(len < 20 || hl < 20 || len < hl)) {
					// bytes 6, 7: ((b6 << 8 | b7) & 0x3FFF) != 0
					const bool frag = (R[1] & 0xff3f0000u) != 0;
					st = frag ? 1 : 2;
					off = hl;
					proto = (R[2] >> 8) & 255u;
					F = R[3];
				}
			} else if (v == 6) {
				if (len >= 40) {
					walk = true;
					off = 40;
					nh = (R[1] >> 16) & 255u;
					F = R[2] ^ R[3] ^ R[4] ^ R[5];
				}
			}
			// The IPv6 walk.  A frame without an extension header ends in the first
			// pass with no load; the loop runs again only while some lane has a
			// header to read.
			for (;;) {
				bool ext = false;
				if (walk) {
					switch (v6_next(off, len, nh, seen)) {
					case kV6Past:
					case kV6Cut:
						break; // st stays 0
					case kV6Frag:
						st = 1;
						break;
					case kV6Upper:
						st = 2;
						proto = nh;
						break;
					case kV6More:
						ext = true;
						break;
					}
					walk = ext;
				}
				if (!__any(ext))
					break;
				if (ext) {
					const V6At nx = v6_eat(frame_dword_at(a0, len, off), off, nh, seen);
					off = nx.off;
					nh = nx.nh;
					seen = nx.seen;
				}
			}

			// step 2: what is left behind l4_off, and whether the transport header
			// has to be read: TCP needs t[12] before it knows how much
			const uint32_t m = len - off; // st != 0: off <= len
			const bool tcp = st == 2 && proto == 6 && m >= 20, udp = st == 2 && proto == 17 && m >= 8;
#pragma unroll
			for (int i = 0; i < 4 * kL4dChunks - 4; ++i)
				row[i] = R[i];
			uint32_t rb = off; // the row byte of t[0]
			bool second = false;
			if (tcp) {
				if (off + 20 <= kL4dWin) {
					const uint32_t th = ((row[(off >> 2) + 3] >> 4) & 15u) * 4;
					const uint32_t want = SG && th >= 20 && th <= m ? th : 20u;
					second = off + want > kL4dWin;
				} else {
					second = true;
				}
			} else if (udp) {
				second = off + 8 > kL4dWin;
			}
			if (__any(second)) {
				if (second) {
					l4d_second(a0, len, off, row);
					rb = 0;
				}
			}

			// steps 3 to 5
			uint32_t cls, pay = m, ports = 0, seq = 0, ack = 0, win = 0, thf = 0, hdr = 0;
			uint32_t opt = 0, mss = 0, wsc = 0, tsv = 0, tse = 0;
			if (st == 0) {
				cls = CGCK_SEG_NONE;
				off = 0;
				pay = 0;
			} else if (st == 1) {
				cls = CGCK_SEG_FRAG;
			} else if (proto == 6) {
				if (m < 20) {
					cls = CGCK_SEG_TCP_SHORT;
				} else {
					const uint32_t *t = row + (rb >> 2);
					const uint32_t w3 = t[3];
					const uint32_t th = ((w3 >> 4) & 15u) * 4;
					if (th < 20) {
						cls = CGCK_SEG_TCP_BADOFF;
					} else if (th > m) {
						cls = CGCK_SEG_TCP_OFFLONG;
					} else {
						cls = CGCK_SEG_TCP;
						ports = t[0];
						pay = m - th;
						thf = (w3 >> 8) & 255u;
						if (SG) {
							seq = __builtin_bswap32(t[1]);
							ack = __builtin_bswap32(t[2]);
							win = bswap16(w3 >> 16);
							hdr = th;
							// tcp_dooptions (tcp_input.c:925-996) over o[0, cnt): no
							// byte at or past th is consulted
							const uint8_t *o = rowb + rb + 20;
							const uint32_t cnt = th - 20;
							const bool syn = (thf & 0x02u) != 0;
							uint32_t i = 0;
							while (i < cnt) {
								const uint32_t kind = o[i];
								if (kind == 0)
									break;
								if (kind == 1) {
									++i;
									continue;
								}
								if (i + 1 >= cnt) {
									opt |= CGCK_SEG_OPT_BAD;
									break;
								}
								const uint32_t ol = o[i + 1];
								if (ol == 0 || i + ol > cnt) {
									opt |= CGCK_SEG_OPT_BAD;
									break;
								}
								if (kind == 2 && ol == 4 && syn) {
									mss = (uint32_t)o[i + 2] << 8 | o[i + 3];
									opt |= CGCK_SEG_MSS;
								} else if (kind == 3 && ol == 3 && syn) {
									wsc = min((uint32_t)o[i + 2], 14u);
									opt |= CGCK_SEG_WS;
								} else if (kind == 8 && ol == 10) {
									tsv = (uint32_t)o[i + 2] << 24 | (uint32_t)o[i + 3] << 16 |
									      (uint32_t)o[i + 4] << 8 | o[i + 5];
									tse = (uint32_t)o[i + 6] << 24 | (uint32_t)o[i + 7] << 16 |
									      (uint32_t)o[i + 8] << 8 | o[i + 9];
									opt |= CGCK_SEG_TS;
								}
								i += ol;
							}
						}
					}
				}
			} else if (proto == 17) {
				if (m < 8) {
					cls = CGCK_SEG_UDP_SHORT;
				} else {
					const uint32_t *t = row + (rb >> 2);
					const uint32_t ulen = bswap16(t[1]);
					if (ulen > m || ulen < 8) {
						cls = CGCK_SEG_UDP_BADLEN;
					} else {
						cls = CGCK_SEG_UDP;
						ports = t[0];
						hdr = 8;
						pay = ulen - 8;
					}
				}
			} else {
				cls = proto == (six ? 58u : 1u) ? (uint32_t)CGCK_SEG_ICMP : (uint32_t)CGCK_SEG_OTHER;
			}
			const bool l4 = cls == CGCK_SEG_TCP || cls == CGCK_SEG_UDP;

			if (SG) {
				// 128 consecutive 16-byte pieces a step
				const u32x4_t mine[2] = {
					{seq, ack, tsv, tse},
					{ports, win | (mss << 16), off | (pay << 16),
					 cls == CGCK_SEG_TCP ? thf | (hdr << 8) | (wsc << 16) | (opt << 24) : hdr << 8}};
				wave_turn_store(xpose[threadIdx.x >> 6], mine, (CGCK_GLOBAL u32x4_t *)p.seg + 128 * cur.s,
						p.n - cur.s * 64, cur.lane);
			}
			if (X && ok) {
				if (p.cls)
					((CGCK_GLOBAL uint8_t *)p.cls)[k] = (uint8_t)(cls | (six ? (uint32_t)CGCK_SEG_IP6 : 0u));
				if (p.hash) {
					// SO_HASH(faddr, lport, fport), subr.h:179-180, as the receiver's
					// in_pcblookup computes it
					const uint32_t h = F ^ (F >> 16) ^ __builtin_bswap16((uint16_t)((ports >> 16) ^ ports));
					((CGCK_GLOBAL uint32_t *)p.hash)[k] = l4 ? h : 0u;
				}
				if (count) {
					__hip_atomic_fetch_add(hist + cls, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					if (six)
						__hip_atomic_fetch_add(hist + 11, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
		}
	}
	if (X)
		frame_hist_flush(hist, kL4dBins, p.count);
}

hipError_t launch_l4d(const L4dParams &p, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool sg = p.seg != nullptr, x = p.cls != nullptr || p.hash != nullptr || p.count != nullptr;
#define CGCK_L4D(Ss, Xx)                                                          \
	do {                                                                      \
		CGCK_NOTE_KERNEL("l4d_kernel<%s, %s>", tf(Ss), tf(Xx));           \
		hipLaunchKernelGGL((l4d_kernel<Ss, Xx>), g, b, 0, st, p);         \
	} while (0)
	if (sg && x)
		CGCK_L4D(true, true);
	else if (sg)
		CGCK_L4D(true, false);
	else
		CGCK_L4D(false, true);
#undef CGCK_L4D
	return hipGetLastError();
}

} // namespace cgck
