// cgck_rssf.hip — per-frame Toeplitz RSS hash of a receive burst
// (cgck_rss_strided / cgck_rss_desc / cgck_rss_desc_host, include/cgck.h
// section 3): the kernel finds each frame's tuple itself (IPv4 with options,
// fragments, the IPv6 extension chain) and hashes it with the byte tables of
// cgck_rss.hip, so the host neither parses headers nor uploads tuples.
//
// Shape and memory are cgck_frame.h's, with four chunks a frame: the tuple of a
// typical frame lies in its first 24 (IPv4, no options) or 44 bytes (IPv6, no
// extension header), and four chunks cover [0, 48).  Besides descriptors the
// kernel takes frames at a fixed stride (RssfFrames).  A second load round —
// the ports of an IPv4 frame with options, the headers of an IPv6 extension
// chain — runs only in the lanes that need it, behind a wave-wide __any (as
// result6()'s chain walk, cgck_lane.h).
//
// LDS.  The 36 x 256 byte tables (36 KiB) are staged once per workgroup; with
// the 128-bin queue histogram a workgroup takes 36.5 KiB, so four workgroups
// share a CU's 160 KiB.  Random byte-table lookups conflict about 3.5-way
// (cgck_rss.hip); an IPv4 frame costs 8 or 12 lookups, an IPv6 frame 32 or 36.
#include "cgck_frame.h"

namespace cgck {

constexpr uint32_t kRssfTabWords = 36 * 256;
constexpr uint32_t kRssfBins = 128; // RSS_QUEUE_ID_MAX
constexpr size_t kRssfLds = (kRssfTabWords + kRssfBins) * 4;

// The frame source: descriptors, or frame k at base + k * stride + l3_off with
// ip_len bytes and nothing to fetch ahead.
template <bool DESC>
struct RssfFrames {
	const RssfParams &p;

	__device__ __forceinline__ FDesc load(uint64_t k) const
	{
		return DESC ? frame_desc(p.desc, p.n, k) : FDesc{0, 0, 0};
	}
	__device__ __forceinline__ void at(const FDesc &d, uint64_t k, uint64_t &a0, uint32_t &len) const
	{
		if (DESC) {
			frame_at(p.base, d, k < p.n, a0, len);
		} else {
			a0 = reinterpret_cast<uint64_t>(p.base) + k * p.stride + p.l3_off;
			len = k < p.n ? p.ip_len : 0;
		}
	}
};

// The four table lookups of hashed dword c (data bytes 4c .. 4c + 3).
__device__ __forceinline__ uint32_t rssf_look(const uint32_t *T, int c, uint32_t w)
{
	return T[(4 * c + 0) * 256 + (w & 255u)] ^ T[(4 * c + 1) * 256 + ((w >> 8) & 255u)] ^
	       T[(4 * c + 2) * 256 + ((w >> 16) & 255u)] ^ T[(4 * c + 3) * 256 + (w >> 24)];
}

// DESC: descriptors or a fixed stride; Q: queue ids and / or the histogram.
template <bool DESC, bool Q>
__global__ __launch_bounds__(kFrameThreads) void rssf_kernel(RssfParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	uint32_t *T = smem;
	uint32_t *hist = smem + kRssfTabWords;
	{
		const CGCK_GLOBAL u32x4_t *gt = (const CGCK_GLOBAL u32x4_t *)p.tab;
		u32x4_t *lt = reinterpret_cast<u32x4_t *>(T);
		for (uint32_t i = threadIdx.x; i < kRssfTabWords / 4; i += kFrameThreads)
			lt[i] = gt[i];
		if (Q)
			frame_hist_zero(hist, kRssfBins);
	}
	__syncthreads();

	const bool count = Q && p.qcount != nullptr;
	const RssfFrames<DESC> frames = {p};
	FrameCursor<4, RssfFrames<DESC>> cur(frames, p.n, p.zero);

	if (cur.more()) {
		for (cur.start(); cur.more(); cur.advance()) {
			cur.ahead();
			const uint64_t a0 = cur.a0, k = cur.k();
			const uint32_t len = cur.len;
			const bool ok = k < p.n;
			// frame-relative dwords R0 .. R10 = bytes [0, 44)
			uint32_t R[11];
			frame_realign(cur.c.c, (uint32_t)(a0 & 15), R);

			// which tuple: nd hashed dwords (0: no hash), the ports dword, and
			// for the second round `off`, the byte the lane reads next
			const uint32_t b0 = R[0] & 255u, v = b0 >> 4;
			uint32_t kind = 0, nd = 0, ports = 0, off = 0, nh = 0, seen = 0;
			bool pend4 = false, walk = false;
			if (len == 0) {
				kind = CGCK_BAD_LEN;
			} else if (v == 4) {
				const uint32_t hl = (b0 & 15u) * 4;
				if (len < 20 || hl < 20 || len < hl) {
					kind = CGCK_BAD_LEN;
				} else {
					// bytes 6, 7: ((b6 << 8 | b7) & 0x3FFF) != 0
					const bool frag = (R[1] & 0xff3f0000u) != 0;
					const uint32_t proto = (R[2] >> 8) & 255u;
					const bool l4 = !frag && len >= hl + 4 &&
							((proto == 6 && (p.hf & CGCK_RSS_TCP)) || (proto == 17 && (p.hf & CGCK_RSS_UDP)));
					nd = l4 ? 3 : 2;
					kind = l4 ? CGCK_RSS_L4 : 0;
					ports = R[5];
					pend4 = l4 && hl != 20;
					off = hl;
				}
			} else if (v == 6) {
				if (len < 40) {
					kind = CGCK_BAD_LEN;
				} else {
					walk = true;
					off = 40;
					nh = (R[1] >> 16) & 255u;
				}
			} else {
				kind = CGCK_NOT_IP;
			}
			const bool six = v == 6;
			// The IPv6 walk (CGCK_IP6's without its checksum-field clause).  A
			// frame without an extension header ends in the first pass with no
			// load; the loop runs again only while some lane has a header or
			// its ports to read.
			for (;;) {
				bool ext = false, prt = pend4;
				if (walk) {
					switch (v6_next(off, len, nh, seen)) {
					case kV6Past:
					case kV6Cut:
						kind = CGCK_BAD_LEN;
						break;
					case kV6Frag:
						nd = 8;
						kind = CGCK_RSS_IP6;
						break;
					case kV6Upper: {
						const bool l4 = len >= off + 4 && ((nh == 6 && (p.hf & CGCK_RSS_TCP)) ||
										     (nh == 17 && (p.hf & CGCK_RSS_UDP)));
						nd = l4 ? 9 : 8;
						kind = CGCK_RSS_IP6 | (l4 ? CGCK_RSS_L4 : 0);
						ports = R[10];
						prt = l4 && off != 40;
						break;
					}
					case kV6More:
						ext = true;
						break;
					}
					walk = ext;
				}
				if (!__any(ext || prt))
					break;
				if (ext || prt) {
					const uint32_t w = frame_dword_at(a0, len, off);
					if (ext) {
						const V6At nx = v6_eat(w, off, nh, seen);
						off = nx.off;
						nh = nx.nh;
						seen = nx.seen;
					} else {
						ports = w;
						pend4 = false;
					}
				}
			}

			// hashed dwords: IPv4 R3 R4 ports, IPv6 R2 .. R9 ports
			const uint32_t H0 = six ? R[2] : R[3], H1 = six ? R[3] : R[4], H2 = six ? R[4] : ports;
			uint32_t h = rssf_look(T, 0, H0) ^ rssf_look(T, 1, H1);
			const uint32_t h2 = rssf_look(T, 2, H2);
			h ^= nd > 2 ? h2 : 0u;
			if (__any(nd > 3)) {
				if (nd > 3) {
#pragma unroll
					for (int c = 3; c < 8; ++c)
						h ^= rssf_look(T, c, R[c + 2]);
					if (nd == 9)
						h ^= rssf_look(T, 8, ports);
				}
			}
			h = nd ? h & p.mask : 0u;

			if (ok) {
				if (p.hash)
					((CGCK_GLOBAL uint32_t *)p.hash)[k] = h;
				if (p.kind)
					((CGCK_GLOBAL uint8_t *)p.kind)[k] = (uint8_t)kind;
				if (Q) {
					const uint32_t qv = nd ? h % p.queue_num : 0xffu;
					if (p.queue)
						((CGCK_GLOBAL uint8_t *)p.queue)[k] = (uint8_t)qv;
					if (count && nd)
						__hip_atomic_fetch_add(hist + qv, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
		}
	}
	if (Q) // a queue id is below queue_num: no bin past it was touched
		frame_hist_flush(hist, min(kRssfBins, p.queue_num), p.qcount);
}

// Frames one pass of the widest grid covers, whichever of the three kernels runs.
uint64_t frame_pass_frames(int num_cus)
{
	return (uint64_t)num_cus * kFrameWgPerCu * kFrameThreads;
}

hipError_t launch_rssf(const RssfParams &p, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool desc = p.desc != nullptr, q = p.queue_num != 0;
#define CGCK_RSSF(D, Qq)                                                                 \
	do {                                                                             \
		CGCK_NOTE_KERNEL("rssf_kernel<%s, %s>", tf(D), tf(Qq));                  \
		hipLaunchKernelGGL((rssf_kernel<D, Qq>), g, b, kRssfLds, st, p);         \
	} while (0)
	if (desc && q)
		CGCK_RSSF(true, true);
	else if (desc)
		CGCK_RSSF(true, false);
	else if (q)
		CGCK_RSSF(false, true);
	else
		CGCK_RSSF(false, false);
#undef CGCK_RSSF
	return hipGetLastError();
}

} // namespace cgck
