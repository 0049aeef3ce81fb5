// cgck_rssf.hip — per-frame Toeplitz RSS hash of a receive burst
// (cgck_rss_strided / cgck_rss_desc / cgck_rss_desc_host, include/cgck.h
// section 3): the kernel finds each frame's tuple itself (IPv4 with options,
// fragments, the IPv6 extension chain) and hashes it with the byte tables of
// cgck_rss.hip, so the host neither parses headers nor uploads tuples.
//
// Shape.  One lane per frame, 64 frames per wave-step, waves grid-stride over
// the steps.  The 36 x 256 byte tables (36 KiB) are staged in LDS once per
// workgroup; with the 128-bin queue histogram a workgroup takes 36.5 KiB, so
// four 256-thread workgroups share a CU's 160 KiB.
//
// Memory.  The kernel is a gather of one granule per frame.  The tuple of a
// typical frame lies in its first 24 (IPv4, no options) or 44 bytes (IPv6, no
// extension header), so every lane loads, unconditionally, the four aligned
// 16-byte chunks from the frame's first granule on — they cover [0, 48) at any
// byte alignment — and realigns them in registers (v_bfi selects by the dword
// shift, v_alignbyte by the byte shift): no byte loads.  Chunk indices are
// clamped to the granules that hold a byte of [frame, frame + ip_len) (ldc's
// rule, cgck_device.h; a lane without a frame reads the zero chunk), so no load
// touches a granule before a frame's first or after its last.  The descriptors
// of step s + 2 and the chunks of step s + 1 are loaded before step s is
// hashed: each wave keeps two steps of loads in flight behind its hashing.
// A second load round — the ports of an IPv4 frame with options, the headers
// of an IPv6 extension chain — runs only in the lanes that need it, behind a
// wave-wide __any (as result6()'s chain walk, cgck_lane.h).
//
// Random byte-table lookups conflict about 3.5-way in LDS (cgck_rss.hip); an
// IPv4 frame costs 8 or 12 lookups, an IPv6 frame 32 or 36.
//
// qcount: frames are counted in an LDS histogram (ds_add), and each workgroup
// adds its non-zero bins to global memory once, after its loop.
#include "cgck_device.h"

namespace cgck {

constexpr int kRssfThreads = 256;
constexpr int kRssfWaves = kRssfThreads / 64;
constexpr int kRssfWgPerCu = 4;
constexpr uint32_t kRssfTabWords = 36 * 256;
constexpr uint32_t kRssfBins = 128; // RSS_QUEUE_ID_MAX
constexpr size_t kRssfLds = (kRssfTabWords + kRssfBins) * 4;
constexpr int kRssfMaxExt = kV6MaxExt;

struct RDesc {
	uint32_t lo, hi, w2;
};

struct RChunks {
	u32x4_t c[4];
};

// Descriptor of frame k (index clamped: the lanes past n of the last step
// re-read the last descriptor and drop it in frame_of).
template <bool DESC>
__device__ __forceinline__ RDesc rssf_desc(const RssfParams &p, uint64_t k)
{
	RDesc d = {0, 0, 0};
	if (DESC) {
		const uint64_t kk = k < p.n ? k : p.n - 1;
		const CGCK_GLOBAL uint32_t *g = (const CGCK_GLOBAL uint32_t *)p.desc + 3 * kk;
		d.lo = g[0];
		d.hi = g[1];
		d.w2 = g[2];
	}
	return d;
}

template <bool DESC>
__device__ __forceinline__ void frame_of(const RssfParams &p, const RDesc &d, uint64_t k, uint64_t &a0, uint32_t &len)
{
	if (DESC) {
		a0 = reinterpret_cast<uint64_t>(p.base) + (((uint64_t)d.hi << 32) | d.lo) + (d.w2 & 0xffffu);
		len = d.w2 >> 16;
	} else {
		a0 = reinterpret_cast<uint64_t>(p.base) + k * p.stride + p.l3_off;
		len = p.ip_len;
	}
	if (k >= p.n)
		len = 0;
}

// Granules that hold a byte of [a0, a0 + len).
__device__ __forceinline__ int granules(uint64_t a0, uint32_t len)
{
	return len ? (int)(((uint32_t)(a0 & 15) + len + 15) >> 4) : 0;
}

// Chunk i of the frame's nch granules (clamped), or the zero chunk.
__device__ __forceinline__ u32x4_t rssf_chunk(uint64_t a0, int nch, int i, const void *zero, int lane)
{
	const uint64_t at = nch > 0 ? (a0 & ~(uint64_t)15) + 16u * (uint32_t)min(i, nch - 1)
				    : reinterpret_cast<uint64_t>(zero) + 64u * (uint32_t)lane;
	return *gbl_at<const u32x4_t>(at);
}

__device__ __forceinline__ RChunks rssf_first(uint64_t a0, uint32_t len, const void *zero, int lane)
{
	RChunks r;
	const int nch = granules(a0, len);
#pragma unroll
	for (int i = 0; i < 4; ++i)
		r.c[i] = rssf_chunk(a0, nch, i, zero, lane);
	return r;
}

// The frame-relative dword at byte `off` (a multiple of 4, off + 2 <= len):
// the one or two granules that hold it, realigned.  Bytes of it past the
// frame's last granule come back as that granule's; the callers consult only
// bytes below len.
__device__ __forceinline__ uint32_t rssf_dword_at(uint64_t a0, uint32_t len, uint32_t off)
{
	const int nch = granules(a0, len);
	const uint32_t at = (uint32_t)(a0 & 15) + off;
	const int j = (int)(at >> 4);
	const uint64_t A = a0 & ~(uint64_t)15;
	const u32x4_t x = *gbl_at<const u32x4_t>(A + 16u * (uint32_t)min(j, nch - 1));
	const u32x4_t y = *gbl_at<const u32x4_t>(A + 16u * (uint32_t)min(j + 1, nch - 1));
	const uint32_t dq = (at >> 2) & 3u;
	const uint32_t lo = dq == 0 ? x[0] : dq == 1 ? x[1] : dq == 2 ? x[2] : x[3];
	const uint32_t hi = dq == 0 ? x[1] : dq == 1 ? x[2] : dq == 2 ? x[3] : y[0];
	return __builtin_amdgcn_alignbyte(hi, lo, at & 3u);
}

// The four table lookups of hashed dword c (data bytes 4c .. 4c + 3).
__device__ __forceinline__ uint32_t rssf_look(const uint32_t *T, int c, uint32_t w)
{
	return T[(4 * c + 0) * 256 + (w & 255u)] ^ T[(4 * c + 1) * 256 + ((w >> 8) & 255u)] ^
	       T[(4 * c + 2) * 256 + ((w >> 16) & 255u)] ^ T[(4 * c + 3) * 256 + (w >> 24)];
}

// DESC: descriptors or a fixed stride; Q: queue ids and / or the histogram.
template <bool DESC, bool Q>
__global__ __launch_bounds__(kRssfThreads) void rssf_kernel(RssfParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	uint32_t *T = smem;
	uint32_t *hist = smem + kRssfTabWords;
	{
		const CGCK_GLOBAL u32x4_t *gt = (const CGCK_GLOBAL u32x4_t *)p.tab;
		u32x4_t *lt = reinterpret_cast<u32x4_t *>(T);
		for (uint32_t i = threadIdx.x; i < kRssfTabWords / 4; i += kRssfThreads)
			lt[i] = gt[i];
		if (Q && threadIdx.x < kRssfBins)
			hist[threadIdx.x] = 0;
	}
	__syncthreads();

	const int lane = threadIdx.x & 63;
	const uint64_t nsteps = (p.n + 63) / 64;
	const uint64_t W = (uint64_t)gridDim.x * kRssfWaves;
	uint64_t s = (uint64_t)blockIdx.x * kRssfWaves + (threadIdx.x >> 6);
	const bool count = Q && p.qcount != nullptr;

	if (s < nsteps) {
		// step s: descriptor and chunks; step s + W: descriptor
		const RDesc dc = rssf_desc<DESC>(p, s * 64 + lane);
		uint64_t a0;
		uint32_t len;
		frame_of<DESC>(p, dc, s * 64 + lane, a0, len);
		RChunks cc = rssf_first(a0, len, p.zero, lane);
		RDesc dn = rssf_desc<DESC>(p, (s + W) * 64 + lane);
		for (; s < nsteps; s += W) {
			// step s + W's chunks and step s + 2W's descriptor go out before
			// step s is hashed (past the end: no frame, the zero chunk)
			uint64_t a0n;
			uint32_t lenn;
			frame_of<DESC>(p, dn, (s + W) * 64 + lane, a0n, lenn);
			const RChunks cn = rssf_first(a0n, lenn, p.zero, lane);
			const RDesc dn2 = rssf_desc<DESC>(p, (s + 2 * W) * 64 + lane);

			const uint64_t k = s * 64 + lane;
			const bool ok = k < p.n;
			// frame-relative dwords R0 .. R10 = bytes [0, 44)
			uint32_t D[16];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				D[4 * i + 0] = cc.c[i][0];
				D[4 * i + 1] = cc.c[i][1];
				D[4 * i + 2] = cc.c[i][2];
				D[4 * i + 3] = cc.c[i][3];
			}
			const uint32_t q = (uint32_t)(a0 & 15);
			const uint32_t m1 = opaque((q & 4) ? ~0u : 0u), m2 = opaque((q & 8) ? ~0u : 0u);
			uint32_t S[12], R[11];
#pragma unroll
			for (int i = 0; i < 12; ++i)
				S[i] = pick(m2, pick(m1, D[i + 3], D[i + 2]), pick(m1, D[i + 1], D[i]));
#pragma unroll
			for (int i = 0; i < 11; ++i)
				R[i] = __builtin_amdgcn_alignbyte(S[i + 1], S[i], q & 3u);

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
					if (off > len) {
						kind = CGCK_BAD_LEN;
						walk = false;
					} else if (nh == 44) {
						nd = 8;
						kind = CGCK_RSS_IP6;
						walk = false;
					} else if (!v6_is_ext(nh)) {
						const bool l4 = len >= off + 4 && ((nh == 6 && (p.hf & CGCK_RSS_TCP)) ||
										     (nh == 17 && (p.hf & CGCK_RSS_UDP)));
						nd = l4 ? 9 : 8;
						kind = CGCK_RSS_IP6 | (l4 ? CGCK_RSS_L4 : 0);
						walk = false;
						ports = R[10];
						prt = l4 && off != 40;
					} else if (seen == (uint32_t)kRssfMaxExt || off + 2 > len) {
						kind = CGCK_BAD_LEN;
						walk = false;
					} else {
						ext = true;
					}
				}
				if (!__any(ext || prt))
					break;
				if (ext || prt) {
					const uint32_t w = rssf_dword_at(a0, len, off);
					if (ext) {
						const uint32_t hlen = (w >> 8) & 255u;
						off += nh == 51 ? (hlen + 2) * 4 : (hlen + 1) * 8;
						nh = w & 255u;
						++seen;
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

			dn = dn2;
			cc = cn;
			a0 = a0n;
			len = lenn;
		}
	}
	if (Q) {
		__syncthreads();
		if (count && threadIdx.x < kRssfBins && threadIdx.x < p.queue_num) {
			const uint32_t cnt = hist[threadIdx.x];
			if (cnt)
				__hip_atomic_fetch_add((CGCK_GLOBAL uint32_t *)p.qcount + threadIdx.x, cnt, __ATOMIC_RELAXED,
						       __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

hipError_t launch_rssf(const RssfParams &p, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const uint64_t steps = (p.n + 63) / 64;
	const uint64_t want = (steps + kRssfWaves - 1) / kRssfWaves;
	const uint64_t cap = (uint64_t)num_cus * kRssfWgPerCu;
	const dim3 g((unsigned)(want < cap ? want : cap)), b(kRssfThreads);
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
