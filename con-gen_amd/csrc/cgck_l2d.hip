// cgck_l2d.hip — classify and trim a raw Ethernet burst (cgck_l2_desc,
// include/cgck.h section 3): ether_input's demultiplex (bsd44/if_ether.c:152-183)
// and ip_input's length rules (ip_input.c:28-44, 63-79) over a device-resident
// burst.  It turns the transport's {frame offset, delivered bytes} into the
// descriptors every other call takes: the IP header found behind up to two VLAN
// tags, Ethernet padding cut off by the header's own length field.
//
// Shape.  rssf_kernel's (cgck_rssf.hip): one lane per frame, 64 frames per
// wave-step, waves grid-stride over the steps, the descriptors of step s + 2 and
// the chunks of step s + 1 loaded before step s is judged.
//
// Memory.  Everything the rules consult lies in the frame's first 28 bytes: the
// destination address, the ethertype, two tags, and the first six bytes of the IP
// header behind them (14 + 8 + 6).  At any start alignment those are covered by
// the three aligned 16-byte chunks from the frame's first granule on ([0, 33) at
// the least), loaded unconditionally and realigned in registers as rssf does
// (v_bfi by the dword shift, v_alignbyte by the byte shift): no byte loads and no
// second load round.  Chunk indices are clamped to the granules that hold a byte
// of [frame, frame + L); a lane without a frame reads the zero chunk.  A byte past
// L may come back as anything: every rule compares L before it consults a byte.
//
// Stores.  A wave-step's 64 output descriptors are 768 consecutive bytes.  Each
// lane puts its three dwords into the wave's own LDS row and the wave stores the
// row as three instructions of 64 consecutive dwords; three stores at a 12-byte
// lane stride took 0.525 ms where these take 0.484 on the 16M-frame set
// (profiles/l2d/).  Plain vector stores, any 4-byte alignment of desc_out.
//
// The kernel has no tables: 3 KiB of LDS for the rows and 48 bytes for the 12
// counters, four 256-thread workgroups per CU, as rssf runs.  Counters go through
// an LDS histogram (ds_add), and each workgroup adds its non-zero bins to global
// memory once.
//
// The chunk helpers are private copies of rssf's, so that rssf_kernel's device
// code does not depend on this unit.
#include "cgck_device.h"

namespace cgck {

constexpr int kL2dThreads = 256;
constexpr int kL2dWaves = kL2dThreads / 64;
constexpr int kL2dWgPerCu = 4;
constexpr uint32_t kL2dBins = CGCK_L2_NCOUNT;

struct LDesc {
	uint32_t lo, hi, w2;
};

struct LChunks {
	u32x4_t c[3];
};

// Raw descriptor of frame k (index clamped: the lanes past n of the last step
// re-read the last descriptor and drop it in l2d_frame).
__device__ __forceinline__ LDesc l2d_desc(const L2dParams &p, uint64_t k)
{
	const uint64_t kk = k < p.n ? k : p.n - 1;
	const CGCK_GLOBAL uint32_t *g = (const CGCK_GLOBAL uint32_t *)p.raw + 3 * kk;
	LDesc d;
	d.lo = g[0];
	d.hi = g[1];
	d.w2 = g[2];
	return d;
}

// a0: the Ethernet header's address; len: the bytes delivered (0: no frame).
__device__ __forceinline__ void l2d_frame(const L2dParams &p, const LDesc &d, uint64_t k, uint64_t &a0, uint32_t &len)
{
	a0 = reinterpret_cast<uint64_t>(p.base) + (((uint64_t)d.hi << 32) | d.lo) + (d.w2 & 0xffffu);
	len = k < p.n ? d.w2 >> 16 : 0;
}

// The first three granules that hold a byte of [a0, a0 + len), clamped to the
// last of them; the zero chunk for a lane without a byte.
__device__ __forceinline__ LChunks l2d_first(uint64_t a0, uint32_t len, const void *zero, int lane)
{
	const int nch = len ? (int)(((uint32_t)(a0 & 15) + len + 15) >> 4) : 0;
	LChunks r;
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		const uint64_t at = nch > 0 ? (a0 & ~(uint64_t)15) + 16u * (uint32_t)min(i, nch - 1)
					    : reinterpret_cast<uint64_t>(zero) + 64u * (uint32_t)lane;
		r.c[i] = *gbl_at<const u32x4_t>(at);
	}
	return r;
}

// Big-endian 16-bit field in the low half of a little-endian load.
__device__ __forceinline__ uint32_t be16_lo(uint32_t w)
{
	return ((w & 255u) << 8) | ((w >> 8) & 255u);
}

__device__ __forceinline__ bool is_tpid(uint32_t et)
{
	return et == 0x8100u || et == 0x88A8u;
}

// D: desc_out is written; C: cls and / or the counters.
template <bool D, bool C>
__global__ __launch_bounds__(kL2dThreads) void l2d_kernel(L2dParams p)
{
	__shared__ uint32_t hist[kL2dBins];
	__shared__ uint32_t xpose[D ? kL2dWaves : 1][192]; // a wave-step's descriptors on their way out
	const bool count = C && p.count != nullptr;
	if (C) {
		if (threadIdx.x < kL2dBins)
			hist[threadIdx.x] = 0;
		__syncthreads();
	}

	const int lane = threadIdx.x & 63;
	const uint64_t nsteps = (p.n + 63) / 64;
	const uint64_t W = (uint64_t)gridDim.x * kL2dWaves;
	uint64_t s = (uint64_t)blockIdx.x * kL2dWaves + (threadIdx.x >> 6);

	if (s < nsteps) {
		// step s: descriptor and chunks; step s + W: descriptor
		LDesc dc = l2d_desc(p, s * 64 + lane);
		uint64_t a0;
		uint32_t len;
		l2d_frame(p, dc, s * 64 + lane, a0, len);
		LChunks cc = l2d_first(a0, len, p.zero, lane);
		LDesc dn = l2d_desc(p, (s + W) * 64 + lane);
		for (; s < nsteps; s += W) {
			// step s + W's chunks and step s + 2W's descriptor go out before
			// step s is judged (past the end: no frame, the zero chunk)
			uint64_t a0n;
			uint32_t lenn;
			l2d_frame(p, dn, (s + W) * 64 + lane, a0n, lenn);
			const LChunks cn = l2d_first(a0n, lenn, p.zero, lane);
			const LDesc dn2 = l2d_desc(p, (s + 2 * W) * 64 + lane);

			const uint64_t k = s * 64 + lane;
			const bool ok = k < p.n;
			// frame-relative dwords R0 .. R6 = bytes [0, 28)
			uint32_t Dw[12];
#pragma unroll
			for (int i = 0; i < 3; ++i) {
				Dw[4 * i + 0] = cc.c[i][0];
				Dw[4 * i + 1] = cc.c[i][1];
				Dw[4 * i + 2] = cc.c[i][2];
				Dw[4 * i + 3] = cc.c[i][3];
			}
			const uint32_t q = (uint32_t)(a0 & 15);
			const uint32_t m1 = opaque((q & 4) ? ~0u : 0u), m2 = opaque((q & 8) ? ~0u : 0u);
			uint32_t S[8], R[7];
#pragma unroll
			for (int i = 0; i < 8; ++i)
				S[i] = pick(m2, pick(m1, Dw[i + 3], Dw[i + 2]), pick(m1, Dw[i + 1], Dw[i]));
#pragma unroll
			for (int i = 0; i < 7; ++i)
				R[i] = __builtin_amdgcn_alignbyte(S[i + 1], S[i], q & 3u);

			const uint32_t L = len;
			const uint32_t l3 = dc.w2 & 0xffffu;
			// rule 2: the tag walk (bytes 12-13, 16-17, 20-21)
			uint32_t et = be16_lo(R[3]), off = 14, tags = 0;
			bool runt = L < 14;
			if (!runt && is_tpid(et)) {
				if (L < 18) {
					runt = true;
				} else {
					et = be16_lo(R[4]);
					off = 18;
					tags = 1;
					if (is_tpid(et)) {
						if (L < 22) {
							runt = true;
						} else {
							et = be16_lo(R[5]);
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
				const uint32_t hl = (B0 & 15u) * 4, total = be16_lo(B0 >> 16);
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
				const uint32_t total = 40 + be16_lo(B1);
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
				// The step's 64 descriptors are 192 consecutive dwords: turned
				// through the wave's LDS rows (stride 3: no bank conflict) they go
				// out as three stores of 64 consecutive dwords instead of three at
				// a 12-byte stride.
				uint32_t *xs = xpose[threadIdx.x >> 6];
				xs[3 * lane + 0] = dc.lo;
				xs[3 * lane + 1] = dc.hi;
				xs[3 * lane + 2] = (ip_len << 16) | (cls == CGCK_L2_RUNT ? l3 : l3 + off);
				__builtin_amdgcn_wave_barrier();
				asm volatile("" ::: "memory");
				const uint64_t left = p.n - s * 64;
				const uint32_t nv = 3 * (uint32_t)(left < 64 ? left : 64);
				CGCK_GLOBAL uint32_t *g = (CGCK_GLOBAL uint32_t *)p.desc_out + 192 * s;
#pragma unroll
				for (int j = 0; j < 3; ++j)
					if ((uint32_t)(64 * j + lane) < nv)
						g[64 * j + lane] = xs[64 * j + lane];
				__builtin_amdgcn_wave_barrier();
				asm volatile("" ::: "memory");
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

			dc = dn;
			dn = dn2;
			cc = cn;
			a0 = a0n;
			len = lenn;
		}
	}
	if (C) {
		__syncthreads();
		if (count && threadIdx.x < kL2dBins) {
			const uint32_t cnt = hist[threadIdx.x];
			if (cnt)
				__hip_atomic_fetch_add((CGCK_GLOBAL uint32_t *)p.count + threadIdx.x, cnt, __ATOMIC_RELAXED,
						       __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

uint64_t l2d_pass_frames(int num_cus)
{
	return (uint64_t)num_cus * kL2dWgPerCu * kL2dThreads;
}

hipError_t launch_l2d(const L2dParams &p, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const uint64_t steps = (p.n + 63) / 64;
	const uint64_t want = (steps + kL2dWaves - 1) / kL2dWaves;
	const uint64_t cap = (uint64_t)num_cus * kL2dWgPerCu;
	const dim3 g((unsigned)(want < cap ? want : cap)), b(kL2dThreads);
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
