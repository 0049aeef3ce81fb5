// cgck_frame.h — what the one-lane-per-frame kernels over a descriptor burst
// share (rssf_kernel, l2d_kernel, l4d_kernel: cgck_rssf.hip, cgck_l2d.hip,
// cgck_l4d.hip).  Each kernel keeps its rules, its second load round, its tables
// and its outputs; the walk over the burst and the way frame bytes reach
// registers are here, once.
//
// Shape.  One lane per frame, 64 frames per wave-step, waves grid-stride over
// the steps; four 256-thread workgroups per CU (frame_grid).  FrameCursor holds a
// wave's place: the descriptors of step s + 2W and the chunks of step s + W are
// loaded before step s is judged (W: the waves of the grid), so each wave keeps
// two steps of loads in flight behind its work.
//
// Memory.  A kernel is a gather of the first NC granules of every frame.  Each
// lane loads, unconditionally, NC aligned 16-byte chunks from the frame's first
// granule on (frame_first) — they cover the frame-relative bytes [0, 16 NC - 16)
// at any byte alignment — and realigns them in registers (frame_realign: v_bfi
// selects by the dword shift, v_alignbyte by the byte shift): no byte loads.
// Chunk indices are clamped to the granules that hold a byte of
// [frame, frame + len) (ldc's rule, cgck_device.h), so no load touches a granule
// before a frame's first or after its last; a lane without a frame reads the zero
// chunk.  A byte past len may come back as anything: every rule compares a
// length before it consults a byte.
//
// Counters go through an LDS histogram (ds_add), and each workgroup adds its
// non-zero bins to global memory once, after its loop (frame_hist_*).  Records
// of more than a dword per frame are turned through LDS and leave as consecutive
// pieces (wave_turn_store).
#pragma once
#include "cgck_device.h"

namespace cgck {

constexpr int kFrameThreads = 256;
constexpr int kFrameWaves = kFrameThreads / 64;
constexpr int kFrameWgPerCu = 4;

// Workgroups of a launch over n frames: one wave-step per wave, at most a pass
// (frame_pass_frames, cgck_internal.h, gives the host a pass in frames).
inline unsigned frame_grid(uint64_t n, int num_cus)
{
	const uint64_t steps = (n + 63) / 64;
	const uint64_t want = (steps + kFrameWaves - 1) / kFrameWaves;
	const uint64_t cap = (uint64_t)num_cus * kFrameWgPerCu;
	return (unsigned)(want < cap ? want : cap);
}

struct FDesc {
	uint32_t lo, hi, w2;
};

template <int NC>
struct FChunks {
	u32x4_t c[NC];
};

// Descriptor of frame k of n (index clamped: the lanes past n of the last step
// re-read the last descriptor and drop it in frame_at).
__device__ __forceinline__ FDesc frame_desc(const void *desc, uint64_t n, uint64_t k)
{
	const uint64_t kk = k < n ? k : n - 1;
	const CGCK_GLOBAL uint32_t *g = (const CGCK_GLOBAL uint32_t *)desc + 3 * kk;
	FDesc d;
	d.lo = g[0];
	d.hi = g[1];
	d.w2 = g[2];
	return d;
}

// a0: the address of the descriptor's first byte; len: its bytes (0: no frame).
__device__ __forceinline__ void frame_at(const uint8_t *base, const FDesc &d, bool live, uint64_t &a0, uint32_t &len)
{
	a0 = reinterpret_cast<uint64_t>(base) + (((uint64_t)d.hi << 32) | d.lo) + (d.w2 & 0xffffu);
	len = live ? d.w2 >> 16 : 0;
}

// Granules that hold a byte of [a0, a0 + len).
__device__ __forceinline__ int frame_granules(uint64_t a0, uint32_t len)
{
	return len ? (int)(((uint32_t)(a0 & 15) + len + 15) >> 4) : 0;
}

// The frame's first NC granules, clamped to its last; the zero chunk for a lane
// without a byte.
template <int NC>
__device__ __forceinline__ FChunks<NC> frame_first(uint64_t a0, uint32_t len, const void *zero, int lane)
{
	const int nch = frame_granules(a0, len);
	FChunks<NC> r;
#pragma unroll
	for (int i = 0; i < NC; ++i) {
		const uint64_t at = nch > 0 ? (a0 & ~(uint64_t)15) + 16u * (uint32_t)min(i, nch - 1)
					    : reinterpret_cast<uint64_t>(zero) + 64u * (uint32_t)lane;
		r.c[i] = *gbl_at<const u32x4_t>(at);
	}
	return r;
}

// NC chunks whose first holds byte q (0..15) of the run wanted: the first NR
// dwords from that byte on, NR <= 4 NC - 4.
template <int NC, int NR>
__device__ __forceinline__ void frame_realign(const u32x4_t (&c)[NC], uint32_t q, uint32_t (&R)[NR])
{
	static_assert(NR <= 4 * NC - 4, "the last dword needs a chunk behind it");
	uint32_t D[4 * NC];
#pragma unroll
	for (int i = 0; i < NC; ++i) {
		D[4 * i + 0] = c[i][0];
		D[4 * i + 1] = c[i][1];
		D[4 * i + 2] = c[i][2];
		D[4 * i + 3] = c[i][3];
	}
	const uint32_t m1 = opaque((q & 4) ? ~0u : 0u), m2 = opaque((q & 8) ? ~0u : 0u);
	uint32_t S[NR + 1];
#pragma unroll
	for (int i = 0; i < NR + 1; ++i)
		S[i] = pick(m2, pick(m1, D[i + 3], D[i + 2]), pick(m1, D[i + 1], D[i]));
#pragma unroll
	for (int i = 0; i < NR; ++i)
		R[i] = __builtin_amdgcn_alignbyte(S[i + 1], S[i], q & 3u);
}

// The frame-relative dword at byte `off` (a multiple of 4, off + 2 <= len):
// the one or two granules that hold it, realigned.  Bytes of it past the
// frame's last granule come back as that granule's; the callers consult only
// bytes below len.
__device__ __forceinline__ uint32_t frame_dword_at(uint64_t a0, uint32_t len, uint32_t off)
{
	const int nch = frame_granules(a0, len);
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

// --------------------------------------------------------------------------
// The IPv6 extension walk, a header a pass (CGCK_IP6's rules, v6_walk in
// cgck_device.h, without its checksum-field clause).  A lane's state is `off`,
// the byte its next header starts at (40 at first), `nh`, that header's
// protocol, and `seen`, the extension headers behind it.  The kernel loops
// behind a wave-wide __any, switches on v6_next and, on kV6More, reads
// frame_dword_at(a0, len, off) and takes its next state from v6_eat.
// --------------------------------------------------------------------------

enum V6Next {
	kV6Past,  // the header starts past the frame's end
	kV6Frag,  // a Fragment header: no upper-layer header to speak of
	kV6Upper, // nh is the upper-layer protocol, its header at off
	kV6Cut,   // a ninth extension header, or one cut before its length byte
	kV6More,  // an extension header to read
};

__device__ __forceinline__ V6Next v6_next(uint32_t off, uint32_t len, uint32_t nh, uint32_t seen)
{
	if (off > len)
		return kV6Past;
	if (nh == 44)
		return kV6Frag;
	if (!v6_is_ext(nh))
		return kV6Upper;
	if (seen == (uint32_t)kV6MaxExt || off + 2 > len)
		return kV6Cut;
	return kV6More;
}

// The state behind the extension header whose first dword is w: Hop-by-Hop,
// Routing and Destination Options are (b[1] + 1) * 8 bytes, AH (b[1] + 2) * 4.
// By value: with reference parameters the walk's loop compiled to 4 to 7 % more
// code in both kernels.
struct V6At {
	uint32_t off, nh, seen;
};

__device__ __forceinline__ V6At v6_eat(uint32_t w, uint32_t off, uint32_t nh, uint32_t seen)
{
	const uint32_t hlen = (w >> 8) & 255u;
	return {off + (nh == 51 ? (hlen + 2) * 4 : (hlen + 1) * 8), w & 255u, seen + 1};
}

// --------------------------------------------------------------------------
// The step cursor
// --------------------------------------------------------------------------

// Where frame k of a burst of n lies: the descriptor form.  A source has
// load(k), the words to fetch ahead for frame k, and at(d, k, a0, len).
struct FrameDescs {
	const uint8_t *base;
	const void *desc;
	uint64_t n;

	__device__ __forceinline__ FDesc load(uint64_t k) const
	{
		return frame_desc(desc, n, k);
	}
	__device__ __forceinline__ void at(const FDesc &d, uint64_t k, uint64_t &a0, uint32_t &len) const
	{
		frame_at(base, d, k < n, a0, len);
	}
};

// A wave's place in the burst.  In a step's body d, a0, len and c are the
// lane's frame of step s (frame k()); the rest is on its way.
//
//	FrameCursor<NC, SRC> cur(src, n, zero);
//	if (cur.more())
//		for (cur.start(); cur.more(); cur.advance()) {
//			cur.ahead();
//			... step cur.s ...
//		}
template <int NC, class SRC>
struct FrameCursor {
	const SRC &src;
	const void *zero;
	const int lane;
	const uint64_t nsteps, W;
	uint64_t s;
	FDesc d, dn, dn2; // the descriptors of steps s, s + W, s + 2W
	uint64_t a0, a0n;
	uint32_t len, lenn;
	FChunks<NC> c, cn; // the chunks of steps s, s + W

	__device__ __forceinline__ FrameCursor(const SRC &src_, uint64_t n, const void *zero_)
		: src(src_), zero(zero_), lane(threadIdx.x & 63), nsteps((n + 63) / 64),
		  W((uint64_t)gridDim.x * kFrameWaves), s((uint64_t)blockIdx.x * kFrameWaves + (threadIdx.x >> 6))
	{
	}

	__device__ __forceinline__ bool more() const
	{
		return s < nsteps;
	}
	__device__ __forceinline__ uint64_t k() const
	{
		return s * 64 + lane;
	}
	// step s: descriptor and chunks; step s + W: descriptor
	__device__ __forceinline__ void start()
	{
		d = src.load(k());
		src.at(d, k(), a0, len);
		c = frame_first<NC>(a0, len, zero, lane);
		dn = src.load((s + W) * 64 + lane);
	}
	// First in a step's body: step s + W's chunks and step s + 2W's descriptor
	// go out before step s is judged (past the end: no frame, the zero chunk).
	__device__ __forceinline__ void ahead()
	{
		src.at(dn, (s + W) * 64 + lane, a0n, lenn);
		cn = frame_first<NC>(a0n, lenn, zero, lane);
		dn2 = src.load((s + 2 * W) * 64 + lane);
	}
	__device__ __forceinline__ void advance()
	{
		d = dn;
		dn = dn2;
		c = cn;
		a0 = a0n;
		len = lenn;
		s += W;
	}
};

// --------------------------------------------------------------------------
// LDS counters and turned stores
// --------------------------------------------------------------------------

// Zero the workgroup's bins; the caller's __syncthreads comes before the first add.
__device__ __forceinline__ void frame_hist_zero(uint32_t *hist, uint32_t bins)
{
	if (threadIdx.x < bins)
		hist[threadIdx.x] = 0;
}

// After the loop: add the workgroup's non-zero bins to `global` (nullptr: none).
__device__ __forceinline__ void frame_hist_flush(const uint32_t *hist, uint32_t bins, uint32_t *global)
{
	__syncthreads();
	if (global != nullptr && threadIdx.x < bins) {
		const uint32_t cnt = hist[threadIdx.x];
		if (cnt)
			__hip_atomic_fetch_add((CGCK_GLOBAL uint32_t *)global + threadIdx.x, cnt, __ATOMIC_RELAXED,
					       __HIP_MEMORY_SCOPE_AGENT);
	}
}

// A wave-step's records, PER pieces of type T a lane, are 64 PER consecutive
// pieces at g.  Each lane puts `mine` into the wave's own LDS block xs
// (T[64 PER]) and the wave stores the block as PER instructions of 64
// consecutive pieces instead of PER at a lane stride; `left` = the frames from
// the step's first on (a last step stores 64 or fewer records).  Plain vector
// stores.
template <class T, int PER>
__device__ __forceinline__ void wave_turn_store(T *xs, const T (&mine)[PER], CGCK_GLOBAL T *g, uint64_t left, int lane)
{
#pragma unroll
	for (int j = 0; j < PER; ++j)
		xs[PER * lane + j] = mine[j];
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
	const uint32_t nv = PER * (uint32_t)(left < 64 ? left : 64);
#pragma unroll
	for (int j = 0; j < PER; ++j)
		if ((uint32_t)(64 * j + lane) < nv)
			g[64 * j + lane] = xs[64 * j + lane];
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
}

} // namespace cgck
