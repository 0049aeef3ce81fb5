// cgck_steer.hip — stable counting partition of a burst by queue id (cgck_steer,
// cgck_rss_steer_desc; include/cgck.h section 3): from rssf's
// one byte per frame to per-queue slot ranges (qoff), the permutation both ways
// (perm, slot) and the descriptors in queue order (desc_out), so that worker q
// verifies desc_out[qoff[q] .. qoff[q + 1]) without a host pass.
//
// bin(k) = queue[k] when it is below queue_num, else queue_num (the unsteered
// bin: rssf's 0xFF and every other byte); slots ascend by bin, and within a bin
// by arrival index k.
//
// Shape.  A tile is p.tile frames (steer_plan, cgck_steer_plan.h), one workgroup
// of four waves per tile, the tile cut into one contiguous sub-range per wave.
// Three ordinary launches, no workgroup ever waits for another:
//   steer_count_kernel    each wave counts its sub-range per bin into its own LDS
//                         row; the workgroup writes the tile's column of
//                         hist[bin][tile] (bin-major, the caller's workspace).
//   steer_scan_kernel     one workgroup scans hist in place, exclusive, read
//                         linearly: word (bin, tile) becomes the first slot of
//                         that tile's frames of that bin.  qoff[q] is word (q, 0).
//   steer_scatter_kernel  the count's geometry.  Each wave recounts its sub-range
//                         (1 B per frame), the rows are prefixed across the waves
//                         and added to the tile's scanned column, then each wave
//                         walks its sub-range in order, 64 frames per step: a
//                         lane's rank among the step's lanes of its bin comes from
//                         one __ballot per bit of the bin, the wave's row holds
//                         the bin's next slot, the lowest lane of each bin
//                         advances it.
// One tile (every receive burst): steer_one_kernel does all of it in one launch
// of one workgroup, the scan of the bins in LDS, and uses no workspace.
//
// Memory.  queue[] is read one byte per lane, coalesced, the next step's byte
// before this step is ranked; desc_in[k] is three dwords per lane at 12 k
// (independent of the bin, so issued before the ballots); slot[k] is written
// coalesced; perm[s] and desc_out[s] go to consecutive slots for consecutive
// frames of one queue.  Every count and offset is an ordinary vector store.
#include "cgck_device.h"
#include "cgck_steer_plan.h"

namespace cgck {

static_assert(kSteerThreads == 256 && kSteerScanThreads == 1024, "the kernels' launch bounds");

__device__ __forceinline__ uint32_t steer_bin(const SteerParams &p, uint64_t k)
{
	const uint32_t q = ((const CGCK_GLOBAL uint8_t *)p.queue)[k];
	return q < p.queue_num ? q : p.queue_num;
}

// The sub-range [k0, k1) of wave w of tile t.
__device__ __forceinline__ void steer_range(const SteerParams &p, uint32_t t, uint32_t w, uint64_t &k0, uint64_t &k1)
{
	const uint64_t lo = (uint64_t)t * p.tile, hi = lo + p.tile < p.n ? lo + p.tile : p.n;
	k0 = lo + (uint64_t)w * p.per_wave;
	k0 = k0 < hi ? k0 : hi;
	k1 = k0 + p.per_wave < hi ? k0 + p.per_wave : hi;
}

// Zero the rows, then each wave counts its sub-range into its own row.
__device__ __forceinline__ void steer_count(const SteerParams &p, uint32_t (*rows)[kSteerMaxBins], uint64_t k0,
					    uint64_t k1)
{
	uint32_t *all = &rows[0][0];
	for (uint32_t i = threadIdx.x; i < kSteerWaves * kSteerMaxBins; i += kSteerThreads)
		all[i] = 0;
	__syncthreads();
	uint32_t *row = rows[threadIdx.x >> 6];
	for (uint64_t k = k0 + (threadIdx.x & 63); k < k1; k += 64)
		__hip_atomic_fetch_add(row + steer_bin(p, k), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	__syncthreads();
}

// Bin b's rows become each wave's first slot: base, base + row[0][b], ...
__device__ __forceinline__ void steer_prefix_rows(uint32_t (*rows)[kSteerMaxBins], uint32_t b, uint32_t base)
{
#pragma unroll
	for (uint32_t w = 0; w < kSteerWaves; ++w) {
		const uint32_t c = rows[w][b];
		rows[w][b] = base;
		base += c;
	}
}

// Exclusive scan of one value per thread over a workgroup of NW waves; `total`
// is the workgroup's sum.  wsum: NW words of LDS, free again on return.
template <int NW>
__device__ __forceinline__ uint32_t steer_block_scan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(inc, d);
		if (lane >= d)
			inc += o;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	uint32_t off = 0, sum = 0;
#pragma unroll
	for (int i = 0; i < NW; ++i) {
		const uint32_t x = wsum[i];
		off += i < w ? x : 0u;
		sum += x;
	}
	__syncthreads();
	total = sum;
	return off + inc - v;
}

// One wave walks [k0, k1) in order; row[b] is bin b's next slot.
template <bool PERM, bool SLOT, bool DESC>
__device__ __forceinline__ void steer_walk(const SteerParams &p, volatile uint32_t *row, uint64_t k0, uint64_t k1)
{
	const int lane = threadIdx.x & 63;
	const uint64_t below = (1ull << lane) - 1;
	uint32_t bn = k0 + lane < k1 ? steer_bin(p, k0 + lane) : 0u;
	for (uint64_t kb = k0; kb < k1; kb += 64) {
		const uint64_t k = kb + lane;
		const bool ok = k < k1;
		const uint32_t b = bn;
		bn = k + 64 < k1 ? steer_bin(p, k + 64) : 0u;
		uint32_t d0 = 0, d1 = 0, d2 = 0;
		if (DESC && ok) {
			const CGCK_GLOBAL uint32_t *g = (const CGCK_GLOBAL uint32_t *)p.desc_in + 3 * k;
			d0 = g[0];
			d1 = g[1];
			d2 = g[2];
		}
		// the step's lanes of this lane's bin
		uint64_t m = __ballot(ok);
		for (uint32_t i = 0; i < p.nbits; ++i) {
			const bool bit = (b >> i) & 1u;
			const uint64_t bi = __ballot(bit);
			m &= bit ? bi : ~bi;
		}
		uint32_t s = 0;
		if (ok)
			s = row[b] + (uint32_t)__popcll(m & below);
		__builtin_amdgcn_wave_barrier();
		if (ok && (m & below) == 0)
			row[b] = s + (uint32_t)__popcll(m);
		__builtin_amdgcn_wave_barrier();
		if (ok) {
			if (PERM)
				((CGCK_GLOBAL uint32_t *)p.perm)[s] = (uint32_t)k;
			if (SLOT)
				((CGCK_GLOBAL uint32_t *)p.slot)[k] = s;
			if (DESC) {
				CGCK_GLOBAL uint32_t *o = (CGCK_GLOBAL uint32_t *)p.desc_out + 3 * (uint64_t)s;
				o[0] = d0;
				o[1] = d1;
				o[2] = d2;
			}
		}
	}
}

__global__ __launch_bounds__(kSteerThreads) void steer_count_kernel(SteerParams p)
{
	__shared__ uint32_t rows[kSteerWaves][kSteerMaxBins];
	uint64_t k0, k1;
	steer_range(p, blockIdx.x, threadIdx.x >> 6, k0, k1);
	steer_count(p, rows, k0, k1);
	const uint32_t b = threadIdx.x;
	if (b <= p.queue_num) {
		uint32_t c = 0;
#pragma unroll
		for (uint32_t w = 0; w < kSteerWaves; ++w)
			c += rows[w][b];
		((CGCK_GLOBAL uint32_t *)p.hist)[(uint64_t)b * p.tiles + blockIdx.x] = c;
	}
}

__global__ __launch_bounds__(kSteerScanThreads) void steer_scan_kernel(SteerParams p)
{
	__shared__ uint32_t wsum[kSteerScanThreads / 64];
	CGCK_GLOBAL uint32_t *hist = (CGCK_GLOBAL uint32_t *)p.hist;
	CGCK_GLOBAL uint32_t *qoff = (CGCK_GLOBAL uint32_t *)p.qoff;
	const uint32_t words = p.tiles * (p.queue_num + 1); // within kSteerBudget
	uint32_t carry = 0;
	for (uint32_t base = 0; base < words; base += kSteerScanPass) {
		const uint32_t i0 = base + kSteerScanPer * threadIdx.x;
		uint32_t v[kSteerScanPer], sum = 0, total;
#pragma unroll
		for (uint32_t j = 0; j < kSteerScanPer; ++j) {
			v[j] = i0 + j < words ? hist[i0 + j] : 0u;
			sum += v[j];
		}
		uint32_t run = carry + steer_block_scan<kSteerScanThreads / 64>(sum, wsum, total);
#pragma unroll
		for (uint32_t j = 0; j < kSteerScanPer; ++j) {
			if (i0 + j < words) {
				hist[i0 + j] = run;
				if (qoff && (i0 + j) % p.tiles == 0)
					qoff[(i0 + j) / p.tiles] = run;
			}
			run += v[j];
		}
		carry += total;
	}
	if (qoff && threadIdx.x == 0)
		qoff[p.queue_num + 1] = (uint32_t)p.n;
}

template <bool PERM, bool SLOT, bool DESC>
__global__ __launch_bounds__(kSteerThreads) void steer_scatter_kernel(SteerParams p)
{
	__shared__ uint32_t rows[kSteerWaves][kSteerMaxBins];
	uint64_t k0, k1;
	steer_range(p, blockIdx.x, threadIdx.x >> 6, k0, k1);
	steer_count(p, rows, k0, k1);
	const uint32_t b = threadIdx.x;
	if (b <= p.queue_num)
		steer_prefix_rows(rows, b, ((const CGCK_GLOBAL uint32_t *)p.hist)[(uint64_t)b * p.tiles + blockIdx.x]);
	__syncthreads();
	steer_walk<PERM, SLOT, DESC>(p, rows[threadIdx.x >> 6], k0, k1);
}

template <bool PERM, bool SLOT, bool DESC>
__global__ __launch_bounds__(kSteerThreads) void steer_one_kernel(SteerParams p)
{
	__shared__ uint32_t rows[kSteerWaves][kSteerMaxBins];
	__shared__ uint32_t wsum[kSteerWaves];
	uint64_t k0, k1;
	steer_range(p, 0, threadIdx.x >> 6, k0, k1);
	steer_count(p, rows, k0, k1);
	const uint32_t b = threadIdx.x;
	uint32_t c = 0, total;
	if (b <= p.queue_num) {
#pragma unroll
		for (uint32_t w = 0; w < kSteerWaves; ++w)
			c += rows[w][b];
	}
	const uint32_t first = steer_block_scan<kSteerWaves>(c, wsum, total);
	CGCK_GLOBAL uint32_t *qoff = (CGCK_GLOBAL uint32_t *)p.qoff;
	if (b <= p.queue_num) {
		if (qoff)
			qoff[b] = first;
		steer_prefix_rows(rows, b, first);
	}
	if (qoff && b == 0)
		qoff[p.queue_num + 1] = total;
	if (PERM || SLOT || DESC) {
		__syncthreads();
		steer_walk<PERM, SLOT, DESC>(p, rows[threadIdx.x >> 6], k0, k1);
	}
}

// p.tile, p.tiles: steer_plan(p.n, p.queue_num); p.hist: the workspace (unused
// with one tile).  nbits and per_wave are set here.
hipError_t launch_steer(const SteerParams &in, hipStream_t st)
{
	if (in.n == 0)
		return hipSuccess;
	SteerParams p = in;
	p.nbits = 32u - (uint32_t)__builtin_clz(p.queue_num); // the bins are 0 .. queue_num
	// lab build only: a one-tile call that brings a workspace of queue_num + 1
	// words takes the three launches (tools/steer_ab.py times both)
	static const bool lab_three = CGCK_ENV("CGCK_STEER_THREE") != nullptr;
	const bool one = p.tiles <= 1 && !(lab_three && p.hist);
	// one tile: the waves share the burst's steps evenly instead of 16 steps each
	p.per_wave = p.tiles <= 1 ? (uint32_t)((((p.n + kSteerWaves - 1) / kSteerWaves) + 63) / 64 * 64) : p.tile / kSteerWaves;
	const dim3 g(p.tiles), b(kSteerThreads);
	const int outs = (p.perm ? 4 : 0) | (p.slot ? 2 : 0) | (p.desc_out ? 1 : 0);
	if (!one) {
		CGCK_NOTE_KERNEL("steer_count_kernel");
		hipLaunchKernelGGL(steer_count_kernel, g, b, 0, st, p);
		CGCK_NOTE_KERNEL("steer_scan_kernel");
		hipLaunchKernelGGL(steer_scan_kernel, dim3(1), dim3(kSteerScanThreads), 0, st, p);
		if (!outs)
			return hipGetLastError();
	}
#define CGCK_STEER(K, P, S, D)                                                           \
	do {                                                                             \
		CGCK_NOTE_KERNEL(#K "<%s, %s, %s>", tf(P), tf(S), tf(D));                \
		hipLaunchKernelGGL((K<P, S, D>), g, b, 0, st, p);                        \
	} while (0)
#define CGCK_STEER_OUTS(K)                                                               \
	switch (outs) {                                                                  \
	case 0: CGCK_STEER(K, false, false, false); break;                               \
	case 1: CGCK_STEER(K, false, false, true); break;                                \
	case 2: CGCK_STEER(K, false, true, false); break;                                \
	case 3: CGCK_STEER(K, false, true, true); break;                                 \
	case 4: CGCK_STEER(K, true, false, false); break;                                \
	case 5: CGCK_STEER(K, true, false, true); break;                                 \
	case 6: CGCK_STEER(K, true, true, false); break;                                 \
	default: CGCK_STEER(K, true, true, true); break;                                 \
	}
	if (one)
		CGCK_STEER_OUTS(steer_one_kernel)
	else
		CGCK_STEER_OUTS(steer_scatter_kernel)
#undef CGCK_STEER_OUTS
#undef CGCK_STEER
	return hipGetLastError();
}

} // namespace cgck
