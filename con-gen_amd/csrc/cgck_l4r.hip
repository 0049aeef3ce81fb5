// cgck_l4r.hip — tcp_respond's RSTs for a burst (cgck_l4_reply, include/cgck.h
// section 3): cgck_l4_desc's records, cgck_pcb_lookup's kinds and the verify's
// verdicts in, the segment and flow records cgck_l4_build takes out.  The rule is
// cgck_reply_rule.h's, which cgck_l4_reply_rule compiles for the host too; here
// are the kernel around it and its launcher.
//
// l4r_kernel: cgck_frame.h's shape, a lane per frame, FrameCursor<4>: the 48
// frame-relative bytes the four chunks cover hold everything the rule reads (the
// version nibble, b[8..40)) at any alignment, realigned in registers: no byte
// loads, nothing outside the granules that hold a frame byte.  The record (two
// 16-byte halves), the four selector bytes and at[k] are fetched a step ahead
// with the chunks.
//
// Stores.  Without `at` a wave-step's 64 reply records are 2 KiB consecutive and
// its 64 flow records 3 KiB: both leave through wave_turn_store as consecutive
// 16-byte pieces.  With `at` a record lies where at[k] says.  AT 1: a lane stores
// its own two and three pieces.  AT 2: pieces and targets are turned through LDS,
// so consecutive lanes store the consecutive pieces of one record and, where at[]
// runs consecutive (cgck_l4_reply_packed's does within a class), of neighbouring
// records (wave_turn_scatter).  cls leaves as a lane's own byte at at[k], queue at
// k, the counters through the LDS histogram.  Plain vector stores; no lane or
// workgroup waits for another.
//
// LDS.  12 KiB of turned pieces, 1 KiB of targets and 32 bytes of counters per
// workgroup.
#include "cgck_frame.h"
#include "cgck_reply_rule.h"

namespace cgck {

constexpr uint32_t kL4rBins = CGCK_RPL_NCOUNT;
constexpr uint32_t kL4rNoAt = 0xFFFFFFFFu;

// wave_turn_store to scattered records: lane l's record, PER pieces, goes to
// g[PER xa[l] ..), or nowhere when xa[l] is kL4rNoAt.  The lanes put their
// pieces into the wave's LDS block xs (T[64 PER]); store instruction j then takes
// pieces 64 j .. 64 j + 63 of the block in lane order.  xa (u32[64], the wave's) is
// written by the caller before the call.
template <class T, int PER>
__device__ __forceinline__ void wave_turn_scatter(T *xs, const uint32_t *xa, const T (&mine)[PER], CGCK_GLOBAL T *g,
						  int lane)
{
#pragma unroll
	for (int j = 0; j < PER; ++j)
		xs[PER * lane + j] = mine[j];
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const uint32_t i = 64u * j + (uint32_t)lane, src = i / PER, piece = i - PER * src;
		const uint32_t a = xa[src];
		if (a != kL4rNoAt)
			g[(uint64_t)PER * a + piece] = xs[i];
	}
	__builtin_amdgcn_wave_barrier();
	asm volatile("" ::: "memory");
}

// What is fetched a step ahead for frame k beside its chunks.
struct L4rAhead {
	u32x4_t s0, s1; // seg[k]
	uint32_t sel;   // c | kd << 8 | vd << 16 | lc << 24
	uint32_t at;
};

// REC: seg and / or flow are written; X: cls, queue and / or the counters; AT: 0
// no `at`, 1 a lane's own stores, 2 turned (see above).
template <bool REC, bool X, int AT>
__global__ __launch_bounds__(kFrameThreads) void l4r_kernel(L4rParams p)
{
	__shared__ uint32_t hist[kL4rBins];
	__shared__ __attribute__((aligned(16))) u32x4_t xpose[REC && AT != 1 ? kFrameWaves : 1][REC && AT != 1 ? 192 : 1];
	__shared__ uint32_t xat[REC && AT == 2 ? kFrameWaves : 1][64];
	const bool count = X && p.count != nullptr;
	if (X) {
		frame_hist_zero(hist, kL4rBins);
		__syncthreads();
	}
	const FrameDescs src = {p.base, p.desc, p.n};
	FrameCursor<4, FrameDescs> cur(src, p.n, p.zero);
	const CGCK_GLOBAL u32x4_t *segv = (const CGCK_GLOBAL u32x4_t *)p.seg;
	const CGCK_GLOBAL uint8_t *clsb = (const CGCK_GLOBAL uint8_t *)p.cls, *kindb = (const CGCK_GLOBAL uint8_t *)p.kind;
	const CGCK_GLOBAL uint8_t *verb = (const CGCK_GLOBAL uint8_t *)p.verdict, *l2b = (const CGCK_GLOBAL uint8_t *)p.l2cls;
	const CGCK_GLOBAL uint32_t *atw = (const CGCK_GLOBAL uint32_t *)p.at;
	const uint32_t link[4] = {p.link[0], p.link[1], p.link[2], p.link[3]};
	// index clamped as frame_desc's
	auto fetch = [&](uint64_t k) {
		const uint64_t kk = k < p.n ? k : p.n - 1;
		L4rAhead a;
		a.s0 = segv[2 * kk];
		a.s1 = segv[2 * kk + 1];
		a.sel = (clsb ? clsb[kk] & 15u : (uint32_t)CGCK_SEG_TCP) | (kindb ? (uint32_t)kindb[kk] : (uint32_t)CGCK_PCB_MISS) << 8 |
			(verb ? (uint32_t)verb[kk] : 0u) << 16 | (l2b ? (uint32_t)l2b[kk] : 0u) << 24;
		a.at = AT != 0 ? atw[kk] : 0u;
		return a;
	};
	if (cur.more()) {
		cur.start();
		L4rAhead in = fetch(cur.k()), nx;
		for (; cur.more(); cur.advance(), in = nx) {
			cur.ahead();
			nx = fetch((cur.s + cur.W) * 64 + cur.lane);
			const uint64_t k = cur.k();
			const bool ok = k < p.n;
			uint32_t B[12]; // the frame's bytes [0, 48)
			frame_realign(cur.c.c, (uint32_t)(cur.a0 & 15), B);
			const uint32_t S[8] = {in.s0[0], in.s0[1], in.s0[2], in.s0[3], in.s1[0], in.s1[1], in.s1[2], in.s1[3]};
			uint32_t r[8], f[12];
			const uint32_t cb = reply_rule(S, in.sel & 255u, (in.sel >> 8) & 255u, (in.sel >> 16) & 255u, p.vmask, in.sel >> 24,
						       p.flags, B, cur.len, link, r, f);
			const uint32_t cl = cb & 15u;
			// where the frame's seg, flow and cls go; none past the arrays
			const uint64_t a = AT != 0 ? in.at : k;
			const bool put = ok && a < p.n;
			if (REC) {
				const u32x4_t rs[2] = {{r[0], r[1], r[2], r[3]}, {r[4], r[5], r[6], r[7]}};
				const u32x4_t fl[3] = {{f[0], f[1], f[2], f[3]}, {f[4], f[5], f[6], f[7]}, {f[8], f[9], f[10], f[11]}};
				CGCK_GLOBAL u32x4_t *so = (CGCK_GLOBAL u32x4_t *)p.seg_out, *fo = (CGCK_GLOBAL u32x4_t *)p.flow_out;
				if (AT == 0) {
					const uint64_t left = p.n - cur.s * 64;
					u32x4_t *xs = xpose[threadIdx.x >> 6];
					if (so)
						wave_turn_store(xs, rs, so + 128 * cur.s, left, cur.lane);
					if (fo)
						wave_turn_store(xs, fl, fo + 192 * cur.s, left, cur.lane);
				} else if (AT == 1) {
					if (put && so) {
						so[2 * a] = rs[0];
						so[2 * a + 1] = rs[1];
					}
					if (put && fo) {
						fo[3 * a] = fl[0];
						fo[3 * a + 1] = fl[1];
						fo[3 * a + 2] = fl[2];
					}
				} else {
					u32x4_t *xs = xpose[threadIdx.x >> 6];
					uint32_t *xa = xat[threadIdx.x >> 6];
					xa[cur.lane] = put ? (uint32_t)a : kL4rNoAt;
					if (so)
						wave_turn_scatter(xs, xa, rs, so, cur.lane);
					if (fo)
						wave_turn_scatter(xs, xa, fl, fo, cur.lane);
				}
			}
			if (X && ok) {
				if (p.cls_out && put)
					((CGCK_GLOBAL uint8_t *)p.cls_out)[a] = (uint8_t)cb;
				if (p.queue)
					((CGCK_GLOBAL uint8_t *)p.queue)[k] = cl == CGCK_RPL_RST ? 0 : 0xFF;
				if (count) {
					__hip_atomic_fetch_add(hist + cl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					if (cb == ((uint32_t)CGCK_RPL_RST | (uint32_t)CGCK_RPL_IP6))
						__hip_atomic_fetch_add(hist + 7, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
		}
	}
	if (X)
		frame_hist_flush(hist, kL4rBins, p.count);
}

hipError_t launch_l4r(const L4rParams &p, bool turned, int num_cus, hipStream_t st)
{
	if (p.n == 0)
		return hipSuccess;
	const dim3 g(frame_grid(p.n, num_cus)), b(kFrameThreads);
	const bool rec = p.seg_out != nullptr || p.flow_out != nullptr;
	const bool x = p.cls_out != nullptr || p.queue != nullptr || p.count != nullptr;
	// the turned targets are 32-bit with one value set aside: a longer burst stores from its own lanes
	const int at = p.at == nullptr ? 0 : rec && turned && p.n <= 0xFFFFFFFFull ? 2 : 1;
#define CGCK_L4R(Rr, Xx, Aa)                                                          \
	do {                                                                          \
		CGCK_NOTE_KERNEL("l4r_kernel<%s, %s, %d>", tf(Rr), tf(Xx), Aa);       \
		hipLaunchKernelGGL((l4r_kernel<Rr, Xx, Aa>), g, b, 0, st, p);         \
	} while (0)
#define CGCK_L4R_AT(Rr, Xx)                \
	do {                               \
		if (at == 0)               \
			CGCK_L4R(Rr, Xx, 0); \
		else if (at == 1)          \
			CGCK_L4R(Rr, Xx, 1); \
		else                       \
			CGCK_L4R(Rr, Xx, 2); \
	} while (0)
	if (rec && x)
		CGCK_L4R_AT(true, true);
	else if (rec)
		CGCK_L4R_AT(true, false);
	else if (at == 0)
		CGCK_L4R(false, true, 0);
	else
		CGCK_L4R(false, true, 1);
#undef CGCK_L4R_AT
#undef CGCK_L4R
	return hipGetLastError();
}

} // namespace cgck
