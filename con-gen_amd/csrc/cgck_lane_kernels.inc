// cgck_lane_kernels.inc - the text of lpa_kernel and lpd_kernel, included
// twice by cgck_lane.hip: as lpa_kernel / lpd_kernel (CGCK_LANE_IP6 false,
// IPv4) and as lpa6_kernel / lpd6_kernel (true, CGCK_IP6).  Two kernels from
// one text rather than one body behind two wrappers: the IPv4 kernels then
// compile to the code they had before the IPv6 variants existed (a shared
// inlined body did not).
template <bool NT, int DEPTH>
__global__ __launch_bounds__(256) void CGCK_LPA_KERNEL(KParams p)
{
	constexpr bool IP6 = CGCK_LANE_IP6;
	const int len = (int)p.ip_len, nch = (len + 15) >> 4;
	const uint64_t NI = (p.n + 255) / 256, S = gridDim.x;
	uint64_t it = blockIdx.x;
	if (it >= NI)
		return;
	// DEPTH packet groups per lane in a register ring: the load of group
	// d + DEPTH - 1 is issued before group d is reduced.  Loads are never
	// skipped (past the end they read a zero line), so the loop has no load
	// under a branch and every wait is a counted vmcnt.
	Quad Q[DEPTH];
#pragma unroll
	for (int d = 0; d < DEPTH - 1; ++d)
		lpa_load<NT>(p, (it + d * S) * 256 + threadIdx.x, it + d * S < NI, nch, Q[d]);
	for (;;) {
#pragma unroll
		for (int d = 0; d < DEPTH; ++d) {
			const uint64_t ahead = it + (uint64_t)(d + DEPTH - 1) * S;
			lpa_load<NT>(p, ahead * 256 + threadIdx.x, ahead < NI, nch, Q[(d + DEPTH - 1) % DEPTH]);
			lpa_reduce<NT, false, IP6>(p, (it + d * S) * 256 + threadIdx.x, len, nch, Q[d]);
			if (it + (uint64_t)(d + 1) * S >= NI)
				return;
		}
		it += (uint64_t)DEPTH * S;
	}
}

// --------------------------------------------------------------------------
// Lane per packet fed by LDS-DMA (lpd: the 64 B config's default)
// --------------------------------------------------------------------------
//
// lpa's per-lane loads touch 64 lines per instruction.  Here each step of 64
// packets (63 * stride + len <= 4 KiB) moves as four contiguous 1 KiB
// global_load_lds_dwordx4 instructions into a ring of D LDS slots of its
// wave, and lane L reads packet L's chunks from LDS and reduces them with
// lpa_reduce (the same arithmetic).  Steps come in chunks of C, and chunks
// are grid-interleaved (wave b takes chunks b, b + G, ...), so the grid sweeps
// one window of the batch: the DMA sweep alone then reads 89-99 % of 8 TB/s
// (a contiguous range per wave: 78-89 %).  The output stores were the cost
// left (92 % with the reduce but no stores, 74 % with a u32 store per packet),
// so a chunk's outputs are staged in LDS and leave as one contiguous
// C * 256-byte run of 16-byte stores (sc1 policy).  In one process on one
// buffer (tools/sweep.py, profiles/r02/lpd/): C = 32, D = 2, 8 waves per CU,
// sc1 stores 80.6 % against lpa's 71.8 %; C = 16 75.2 %, nt stores 78.8 %,
// default-policy stores 73.1 %, D = 3 or 10 waves per CU lose (LDS occupancy
// below the grid: a tail of non-resident waves).
//
// Counted vmcnt: per step 4 DMA; a chunk flush adds C / 4 stores, so the wait
// for step j leaves the D - 1 later steps' DMA and, right after a flush, the
// flush's stores in flight.
template <int D, int C, int SP>
__global__ __launch_bounds__(64) void CGCK_LPD_KERNEL(KParams p)
{
	constexpr bool IP6 = CGCK_LANE_IP6;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int lane = threadIdx.x;
	const int len = (int)p.ip_len, nch = (len + 15) >> 4;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	uint32_t *so = reinterpret_cast<uint32_t *>(smem + D * 4096); // C > 1: a chunk's outputs
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t base = reinterpret_cast<uint64_t>(p.base) + p.l3_off;
	const uint64_t last_chunk = (base + (p.n - 1) * p.stride + len - 1) & ~(uint64_t)15;
	// Chunks of C steps of 64 packets, grid-interleaved (wave b takes chunks
	// b, b + G, ...): the grid sweeps one window of the batch, so reads and
	// output writes stay within few DRAM pages chip-wide.  C > 1: a chunk's
	// outputs are staged in LDS and leave as one contiguous C * 256-byte run.
	const uint64_t NS = (p.n + 63) / 64, NC = (NS + C - 1) / C, G = gridDim.x, b = blockIdx.x;
	if (b >= NC)
		return;
	const uint64_t nsteps = (NC - b + G - 1) / G * C;
	auto gstep = [&](uint64_t j) { return (b + (j / C) * G) * C + j % C; };
	// bytes a step covers: lanes past them (stride < 64) read the zero line
	const uint32_t span = (uint32_t)(63 * p.stride) + (uint32_t)len;
	auto issue = [&](uint64_t j) { // step j of this wave into slot j % D
		const uint64_t gs = gstep(j);
		const uint64_t a = base + gs * 64 * p.stride;
		const uint32_t slot = lds0 + (uint32_t)(j % D) * 4096;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const uint32_t at = 1024 * i + 16 * lane;
			const uint64_t src = a + at;
			glds16_nt(j < nsteps && gs < NS && at < span && src <= last_chunk ? reinterpret_cast<const void *>(src)
											  : zero,
				  slot + 1024 * i);
		}
	};
#pragma unroll
	for (int d = 0; d < D - 1; ++d)
		issue(d);
	const int o = lane * (int)p.stride; // packet L's byte offset in a slot
	constexpr bool stage = C > 1; // lpd_ok guarantees an output array
	// SP >= 3 (lab A/B): a full chunk's outputs are read from the staging into
	// registers at the chunk's end and stored right AFTER the next step's DMA
	// issue (as lpw does), so the two following waits leave them in flight
	// (two steps to complete instead of one); store policy SP - 3.
	constexpr bool DEFER = SP >= 3 && C > 1;
	constexpr int policy = SP % 3 == 0 ? kNt : SP % 3 == 1 ? kDefaultPolicy : kSc1;
	u32x4_t held[DEFER ? C / 4 : 1];
	bool pend = false;
	uint64_t pfirst = 0;
	for (uint64_t j = 0; j < nsteps; ++j) {
		issue(j + D - 1);
		if (DEFER && pend) {
			const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + pfirst, C * 256);
#pragma unroll
			for (int i = 0; i < (DEFER ? C / 4 : 0); ++i)
				bstore16<policy>(rs, 16 * (i * 64 + lane), held[i]);
			pend = false;
		}
		// Wait for step j's DMA.  Issued after it: the DMA of the D - 1 later
		// steps, plus the output stores of the steps since (C == 1: one per
		// step once the ring is full; C > 1: C / 4 of the last chunk flush,
		// when that flush came after step j's DMA).
		if (C == 1) {
			if (j + 1 < (uint64_t)D || !p.out)
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4 * (D - 1)) : "memory");
			else
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(5 * (D - 1)) : "memory");
		} else {
			if (stage && j >= (uint64_t)C && (j % C) <= (uint64_t)(DEFER ? D - 1 : D - 2))
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4 * (D - 1) + C / 4) : "memory");
			else
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4 * (D - 1)) : "memory");
		}
		__builtin_amdgcn_s_barrier();
		const uint8_t *sl = smem + (uint32_t)(j % D) * 4096;
		Quad q;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			q.c[i] = *reinterpret_cast<const uint4 *>(sl + o + 16 * (i < nch ? i : nch - 1));
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot is refilled next step
		const uint64_t k = gstep(j) * 64 + lane;
		if (stage)
			lpa_reduce<false, true, IP6>(p, k, len, nch, q, so + (j % C) * 64 + lane);
		else
			lpa_reduce<false, false, IP6>(p, k, len, nch, q);
		if (stage && (j + 1) % C == 0 && p.contig != 2) { // contig 2: lab $CGCK_LPD_SINK, no flush
			// flush the chunk: C / 4 coalesced 16-byte stores per lane
			const uint64_t first = (b + (j / C) * G) * C * 64;
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			if (DEFER && first + C * 64 <= p.n && j + 1 < nsteps) {
				const u32x4_t *s4 = reinterpret_cast<const u32x4_t *>(so);
#pragma unroll
				for (int i = 0; i < (DEFER ? C / 4 : 0); ++i)
					held[i] = s4[i * 64 + lane];
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // read before the next reduce restages
				pend = true;
				pfirst = first;
			} else if (first + C * 64 <= p.n) {
				const uint4 *s4 = reinterpret_cast<const uint4 *>(so);
				const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + first, C * 256);
#pragma unroll
				for (int i = 0; i < C / 4; ++i) {
					const uint4 w = s4[i * 64 + lane];
					bstore16<policy>(rs, 16 * (i * 64 + lane), u32x4_t{w.x, w.y, w.z, w.w});
				}
			} else {
				// the batch's last, partial chunk: per-packet stores, then drain
				for (int i = lane; i < C * 64; i += 64)
					if (first + i < p.n)
						gbl(p.out)[first + i] = so[i];
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			}
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

