// cgck_lane_lab.inc - cgck_lane.hip's lab-only half (libcgck_lab.so): kernels
// that lost their A/B, their launchers, the lab halves of launch_lpd / lpw / lpp.
// Included once under CGCK_LAB, in namespace cgck: text, not a source, as it is
// built from product device helpers and instantiates product kernel templates.

// Software-pipelined lane-per-packet: while iteration i is computed, the
// chunks of iteration i+1 are already in flight (and, for descriptor
// batches, the descriptors of iteration i+2), so a wave never waits for
// memory between iterations.  Small packets only (nch <= S0 + the last
// chunk; longer packets take the same streaming loop as lpp_kernel).
template <bool DESC, bool NT>
__global__ __launch_bounds__(256) void lppp_kernel(KParams p)
{
	constexpr int S0 = 6;
	const bool raw = p.flags & CGCK_RAW;
	const Sched sc = sched((p.n + 255) / 256, p.contig);
	uint64_t it = sc.it;
	if (it >= sc.end)
		return;
	// prologue: descriptors of it and it+step, chunks of it
	Pkt pk = get_pkt<DESC>(p, it * 256 + threadIdx.x);
	Pkt pk2 = get_pkt<DESC>(p, (it + sc.step) * 256 + threadIdx.x);
	uint4 v[S0], last;
	{
		const int nch = nchunks(pk.a0, pk.len);
		const uint4 *c0 = reinterpret_cast<const uint4 *>(pk.a0 & ~(uint64_t)15);
#pragma unroll
		for (int i = 0; i < S0; ++i)
			v[i] = ldc<NT>(c0, i, nch, p.zero);
		last = ldc<NT>(c0, nch - 1, nch, p.zero);
	}
	for (; it < sc.end; it += sc.step) {
		const uint64_t k = it * 256 + threadIdx.x;
		// issue the next iteration's chunks (its descriptor is pk2)
		const Pkt pkn = pk2;
		uint4 vn[S0], lastn;
		{
			const int nch = nchunks(pkn.a0, pkn.len);
			const uint4 *c0 = reinterpret_cast<const uint4 *>(pkn.a0 & ~(uint64_t)15);
#pragma unroll
			for (int i = 0; i < S0; ++i)
				vn[i] = ldc<NT>(c0, i, nch, p.zero);
			lastn = ldc<NT>(c0, nch - 1, nch, p.zero);
		}
		pk2 = get_pkt<DESC>(p, (it + 2 * sc.step) * 256 + threadIdx.x);

		const uint64_t a0 = pk.a0;
		const int len = (int)pk.len, q = (int)(a0 & 15), nch = nchunks(a0, pk.len);
		const uint4 *c0 = reinterpret_cast<const uint4 *>(a0 & ~(uint64_t)15);
		uint32_t tot = 0;
#pragma unroll
		for (int i = 0; i < S0; ++i)
			tot = i < nch ? sum4(v[i], tot) : tot;
		Hdr h{};
		if (!raw)
			h = header<S0, NT>(v, c0, nch, q, len, p.flags, pk.ok);
		for (int t = S0; __any(t < nch - 1); t += 8) {
			uint4 w[8];
#pragma unroll
			for (int i = 0; i < 8; ++i)
				w[i] = t + i < nch - 1 ? ld<NT>(c0 + t + i) : make_uint4(0, 0, 0, 0);
			uint32_t s = 0;
#pragma unroll
			for (int i = 0; i < 8; ++i)
				s = sum4(w[i], s);
			tot = fold16(tot) + fold16(s);
		}
		const bool dw = !__any(((q | len) & 3) != 0);
		if (__any(q != 0))
			tot = fold16(tot) + (0xffffu - fold16(lead_sum(v[0], q, dw)));
		const int e = q + len - 16 * (nch - 1);
		if (__any(nch > S0))
			tot = fold16(tot) + fold16(nch > S0 ? sum4(last, 0) - trail_sum(last, e, dw) : 0u);
		if (__any(nch > 0 && nch <= S0 && e != 16)) {
			uint4 lc = make_uint4(0, 0, 0, 0);
#pragma unroll
			for (int i = 0; i < S0; ++i)
				if (i == nch - 1)
					lc = v[i];
			tot = fold16(tot) + (0xffffu - fold16(nch > 0 && nch <= S0 ? trail_sum(lc, e, dw) : 0u));
		}
		if (pk.ok)
			finish(p, k, a0, len, fold16(tot), h);
		pk = pkn;
#pragma unroll
		for (int i = 0; i < S0; ++i)
			v[i] = vn[i];
		last = lastn;
	}
}

// Loader/consumer form (A/B; lost: 62-72 %): the output store sits in the
// consumers' vmcnt only.
// Wave 0 of a 256-thread workgroup only moves bytes (a phase = 3 steps of 64
// packets, 12 KiB, into a ring of P phases); waves 1..3 each reduce one step
// per phase from LDS and store its outputs.  Per phase: the loader waits
// (counted vmcnt) for phase ph, all four waves pass barrier ph, the loader
// refills the slots of phase ph - 1 (which the consumers finished,
// lgkmcnt(0), before that barrier) with phase ph + P - 1.
template <int P>
__global__ __launch_bounds__(256) void lpd_lc_kernel(KParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	const int len = (int)p.ip_len, nch = (len + 15) >> 4;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t base = reinterpret_cast<uint64_t>(p.base) + p.l3_off;
	const uint64_t last_chunk = (base + (p.n - 1) * p.stride + len - 1) & ~(uint64_t)15;
	// phases of 192 packets, grid-interleaved (workgroup b takes phases b,
	// b + G, ...), as in the per-wave form
	const uint64_t NP = (p.n + 191) / 192, G = gridDim.x, b = blockIdx.x;
	if (b >= NP)
		return; // uniform across the workgroup
	const uint64_t nph = (NP - b + G - 1) / G;
	if (wave == 0) {
		auto issue = [&](uint64_t ph) {
			const uint32_t grp = lds0 + (uint32_t)(ph % P) * 3 * 4096;
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const uint64_t first = (b + ph * G) * 192 + 64 * c;
				const uint64_t a = base + first * p.stride;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const uint64_t src = a + 1024 * i + 16 * lane;
					glds16_nt(ph < nph && first < p.n && src <= last_chunk ? reinterpret_cast<const void *>(src) : zero,
						  grp + c * 4096 + 1024 * i);
				}
			}
		};
#pragma unroll
		for (int d = 0; d < P - 1; ++d)
			issue(d);
		for (uint64_t ph = 0; ph < nph; ++ph) {
			// phase ph landed: phases ph + 1 .. ph + P - 2 may stay in flight
			asm volatile("s_waitcnt vmcnt(%0)" ::"i"((P - 2) * 12) : "memory");
			__builtin_amdgcn_s_barrier();
			issue(ph + P - 1);
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	} else {
		const int c = wave - 1;
		const int o = lane * (int)p.stride;
		for (uint64_t ph = 0; ph < nph; ++ph) {
			__builtin_amdgcn_s_barrier();
			const uint64_t first = (b + ph * G) * 192 + 64 * c;
			if (first < p.n) {
				const uint8_t *sl = smem + ((uint32_t)(ph % P) * 3 + c) * 4096;
				Quad q;
#pragma unroll
				for (int i = 0; i < 4; ++i)
					q.c[i] = *reinterpret_cast<const uint4 *>(sl + o + 16 * (i < nch ? i : nch - 1));
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
				lpa_reduce<false>(p, first + lane, len, nch, q);
			}
			// this phase's slots are refilled after the next barrier
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		}
	}
}

// lpd with a writer wave (A/B): wave 0 of a 128-thread workgroup is
// lpd_kernel's DMA ring and reduce without any global store; at the end of a
// chunk it hands the staged outputs to wave 1 across a barrier, and wave 1
// reads them into registers (before the next step's barrier, so wave 0 may
// refill the staging) and stores them as 16-byte sc1 runs.  The stores then
// count only in the writer's vmcnt, not in front of wave 0's DMA waits.
template <int D, int C>
__global__ __launch_bounds__(128) void lpdw_kernel(KParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int len = (int)p.ip_len, nch = (len + 15) >> 4;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	uint32_t *so = reinterpret_cast<uint32_t *>(smem + D * 4096); // a chunk's outputs
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t base = reinterpret_cast<uint64_t>(p.base) + p.l3_off;
	const uint64_t last_chunk = (base + (p.n - 1) * p.stride + len - 1) & ~(uint64_t)15;
	const uint64_t NS = (p.n + 63) / 64, NC = (NS + C - 1) / C, G = gridDim.x, b = blockIdx.x;
	if (b >= NC)
		return;
	const uint64_t nsteps = (NC - b + G - 1) / G * C;
	if (wave == 1) {
		for (uint64_t j = 0; j < nsteps; ++j) {
			wg_barrier();
			if ((j + 1) % C != 0)
				continue;
			wg_barrier(); // chunk j / C staged
			const uint64_t first = (b + (j / C) * G) * C * 64;
			if (first + C * 64 <= p.n) {
				u32x4_t v[C / 4];
				const uint4 *s4 = reinterpret_cast<const uint4 *>(so);
#pragma unroll
				for (int i = 0; i < C / 4; ++i) {
					const uint4 w = s4[i * 64 + lane];
					v[i] = u32x4_t{w.x, w.y, w.z, w.w};
				}
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // staging free before the next barrier
				const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + first, C * 256);
#pragma unroll
				for (int i = 0; i < C / 4; ++i)
					bstore16<kSc1>(rs, 16 * (i * 64 + lane), v[i]);
			} else {
				for (int i = lane; i < C * 64; i += 64)
					if (first + i < p.n)
						gbl(p.out)[first + i] = so[i];
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			}
		}
		return;
	}
	auto gstep = [&](uint64_t j) { return (b + (j / C) * G) * C + j % C; };
	const uint32_t span = (uint32_t)(63 * p.stride) + (uint32_t)len;
	auto issue = [&](uint64_t j) {
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
	const int o = lane * (int)p.stride;
	for (uint64_t j = 0; j < nsteps; ++j) {
		issue(j + D - 1);
		asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4 * (D - 1)) : "memory");
		wg_barrier();
		const uint8_t *sl = smem + (uint32_t)(j % D) * 4096;
		Quad q;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			q.c[i] = *reinterpret_cast<const uint4 *>(sl + o + 16 * (i < nch ? i : nch - 1));
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot is refilled next step
		const uint64_t k = gstep(j) * 64 + lane;
		lpa_reduce<false, true>(p, k, len, nch, q, so + (j % C) * 64 + lane);
		if ((j + 1) % C == 0) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the chunk's outputs are in LDS
			wg_barrier();                      // hand them to the writer
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// --------------------------------------------------------------------------
// Lane per 128-byte slot, one iteration in flight (slot: slot2 replaced it)
// --------------------------------------------------------------------------

// inclusive prefix sum over the wave (values small enough for u32)
__device__ __forceinline__ uint32_t wave_scan(uint32_t x)
{
	const int l = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t y = __shfl_up(x, d, 64);
		if (l >= d)
			x += y;
	}
	return x;
}

// One window of up to 64 slots of ONE packet (jumbo packets, > 64 slots):
// returns the window's contribution (folded) on every lane.
template <bool NT>
__device__ __forceinline__ uint32_t jumbo_window(const uint4 *c0, int nch, int s, uint4 (&w)[8])
{
#pragma unroll
	for (int i = 0; i < 8; ++i)
		w[i] = 8 * s + i < nch ? ld<NT>(c0 + 8 * s + i) : make_uint4(0, 0, 0, 0);
	uint32_t r = 0;
#pragma unroll
	for (int i = 0; i < 8; ++i)
		r = sum4(w[i], r);
	return r;
}

template <bool DESC, bool NT>
__global__ __launch_bounds__(256) void slot_kernel(KParams p)
{
	__shared__ uint32_t mark[4][64];
	__shared__ uint32_t so[4][kWaveStage];
	__shared__ uint8_t sv[4][kWaveStage];
	const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63; // wave-uniform (SGPR)
	const bool raw = p.flags & CGCK_RAW;
	const uint64_t nwaves = (uint64_t)gridDim.x * 4;
	const uint64_t wid = (uint64_t)blockIdx.x * 4 + wv;
	const uint64_t per = (p.n + nwaves - 1) / nwaves;
	const uint64_t r0 = wid * per;
	const uint64_t r1 = r0 + per < p.n ? r0 + per : p.n;
	WaveStage ws{so[wv], sv[wv], r0};

	for (uint64_t cur = r0; cur < r1;) {
		// -- this iteration's packets and their slots --
		const uint64_t kk = cur + l;
		const Pkt pk = get_pkt<DESC>(p, kk < r1 ? kk : p.n); // past the range: !ok
		const int nch_l = nchunks(pk.a0, pk.len);
		const uint32_t ns = pk.ok ? (uint32_t)max(1, (nch_l + 7) >> 3) : 0u;
		const uint32_t P = wave_scan(ns);
		const uint64_t fit = __ballot(pk.ok && P <= 64);
		const int m = __popcll(fit);

		if (m == 0) {
			// Jumbo packet (> 64 slots): windows of 64 slots, whole-wave sums.
			const uint64_t a0 = shfl64(pk.a0, 0);
			const int len = __shfl((int)pk.len, 0, 64), nch = __shfl(nch_l, 0, 64);
			const int q = (int)(a0 & 15);
			const uint4 *c0 = reinterpret_cast<const uint4 *>(a0 & ~(uint64_t)15);
			const int nsj = (nch + 7) >> 3;
			uint32_t acc = 0;
			Hdr h{};
			for (int wbase = 0; wbase < nsj; wbase += 64) {
				const int s = wbase + l;
				uint4 w[8];
				uint32_t r = jumbo_window<NT>(c0, nch, s, w);
				if (wbase == 0 && !raw)
					h = header<8, NT>(w, c0, nch, q, len, p.flags, l == 0);
				const int j = (nch - 1) - 8 * s; // last chunk's position in this slot
				const int e = q + len - 16 * (nch - 1);
				uint32_t corr = 0;
				if (s == 0 && q != 0)
					corr += lead_sum(w[0], q, false);
				if (j >= 0 && j < 8 && e != 16)
					corr += trail_sum(pick8(w, j), e, false);
				r = fold16(r) + (0xffffu - fold16(corr));
				acc = fold16(acc) + fold16(gsum<64>(r));
			}
			wave_stage_reserve(p, ws, cur, 1);
			if (l == 0)
				wave_stage_put(ws, cur, result(p, a0, len, fold16(acc), h));
			cur += 1;
			continue;
		}

		// -- lane -> (owner packet, slot) through per-wave head markers --
		const int T = __shfl((int)P, m - 1, 64); // slots in use
		const int st = (int)(P - ns);            // first slot of lane l's packet
		mark[wv][l] = 0;
		__builtin_amdgcn_wave_barrier();
		asm volatile("" ::: "memory");
		if (l < m)
			mark[wv][st] = 1;
		__builtin_amdgcn_wave_barrier();
		asm volatile("" ::: "memory");
		const uint32_t hf = mark[wv][l];
		const uint64_t heads = __ballot(hf != 0 && l < T);
		const uint64_t le = l == 63 ? ~0ull : ((2ull << l) - 1);
		const int owner = max(0, __popcll(heads & le) - 1);
		const bool act = l < T;

		const uint64_t a0 = shfl64(pk.a0, owner);
		const int len = __shfl((int)pk.len, owner, 64);
		const int nch = __shfl(nch_l, owner, 64);
		const int st_o = __shfl(st, owner, 64);
		const int ns_o = __shfl((int)ns, owner, 64);
		const int s = l - st_o; // slot index inside the packet
		const int q = (int)(a0 & 15);
		const uint4 *c0 = reinterpret_cast<const uint4 *>(a0 & ~(uint64_t)15);

		// clamped, branch-free: slot tails and idle lanes re-read the
		// packet's last chunk (or the zero chunk) and are dropped below
		uint4 w[8];
#pragma unroll
		for (int i = 0; i < 8; ++i)
			w[i] = ldc<NT>(c0, 8 * s + i, nch, p.zero);
		uint32_t r = 0;
#pragma unroll
		for (int i = 0; i < 8; ++i)
			r = act && 8 * s + i < nch ? sum4(w[i], r) : r;

		const bool head = act && s == 0;
		Hdr h{};
		if (!raw)
			h = header<8, NT>(w, c0, nch, q, len, p.flags, head);

		// edges: lead on the head lane, trail on the lane holding chunk nch-1
		const bool dw = !__any(act && ((q | len) & 3) != 0);
		uint32_t corr = 0;
		if (__any(head && q != 0))
			corr = head && q != 0 ? lead_sum(w[0], q, dw) : 0u;
		const int j = (nch - 1) - 8 * s;
		const int e = q + len - 16 * (nch - 1);
		const bool tail = act && nch > 0 && j >= 0 && j < 8 && e != 16;
		if (__any(tail))
			corr += tail ? trail_sum(pick8(w, j), e, dw) : 0u;
		r = fold16(r) + (0xffffu - fold16(corr));

		// segmented suffix sum towards the head lane
		uint32_t nso = 0; // wave-uniform bound on segment length (OR >= max)
#pragma unroll
		for (int b = 0; b < 7; ++b)
			nso |= __any(act && ((ns_o >> b) & 1)) ? (1u << b) : 0u;
		const int send = st_o + ns_o;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			if ((uint32_t)d >= nso)
				break;
			const uint32_t y = __shfl_down(r, d, 64);
			if (l + d < send)
				r += y;
		}
		wave_stage_reserve(p, ws, cur, m);
		if (head)
			wave_stage_put(ws, cur + owner, result(p, a0, len, fold16(r), h));
		cur += m;
	}
	if (r0 < r1)
		wave_stage_flush(p, ws, r1);
}

// --------------------------------------------------------------------------
// Lane per 128-byte slot fed by LDS-DMA (slotd: IMIX, A/B against slot2)
// --------------------------------------------------------------------------
//
// slot2's register loads sit at the register-load read ceiling (the probe on
// the same buffer: 71.6-73.1 %), while grid-interleaved LDS-DMA reads run near
// the HBM peak (lpd_kernel).  Same slot map as slot2 (smap); each step's slots
// are moved by 8 DMA instructions into an 8 KiB LDS slot of a 2-deep ring:
// instruction i, lane l moves chunk (l & 7) of slot 8 i + (l >> 3), so an
// instruction reads up to 1 KiB contiguous of one packet and slot s lands at
// +128 s.  Lane s then reads its 8 chunks back from LDS and reduces them with
// slot_reduce.  One wave per workgroup; chunks of kSlotdChunk descriptors are
// grid-interleaved.  Descriptor loads are the compiler's (its vmcnt waits for
// them also cover the DMA issued before, which only makes them stricter); the
// wait for a step's DMA is explicit: only the next step's 8 DMA stay in flight.
constexpr int kSlotdChunk = 2048;

template <bool NT>
__device__ __forceinline__ void slotd_issue(const KParams &p, const SMap &M, bool live, uint32_t lds_slot,
					    const uint8_t *zero)
{
	const int l = threadIdx.x & 63;
	// per slot (lane sigma of M): its first chunk and the chunks it holds
	const uint64_t cb = (M.a0 & ~(uint64_t)15) + 128 * (uint64_t)M.s;
	int rem = M.nch - 8 * M.s;
	rem = !live || !M.act || M.m == 0 ? 0 : rem < 0 ? 0 : rem > 8 ? 8 : rem;
	const uint32_t cb_lo = (uint32_t)cb, cb_hi = (uint32_t)(cb >> 32);
	const int c = l & 7;
#pragma unroll
	for (int i = 0; i < 8; ++i) {
		const int sg = 8 * i + (l >> 3);
		const uint32_t lo = __shfl(cb_lo, sg, 64), hi = __shfl(cb_hi, sg, 64);
		const int r = __shfl(rem, sg, 64);
		const uint64_t src = ((uint64_t)hi << 32 | lo) + 16 * (uint64_t)(c < r ? c : r - 1);
		glds16_nt(r > 0 ? reinterpret_cast<const void *>(src) : zero, lds_slot + 1024 * i);
	}
}

template <bool DESC>
__global__ __launch_bounds__(64) void slotd_kernel(KParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	uint32_t *mark = reinterpret_cast<uint32_t *>(smem + 2 * 8192);
	uint32_t *so = mark + 64;
	uint8_t *sv = reinterpret_cast<uint8_t *>(so + kWaveStage);
	const int l = threadIdx.x & 63;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	for (uint64_t ck = blockIdx.x; ck * kSlotdChunk < p.n; ck += gridDim.x) {
		const uint64_t r0 = ck * kSlotdChunk;
		const uint64_t r1 = r0 + kSlotdChunk < p.n ? r0 + kSlotdChunk : p.n;
		WaveStage ws{so, sv, r0};
		uint64_t cur = r0;
		SMap M = smap<DESC>(p, cur, r1, load_desc<DESC>(p, cur + l, r1), *reinterpret_cast<uint32_t(*)[64]>(mark));
		slotd_issue<false>(p, M, true, lds0, zero);
		uint64_t curN = cur + (M.m ? M.m : 1);
		DescW dN = load_desc<DESC>(p, curN + l, r1);
		for (uint32_t j = 0;; ++j) {
			const SMap MN = smap<DESC>(p, curN, r1, dN, *reinterpret_cast<uint32_t(*)[64]>(mark));
			const uint64_t curNN = curN + (MN.m ? MN.m : 1);
			const DescW dNN = load_desc<DESC>(p, curNN + l, r1);
			slotd_issue<false>(p, MN, curN < r1, lds0 + ((j + 1) & 1) * 8192, zero);
			// step j's DMA (and everything before it) has landed: only the
			// next step's 8 DMA may stay in flight
			asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
			__builtin_amdgcn_s_barrier();
			const uint4 *sl = reinterpret_cast<const uint4 *>(smem + (j & 1) * 8192) + 8 * l;
			uint4 w[8];
#pragma unroll
			for (int i = 0; i < 8; ++i)
				w[i] = sl[i];
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot is refilled next step
			slot_reduce<false>(p, cur, M, w, ws);
			if (curN >= r1)
				break;
			cur = curN;
			M = MN;
			curN = curNN;
			dN = dNN;
		}
		wave_stage_flush(p, ws, r1);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the last (zero) DMA landed before the ring is reused
	}
}

// lpx: lpw with TWO rounds in flight.  lpw waits for round r - 1 right after
// issuing round r, so one 8 KiB window per wave is in flight while a window is
// reduced (its DMA rounds alone: 76.8 % of 8 TB/s).  Here a round's slot is
// refilled as soon as the window's bytes are in registers (dstr's trick): the
// wave waits for round r, reads the window (chunk sums, edge chunks, header
// chunks), issues round r + 2 into the same slot, and only then scans; the
// prefix goes to a separate 2 KiB area.  Every step has at least one round (a
// zero round for a step computed from global memory or past the batch), so
// the issue cursor runs exactly two rounds ahead through cur / nxt / nn; round
// (k, 0) carries the descriptors of step k + 2, which processing (k, 0) turns
// into nn before the round after it can need them.  22.3 KiB of LDS: 7 waves
// per CU, 112 KiB in flight per CU against lpw's 64.
template <bool DESC, int C>
__global__ __launch_bounds__(64) void lpx_kernel(KParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	// 2 x 1 KiB descriptor slots and a third the rounds without descriptors
	// write their zero line into (round (k, 0)'s descriptors of step k + 2 wait
	// in their slot while later rounds of step k are issued)
	uint8_t *dring = smem + 2 * kLpwSlot;
	uint32_t *pfx = reinterpret_cast<uint32_t *>(dring + 3 * 1024); // kLpwWin prefix sums
	uint32_t *so = pfx + kLpwWin;
	uint8_t *sv = reinterpret_cast<uint8_t *>(so + C * 64);
	const int l = threadIdx.x & 63;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	const uint32_t ldsd = lds0 + 2 * kLpwSlot;
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t NS = (p.n + 63) / 64, NC = (NS + C - 1) / C, G = gridDim.x, b = blockIdx.x;
	if (b >= NC)
		return;
	const uint64_t nsteps = (NC - b + G - 1) / G * C;
	auto gstep = [&](uint64_t j) { return (b + (j / C) * G) * C + j % C; };
	auto first_of = [&](uint64_t j) { return j < nsteps ? gstep(j) * 64 : p.n; };

	LpwStep cur = lpw_step<DESC>(p, first_of(0), load_desc<DESC>(p, first_of(0) + l, p.n));
	LpwStep nxt = lpw_step<DESC>(p, first_of(1), load_desc<DESC>(p, first_of(1) + l, p.n));
	LpwStep nn = nxt; // step j + 2: from the descriptors round (j, 0) carries, at processing (j, 0)
	uint32_t kiss = 0; // rounds issued (round k uses data slot k & 1)
	int ia = 0;        // issue cursor: step j + ia ...
	uint32_t iw = 0;   // ... window iw
	auto rounds = [](uint32_t nwin) { return nwin ? nwin : 1u; };
	// issue the round at the cursor (one call site per step struct: a selected
	// struct or field would put the structs in scratch), then advance it
#define CGCK_LPX_ISSUE(ST, K)                                                                            \
	do {                                                                                             \
		const uint64_t k_ = (K);                                                                \
		lpw_issue<DESC>(p, ST.S + (uint64_t)iw * kLpwWin, ST.E, ST.nwin > 0 && first_of(k_) < p.n, ST.gather, \
				ST.cs, ST.ce, ST.dl, smem + (kiss & 1) * kLpwSlot, lds0 + (kiss & 1) * kLpwSlot,      \
				first_of(k_ + 2), iw == 0 && first_of(k_ + 2) < p.n,                           \
				ldsd + (iw == 0 ? (uint32_t)((k_ + 2) & 1) : 2u) * 1024, zero);               \
		++kiss;                                                                                 \
		if (iw + 1 < rounds(ST.nwin)) {                                                          \
			++iw;                                                                           \
		} else {                                                                                \
			++ia;                                                                           \
			iw = 0;                                                                         \
		}                                                                                       \
	} while (0)
	auto issue_next = [&](uint64_t j) __attribute__((always_inline)) {
		if (ia == 0)
			CGCK_LPX_ISSUE(cur, j);
		else if (ia == 1)
			CGCK_LPX_ISSUE(nxt, j + 1);
		else
			CGCK_LPX_ISSUE(nn, j + 2);
	};
	issue_next(0);
	issue_next(0);
	static_assert(C % 4 == 0, "C / 4 16-byte stores per lane per chunk");
	const bool defer_ok = p.out && !p.verdict && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
	bool pend = false; // a chunk's outputs wait in the staging for the next round
	int sage = 0;      // waits left that may leave the chunk store in flight
	uint64_t pf0 = 0;
	for (uint64_t j = 0; j < nsteps; ++j) {
		const uint64_t first = first_of(j);
		const bool live = first < p.n && cur.nwin > 0;
		uint32_t acc = 0, corr = 0;
		Hdr h{};
		u32x4_t t8[8];
#pragma unroll
		for (int u = 0; u < 8; ++u)
			t8[u] = u32x4_t{0, 0, 0, 0};
		const uint32_t R = rounds(cur.nwin);
		for (uint32_t t = 0; t < R; ++t) {
			// round (j, t); issued after it: the next round, and a chunk store
			// (after this round: two waits leave it in flight)
			if (sage > 0) {
				--sage;
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1 + C / 4) : "memory");
			} else {
				asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1) : "memory");
			}
			if (t == 0)
				nn = lpw_step<DESC>(p, first_of(j + 2), lpw_desc_lds<DESC>(dring + ((j + 2) & 1) * 1024));
			const uint4 *win = reinterpret_cast<const uint4 *>(smem + (kiss & 1) * kLpwSlot); // round kiss - 2
			const uint64_t wb = cur.S + (uint64_t)t * kLpwWin;
			const uint64_t we = wb + kLpwWin;
			uint32_t cs8[kLpwDma];
			if (live) {
				const bool head = cur.ok && cur.nch > 0 && cur.cs >= wb && cur.cs < we;
				const bool tail = cur.ok && cur.nch > 0 && cur.ce - 1 >= wb && cur.ce - 1 < we;
				const bool dw = !__any(cur.ok && ((cur.q | cur.len) & 3) != 0);
				if (__any(head && cur.q != 0))
					corr += head && cur.q != 0 ? lead_sum(win[(int)(cur.cs - wb)], cur.q, dw) : 0u;
				if (__any(tail && cur.e != 16))
					corr += tail && cur.e != 16 ? trail_sum(win[(int)(cur.ce - 1 - wb)], cur.e, dw) : 0u;
				const bool hwin = cur.ok && cur.cs + 8 > wb && cur.cs < we;
				if (!(p.flags & CGCK_RAW) && __any(hwin)) {
					const u32x4_t *win4 = reinterpret_cast<const u32x4_t *>(win);
#pragma unroll
					for (int u = 0; u < 8; ++u) {
						const uint64_t c = cur.cs + u;
						const bool in = hwin && c >= wb && c < we;
						const u32x4_t c8 = win4[in ? (int)(c - wb) : 0];
						t8[u] = in ? c8 : t8[u];
					}
				}
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					const uint4 v = win[64 * r + l];
					cs8[r] = wb + 64 * r + l < cur.E ? sum4(v, 0u) : 0u;
				}
			}
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the window is in registers: refill its slot
			issue_next(j);
			if (pend) {
				const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + pf0, C * 256);
#pragma unroll
				for (int i = 0; i < C / 4; ++i)
					bstore16<kSc1>(rs, 16 * (64 * i + l), reinterpret_cast<const u32x4_t *>(so)[64 * i + l]);
				pend = false;
				sage = 2;
			}
			if (live) {
				uint32_t carry = 0;
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					const uint32_t xs = wave_scan_dpp(cs8[r]);
					pfx[64 * r + l] = xs + carry;
					carry += __builtin_amdgcn_readlane(xs, 63);
				}
				const uint64_t lo = cur.cs > wb ? cur.cs : wb;
				const uint64_t hi = cur.ce < we ? cur.ce : we;
				if (cur.ok && hi > lo)
					acc += pfx[(int)(hi - 1 - wb)] - (lo > wb ? pfx[(int)(lo - 1 - wb)] : 0u);
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the prefix area is rewritten next round
			}
		}
		if (live) {
			if (!(p.flags & CGCK_RAW)) {
				uint4 w8[8];
#pragma unroll
				for (int u = 0; u < 8; ++u)
					w8[u] = make_uint4(t8[u].x, t8[u].y, t8[u].z, t8[u].w);
				h = header<8, false>(w8, reinterpret_cast<const uint4 *>(cur.a0 & ~(uint64_t)15), cur.nch, cur.q,
						     cur.len, p.flags, cur.ok);
			}
		} else if (first < p.n) {
			// no window covers the step (more than 16 windows): the lane's packet
			// straight from global memory, after a drain (the two rounds in
			// flight complete first; the counts after it only over-wait)
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			sage = 0;
			const uint4 *c0 = reinterpret_cast<const uint4 *>(cur.a0 & ~(uint64_t)15);
			const int cnt = cur.ok ? cur.nch : 0;
			for (int i = 0; __any(i < cnt); ++i) {
				const uint4 v = ldc<false>(c0, i, cnt, p.zero);
				acc = i < cnt ? sum4(v, acc) : acc;
				if (i == 0 && cnt > 0 && cur.q != 0)
					corr += lead_sum(v, cur.q, false);
				if (i == cnt - 1 && cur.e != 16)
					corr += trail_sum(v, cur.e, false);
			}
			if (!(p.flags & CGCK_RAW)) {
				uint4 w8[8];
#pragma unroll
				for (int u = 0; u < 8; ++u)
					w8[u] = ldc<false>(c0, u, cnt, p.zero);
				h = header<8, false>(w8, c0, cur.nch, cur.q, cur.len, p.flags, cur.ok);
			}
		}
		if (first < p.n) {
			const uint32_t r = fold16(acc) + (0xffffu - fold16(corr));
			const Res res = result(p, cur.a0, cur.len, fold16(r), h);
			const int slot = (int)(j % C) * 64 + l;
			so[slot] = res.out;
			if (p.verdict)
				sv[slot] = (uint8_t)res.verdict;
		}
		if ((j + 1) % C == 0 || j + 1 == nsteps) {
			const uint64_t f0 = gstep(j - j % C) * 64;
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			const uint64_t cntp = f0 < p.n ? (p.n - f0 < (uint64_t)C * 64 ? p.n - f0 : (uint64_t)C * 64) : 0;
			if (defer_ok && cntp == (uint64_t)C * 64 && j + 1 < nsteps) {
				pend = true; // stored after the next round's issue
				pf0 = f0;
			} else {
				for (uint64_t i = l; i < cntp; i += 64) {
					if (p.out)
						gbl(p.out)[f0 + i] = so[i];
					if (p.verdict)
						gbl(p.verdict)[f0 + i] = sv[i];
				}
			}
		}
		cur = nxt;
		nxt = nn;
		--ia;
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef CGCK_LPX_ISSUE
}

template <bool DESC>
static hipError_t launch_slot_t(const KParams &p, int max_blocks, bool nt, hipStream_t st)
{
	// each wave owns a contiguous packet range of >= ~64 packets
	const unsigned blocks = grid_blocks(p.n, 4 * 64, max_blocks);
	if (nt) {
		CGCK_NOTE_KERNEL("slot_kernel<%s, true>", tf(DESC));
		hipLaunchKernelGGL((slot_kernel<DESC, true>), dim3(blocks), dim3(256), 0, st, p);
	} else {
		CGCK_NOTE_KERNEL("slot_kernel<%s, false>", tf(DESC));
		hipLaunchKernelGGL((slot_kernel<DESC, false>), dim3(blocks), dim3(256), 0, st, p);
	}
	return hipGetLastError();
}

template <bool DESC>
static hipError_t launch_lppp_t(const KParams &p, int max_blocks, bool nt, hipStream_t st)
{
	const unsigned blocks = grid_blocks(p.n, 256, max_blocks);
	if (nt) {
		CGCK_NOTE_KERNEL("lppp_kernel<%s, true>", tf(DESC));
		hipLaunchKernelGGL((lppp_kernel<DESC, true>), dim3(blocks), dim3(256), 0, st, p);
	} else {
		CGCK_NOTE_KERNEL("lppp_kernel<%s, false>", tf(DESC));
		hipLaunchKernelGGL((lppp_kernel<DESC, false>), dim3(blocks), dim3(256), 0, st, p);
	}
	return hipGetLastError();
}

hipError_t launch_lppp(const KParams &p, int num_cus, bool nt, hipStream_t st)
{
	return p.desc ? launch_lppp_t<true>(p, num_cus * 8, nt, st) : launch_lppp_t<false>(p, num_cus * 8, nt, st);
}

hipError_t launch_slot(const KParams &p, int num_cus, bool nt, hipStream_t st)
{
	return p.desc ? launch_slot_t<true>(p, num_cus * 8, nt, st) : launch_slot_t<false>(p, num_cus * 8, nt, st);
}

hipError_t launch_slotd(const KParams &p, int num_cus, hipStream_t st)
{
	static const int wpc = [] { // $CGCK_SLOTD_WPC: waves per CU
		const char *e = CGCK_ENV("CGCK_SLOTD_WPC");
		return e && atoi(e) > 0 ? atoi(e) : 6;
	}();
	const dim3 g(grid_blocks(p.n, kSlotdChunk, (uint64_t)num_cus * wpc));
	const size_t lds = 2 * 8192 + 64 * 4 + kWaveStage * 4 + kWaveStage;
	if (p.desc) {
		CGCK_NOTE_KERNEL("slotd_kernel<true>");
		hipLaunchKernelGGL((slotd_kernel<true>), g, dim3(64), lds, st, p);
	} else {
		CGCK_NOTE_KERNEL("slotd_kernel<false>");
		hipLaunchKernelGGL((slotd_kernel<false>), g, dim3(64), lds, st, p);
	}
	return hipGetLastError();
}

// The launchers' lab halves, on their locals: the lab launch's status, or nothing (the product launch then runs).
static std::optional<hipError_t> launch_lpd_lab(const KParams &p, const dim3 &g, int num_cus, hipStream_t st)
{
	static const int depth = [] { // $CGCK_LPD_D: ring slots 2..4
		const char *e = CGCK_ENV("CGCK_LPD_D");
		const int d = e ? atoi(e) : 0;
		return d >= 2 && d <= 4 ? d : 2;
	}();
	static const int lc = [] { // $CGCK_LPD_LC: ring phases of the loader/consumer form (0: per-wave form)
		const char *e = CGCK_ENV("CGCK_LPD_LC");
		const int v = e ? atoi(e) : 0;
		return v >= 2 && v <= 5 ? v : 0;
	}();
	if (lc) {
		static const int wgpc = [] { // $CGCK_LPD_WGPC: workgroups per CU
			const char *e = CGCK_ENV("CGCK_LPD_WGPC");
			return e && atoi(e) > 0 ? atoi(e) : 3;
		}();
		const dim3 glc(grid_blocks(p.n, 192 * 16, (uint64_t)num_cus * wgpc)); // >= 16 phases per workgroup
#define CGCK_LPDLC(PP)                                                                           \
	do {                                                                                     \
		CGCK_NOTE_KERNEL("lpd_lc_kernel<%d>", PP);                                       \
		hipLaunchKernelGGL((lpd_lc_kernel<PP>), glc, dim3(256), (PP) * 3 * 4096, st, p); \
	} while (0)
		switch (lc) {
		case 2: CGCK_LPDLC(2); break;
		case 4: CGCK_LPDLC(4); break;
		case 5: CGCK_LPDLC(5); break;
		default: CGCK_LPDLC(3); break;
		}
#undef CGCK_LPDLC
		return hipGetLastError();
	}
	static const int wr = [] { // $CGCK_LPD_W: lpdw_kernel (writer wave), steps per chunk 16 | 32
		const char *e = CGCK_ENV("CGCK_LPD_W");
		return e ? atoi(e) : 0;
	}();
	if (wr == 16 || wr == 32) {
		if (wr == 16) {
			CGCK_NOTE_KERNEL("lpdw_kernel<%d, 16>", 2);
			hipLaunchKernelGGL((lpdw_kernel<2, 16>), g, dim3(128), 2 * 4096 + 16 * 256, st, p);
		} else {
			CGCK_NOTE_KERNEL("lpdw_kernel<%d, 32>", 2);
			hipLaunchKernelGGL((lpdw_kernel<2, 32>), g, dim3(128), 2 * 4096 + 32 * 256, st, p);
		}
		return hipGetLastError();
	}
	static const bool sink = CGCK_ENV("CGCK_LPD_SINK") != nullptr; // measure without output stores
	KParams q = p;
	if (sink)
		q.contig = 2;
	static const int chunk = [] { // $CGCK_LPD_C: steps per output chunk (1, 4, 8, 16, 32, 64)
		const char *e = CGCK_ENV("CGCK_LPD_C");
		const int c = e ? atoi(e) : 32;
		return c == 1 || c == 4 || c == 8 || c == 16 || c == 64 ? c : 32;
	}();
	static const int sp = [] { // $CGCK_LPD_SP: flush store policy 0 nt, 1 default, 2 sc1
		const char *e = CGCK_ENV("CGCK_LPD_SP");
		const int v = e ? atoi(e) : 2;
		return v >= 0 && v <= 5 ? v : 2; // 3..5: the same, stored after the next step's issue
	}();
#define CGCK_LPD_S(DD, CC, SS)                                                                   \
	do {                                                                                     \
		CGCK_NOTE_KERNEL("lpd_kernel<%d, %d, %d>", DD, CC, SS);                          \
		hipLaunchKernelGGL((lpd_kernel<DD, CC, SS>), g, dim3(64), (DD) * 4096 + (CC) * 256, st, q); \
	} while (0)
#define CGCK_LPD(DD, CC)                                                                         \
	do {                                                                                     \
		if (sp == 1)                                                                     \
			CGCK_LPD_S(DD, CC, 1);                                                   \
		else if (sp == 0)                                                                \
			CGCK_LPD_S(DD, CC, 0);                                                   \
		else                                                                             \
			CGCK_LPD_S(DD, CC, 2);                                                   \
	} while (0)
#define CGCK_LPD_D(DD)                                                                           \
	do {                                                                                     \
		if (chunk == 1)                                                                  \
			CGCK_LPD(DD, 1);                                                         \
		else if (chunk == 4)                                                             \
			CGCK_LPD(DD, 4);                                                         \
		else if (chunk == 8)                                                             \
			CGCK_LPD(DD, 8);                                                         \
		else if (chunk == 16)                                                            \
			CGCK_LPD(DD, 16);                                                        \
		else if (chunk == 64)                                                            \
			CGCK_LPD(DD, 64);                                                        \
		else                                                                             \
			CGCK_LPD(DD, 32);                                                        \
	} while (0)
	if (sp == 5 && depth == 2 && chunk == 32) { // the deferred flush, sc1 (lab A/B)
		CGCK_LPD_S(2, 32, 5);
		return hipGetLastError();
	}
	switch (depth) {
	case 3: CGCK_LPD_D(3); break;
	case 4: CGCK_LPD_D(4); break;
	default: CGCK_LPD_D(2); break;
	}
#undef CGCK_LPD_D
#undef CGCK_LPD
#undef CGCK_LPD_S
	return hipGetLastError();
}

static std::optional<hipError_t> launch_lpw_lab(const KParams &p, KParams &q, const dim3 &g, size_t lds, int num_cus,
						int wpc, hipStream_t st)
{
	constexpr int C = 4; // launch_lpw's
	static const bool nocons = CGCK_ENV("CGCK_LPW_NOCONS") != nullptr;
	static const bool noflush = CGCK_ENV("CGCK_LPW_NOFLUSH") != nullptr;
	static const bool nodefer = CGCK_ENV("CGCK_LPW_NODEFER") != nullptr; // the end-of-chunk flush
	if (nocons)
		q.contig = 4;
	else if (noflush)
		q.contig = 5;
	else if (nodefer)
		q.contig = 6;
	// $CGCK_LPW_C=8: chunks of 8 steps for batches without verdicts (20 KiB
	// of LDS per workgroup)
	static const bool c8 = CGCK_ENV("CGCK_LPW_C") && atoi(CGCK_ENV("CGCK_LPW_C")) == 8;
	if (c8 && !p.verdict) {
		constexpr int C8 = 8;
		const dim3 g8(grid_blocks(p.n, 64 * C8, (uint64_t)num_cus * wpc));
		const size_t lds8 = 2 * kLpwSlot + 2 * 1024 + C8 * 64 * 4;
		if (p.desc) {
			CGCK_NOTE_KERNEL("lpw_kernel<true, 8, false>");
			hipLaunchKernelGGL((lpw_kernel<true, C8, false>), g8, dim3(64), lds8, st, q);
		} else {
			CGCK_NOTE_KERNEL("lpw_kernel<false, 8, false>");
			hipLaunchKernelGGL((lpw_kernel<false, C8, false>), g8, dim3(64), lds8, st, q);
		}
		return hipGetLastError();
	}
	// $CGCK_LPW_X=1: lpx_kernel, two rounds in flight (7 waves per CU)
	static const bool two = CGCK_ENV("CGCK_LPW_X") && atoi(CGCK_ENV("CGCK_LPW_X")) != 0;
	if (two) {
		static const int wpcx = [] {
			const char *e = CGCK_ENV("CGCK_LPX_WPC");
			return e && atoi(e) > 0 ? atoi(e) : 7;
		}();
		const dim3 gx(grid_blocks(p.n, 64 * C, (uint64_t)num_cus * wpcx));
		const size_t ldsx = 2 * kLpwSlot + 3 * 1024 + 4 * kLpwWin + C * 64 * (p.verdict ? 5 : 4);
		if (p.desc) {
			CGCK_NOTE_KERNEL("lpx_kernel<true, %d>", C);
			hipLaunchKernelGGL((lpx_kernel<true, C>), gx, dim3(64), ldsx, st, q);
		} else {
			CGCK_NOTE_KERNEL("lpx_kernel<false, %d>", C);
			hipLaunchKernelGGL((lpx_kernel<false, C>), gx, dim3(64), ldsx, st, q);
		}
		return hipGetLastError();
	}
	// $CGCK_LPW_W=1: the writer wave (lost: capped at 128 VGPRs it spills,
	// 52.5-53.7 % vs 70.3-70.4 %, profiles/r02/imix/README.md)
	static const bool wr = CGCK_ENV("CGCK_LPW_W") && atoi(CGCK_ENV("CGCK_LPW_W")) != 0;
	if (wr) {
		if (p.desc) {
			CGCK_NOTE_KERNEL("lpw_kernel<true, %d, true>", C);
			hipLaunchKernelGGL((lpw_kernel<true, C, true>), g, dim3(128), lds, st, q);
		} else {
			CGCK_NOTE_KERNEL("lpw_kernel<false, %d, true>", C);
			hipLaunchKernelGGL((lpw_kernel<false, C, true>), g, dim3(128), lds, st, q);
		}
		return hipGetLastError();
	}
	return std::nullopt;
}

static std::optional<hipError_t> launch_lpp_lab(const KParams &p, int mb, bool nt, int shape, hipStream_t st)
{
	switch (shape) {
	case 1:
		return p.desc ? launch_lpp_t<true, 6, true>(p, mb, nt, st) : launch_lpp_t<false, 6, true>(p, mb, nt, st);
	case 3:
		return p.desc ? launch_lpp_t<true, 4, false>(p, mb, nt, st) : launch_lpp_t<false, 4, false>(p, mb, nt, st);
	case 0:
		return p.desc ? launch_lpp_t<true, 4, true>(p, mb, nt, st) : launch_lpp_t<false, 4, true>(p, mb, nt, st);
	}
	return std::nullopt;
}
