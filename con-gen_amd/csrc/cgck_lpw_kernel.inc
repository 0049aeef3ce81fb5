// cgck_lpw_kernel.inc — the lpw kernel (lane per packet over DMA'd windows of a
// step's span; the comment above its include in cgck_lane.hip), its window
// geometry and its step / issue helpers.  One text, four kernels: cgck_lane.hip
// compiles it as lpw_kernel (CGCK_LPW_IP6 false, IPv4), cgck_lpw6.hip as
// lpw6_kernel (true, CGCK_IP6), cgck_lpf.hip as lpf_kernel (IPv4 with
// CGCK_LPW_FILL true: the in-place field stores of CGCK_STORE and the bad
// counters, the comment there) and cgck_lpwx.hip as lpwx_kernel (CGCK_LPW_MIXED
// true, CGCK_MIXED: the family and the finish chosen per lane, the comment
// there), each in a module of its own, so the IPv4 kernel keeps its code
// (DESIGN.md §5.6, §5.7, §5.8).  The includer defines CGCK_LPW_KERNEL,
// CGCK_LPW_IP6, CGCK_LPW_FILL and CGCK_LPW_MIXED and has included cgck_lane.h.
// Everything the fill variant adds sits behind `if constexpr (FILL)`, everything
// the mixed one adds behind `if constexpr (MIXED)`; the mixed kernel alone has a
// fourth template parameter, DRING (false: a descriptor array that is not
// 16-byte aligned, read from global memory each step instead of by DMA).
#if !CGCK_LAB || !defined(CGCK_LPW_DMA) // compile-time A/B knobs of the lab build only
#undef CGCK_LPW_DMA
#define CGCK_LPW_DMA 8
#endif
// 0: instruction i moves chunks [64 i, 64 i + 64) of the window (1 KiB
// contiguous); 1: lane l moves chunks [8 l, 8 l + 8) over the 8 instructions,
// so its own run lands in conflict-free LDS places (A/B builds)
#if !CGCK_LAB || !defined(CGCK_LPW_SLOTMAJOR)
#undef CGCK_LPW_SLOTMAJOR
#define CGCK_LPW_SLOTMAJOR 0
#endif
// 1: the window's prefix with a lane per pair of chunks (4 wave scans a
// window), 0: a lane per chunk (8) — the A/B builds' knob
#if !CGCK_LAB || !defined(CGCK_LPW_PAIR)
#undef CGCK_LPW_PAIR
#define CGCK_LPW_PAIR 1
#endif
// The fill variant's A/B knobs.  CGCK_LPF_NT: the cache policy of the data
// DMA.  1: nontemporal, as lpw's; 0: cached; 2 (the product): cached for a
// CGCK_STORE batch, whose lines are then still in the L2 when the fields are
// stored into them (16M IMIX packets, FILL_BOTH: 2.20 -> 1.73 ms packed, 2.42
// -> 2.00 ms in ring slots), nontemporal otherwise (VERIFY with counters: 1.06
// ms against 1.15 cached; profiles/lpf/).  CGCK_LPF_DEFER 1: a step's field
// stores issued after the next round's DMA (cgck_lpf.hip); 0: at the end of
// their step, under the counted waits as they stand.
#if !CGCK_LAB || !defined(CGCK_LPF_NT)
#undef CGCK_LPF_NT
#define CGCK_LPF_NT 2
#endif
#if !CGCK_LAB || !defined(CGCK_LPF_DEFER)
#undef CGCK_LPF_DEFER
#define CGCK_LPF_DEFER 1
#endif
// glds16_nt (cgck_device.h) without the nontemporal policy
__device__ __forceinline__ void glds16_cached(const void *gsrc, uint32_t lds_dst)
{
	uint32_t keep;
	asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
		     "s_mov_b32 m0, %0"
		     : "=&s"(keep)
		     : "v"(gsrc), "s"(lds_dst)
		     : "memory");
}
// the data DMA of this batch goes through the cache (the fill variant only)
__device__ __forceinline__ bool lpw_dma_cached(uint32_t flags)
{
	return CGCK_LPW_FILL && (CGCK_LPF_NT == 0 || (CGCK_LPF_NT == 2 && (flags & CGCK_STORE)));
}
// LDS index (in 16-byte units) of window chunk idx
__device__ __forceinline__ int lpw_at(int idx)
{
#if CGCK_LPW_SLOTMAJOR
	return ((idx & 7) << 6) | (idx >> 3);
#else
	return idx;
#endif
}
constexpr int kLpwDma = CGCK_LPW_DMA;            // data DMA instructions per window
constexpr int kLpwWin = kLpwDma * 64;            // chunks a window owns (no overlap: a header
						 // split over two windows is gathered from both)
constexpr int kLpwSlot = kLpwDma * 1024;         // bytes per ring slot

struct LpwStep {
	uint64_t a0;
	int len, q, nch, e;
	bool ok;
	uint64_t cs, ce; // the lane's packet in window coordinates: absolute chunks (chained) or list positions
	uint64_t dl;     // gathered: (a0 >> 4) - cs, the chunk address of list position x is dl + x
	uint64_t S, E;   // wave: span
	uint32_t nwin;   // wave: windows (0: computed from global memory)
	bool gather;     // wave: the windows are the packets' chunk runs concatenated in lane order
};

template <bool DESC>
__device__ __forceinline__ LpwStep lpw_step(const KParams &p, uint64_t first, const DescW &d)
{
	const int l = threadIdx.x & 63;
	const Pkt pk = decode<DESC>(p, first + l, p.n, d);
	LpwStep s;
	s.a0 = pk.a0;
	s.len = (int)pk.len;
	s.ok = pk.ok;
	s.q = (int)(pk.a0 & 15);
	s.nch = nchunks(pk.a0, pk.len);
	s.e = s.q + s.len - 16 * (s.nch - 1);
	s.cs = pk.a0 >> 4;
	s.ce = s.cs + (uint64_t)s.nch;
	// Over the non-empty packets in lane order: running maxima of the starts
	// and of the ends (inclusive DPP scans of 32-bit offsets from the first
	// non-empty packet, then shifted by one lane).  The step chains when every
	// start is >= the starts before it and <= the furthest end before it: then
	// [S, E) is exactly the union of the packets' chunks.
	const bool ne = s.ok && s.nch > 0;
	const uint64_t nonempty = __ballot(ne);
	const int f = nonempty ? __ffsll((long long)nonempty) - 1 : 0; // first non-empty lane
	// the wave's values (base, span, windows) by readlane: scalar, so the
	// window loop and the round bookkeeping (pre, pend, sage) stay uniform
	// branches instead of exec-masked ones
	const uint64_t base = readlane64(s.cs, f);
	const uint64_t ds = s.cs - base, de = s.ce - base;
	const bool far = ne && (s.cs < base || de > 0x7fffffffull); // before the first, or too far for 32 bits
	const uint32_t rs = ne && !far ? (uint32_t)ds : 0u, re = ne && !far ? (uint32_t)de : 0u;
	const uint32_t mS = wave_max_scan_dpp(rs), mE = wave_max_scan_dpp(re);
	const uint32_t prev_s = (uint32_t)__shfl_up((int)mS, 1, 64), prev_e = (uint32_t)__shfl_up((int)mE, 1, 64);
	const bool brk = far || (ne && l > f && (rs < prev_s || rs > prev_e));
	s.S = nonempty ? base : 0;
	s.E = nonempty ? base + (uint64_t)__builtin_amdgcn_readlane(mE, 63) : 0;
	s.dl = 0;
	s.gather = false;
	const uint64_t span = s.E - s.S;
	if (!__any(brk) && span <= 16 * kLpwWin) {
		s.nwin = span ? (uint32_t)((span + kLpwWin - 1) / kLpwWin) : 1u; // (empty packets: one window, nothing moved)
	} else {
		// Not back to back (ring slots, gaps, reordered frames): the windows
		// walk the list of the packets' chunk runs concatenated in lane order,
		// packet p at list positions [P_p, P_p + nch_p) (an exclusive scan of
		// the chunk counts), gathered by the same DMA (lpw_issue).  The
		// per-window work is unchanged in list coordinates.
		const uint32_t nc = ne ? (uint32_t)s.nch : 0u;
		const uint32_t incl = wave_scan_dpp(nc);
		const uint32_t T = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
		s.cs = incl - nc;
		s.ce = incl;
		s.dl = (pk.a0 >> 4) - s.cs;
		s.S = 0;
		s.E = T;
		s.gather = true;
		s.nwin = T > 16 * kLpwWin ? 0u : T ? (T + kLpwWin - 1) / kLpwWin : 1u;
	}
	s.nwin = __builtin_amdgcn_readfirstlane(s.nwin);
	return s;
}

// One round: window t of step s (live) or zero lines, plus the descriptors
// of step dstep (when dlive) into the descriptor slot.  A gathered step
// (gather) maps each list position of the window to its packet's chunk: the
// packets starting in the window mark their position in an owner table built
// in the target slot itself (free until this round's DMA lands; every row's
// address is computed before the first DMA is issued), a max-scan per row of 64
// positions fills the table forward, the row's carry is the last packet that
// started before it (a ballot), and the chunk address is that packet's dl
// (staged next to the table) plus the position.
template <bool DESC>
__device__ __forceinline__ void lpw_issue(const KParams &p, uint64_t wb, uint64_t E, bool live, bool gather,
					  uint64_t cs, uint64_t ce, uint64_t dl, uint8_t *slot, uint32_t lds_slot,
					  uint64_t dfirst, bool dlive, uint32_t lds_dslot, const uint8_t *zero)
{
	// window [wb, wb + 512) of a span ending at E (values, not a step
	// reference: selecting between two steps' structs put them in scratch)
	const int l = threadIdx.x & 63;
	const uint32_t base = __builtin_amdgcn_readfirstlane(lds_slot); // wave-uniform: M0
	if (gather && live) {
		uint32_t *own = reinterpret_cast<uint32_t *>(slot);       // kLpwWin entries: owner lane + 1, 0 none
		uint64_t *dls = reinterpret_cast<uint64_t *>(slot + 4 * kLpwWin); // 64 lanes' dl
		// one element type for the table, and memory clobbers between the
		// phases: the reads must not move above the zeroing or the marks (the
		// slot holds the last window's packet bytes until it is cleared)
#pragma unroll
		for (int r = 0; r < kLpwDma; ++r)
			own[64 * r + l] = 0u;
		asm volatile("" ::: "memory");
		const bool ne = ce > cs;
		if (ne && cs >= wb && cs < wb + kLpwWin)
			own[cs - wb] = (uint32_t)l + 1;
		dls[l] = dl;
		asm volatile("" ::: "memory");
		// every row's address first: row i's DMA lands on bytes [1024 i, 1024 i
		// + 1024) of the slot, over the table the later rows read
		const void *src[kLpwDma];
#pragma unroll
		for (int i = 0; i < kLpwDma; ++i) {
			const uint64_t x = wb + 64 * i + l;
			const uint64_t before = __ballot(ne && cs < wb + 64 * i); // packets started before this row
			const int carry = before ? 64 - __builtin_clzll(before) : 0; // last such lane + 1
			const uint32_t m = wave_max_scan_dpp(own[64 * i + l]);
			const int o = (int)(m > (uint32_t)carry ? m : (uint32_t)carry) - 1;
			const uint64_t d = dls[o > 0 ? o : 0];
			src[i] = x < E ? reinterpret_cast<const void *>((d + x) << 4) : zero;
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the table is read: the slot may be refilled
		if (lpw_dma_cached(p.flags)) {
#pragma unroll
			for (int i = 0; i < kLpwDma; ++i)
				glds16_cached(src[i], base + 1024 * i);
		} else {
#pragma unroll
			for (int i = 0; i < kLpwDma; ++i)
				glds16_nt(src[i], base + 1024 * i);
		}
	} else {
#pragma unroll
		for (int i = 0; i < kLpwDma; ++i) {
#if CGCK_LPW_SLOTMAJOR
			const uint64_t c = wb + 8 * l + i; // lane l's 8 chunks land at +16 l of each KiB
#else
			const uint64_t c = wb + 64 * i + l;
#endif
			const void *src = live && c < E ? reinterpret_cast<const void *>(c << 4) : zero;
			if (lpw_dma_cached(p.flags))
				glds16_cached(src, base + 1024 * i);
			else
				glds16_nt(src, base + 1024 * i);
		}
	}
	const uint64_t doff = 12 * dfirst + 16 * (uint64_t)l;
	const bool dok = DESC && dlive && l < 48 && doff < 12 * p.n;
	glds16_nt(dok ? reinterpret_cast<const void *>(reinterpret_cast<const uint8_t *>(p.desc) + doff) : zero,
		  __builtin_amdgcn_readfirstlane(lds_dslot));
}

template <bool DESC>
__device__ __forceinline__ DescW lpw_desc_lds(const uint8_t *dslot)
{
	DescW d{0, 0, 0};
	if (DESC) {
		const uint32_t *q = reinterpret_cast<const uint32_t *>(dslot) + 3 * (threadIdx.x & 63);
		d.lo = q[0];
		d.hi = q[1];
		d.w2 = q[2];
	}
	return d;
}

// --- the fill variant's helpers (used under `if constexpr (FILL)` only) ---
// The wait for the previous round that leaves this round's kLpwDma + 1 DMA
// instructions and `extra` later VMEM instructions (stores) in flight.
// `extra` is wave-uniform and never more than the stores really issued after
// the round waited for (fewer only waits for more).
__device__ __forceinline__ void lpf_wait(int extra)
{
#define CGCK_LPF_WAIT(x)                                                                       \
	case x:                                                                                \
		asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1 + x) : "memory");         \
		break;
	switch (extra < 10 ? extra : 10) {
		CGCK_LPF_WAIT(1)
		CGCK_LPF_WAIT(2)
		CGCK_LPF_WAIT(3)
		CGCK_LPF_WAIT(4)
		CGCK_LPF_WAIT(5)
		CGCK_LPF_WAIT(6)
		CGCK_LPF_WAIT(7)
		CGCK_LPF_WAIT(8)
		CGCK_LPF_WAIT(9)
		CGCK_LPF_WAIT(10)
	default:
		asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1) : "memory");
	}
#undef CGCK_LPF_WAIT
}

// One field of a step (the IP checksums at a0 + 10, or the L4 checksums at a0
// + hl + fo) stored in place, store16's bytes: a 16-bit store, or two byte
// stores when some lane's address is odd.  Returns the VMEM instructions
// issued (0, 1 or 2), wave-uniform and exact: the stores are inline assembly
// executed by all 64 lanes, so the compiler neither drops, merges nor branches
// over one.  A lane with nothing to store repeats the first storing lane's
// store (the same value to the same address: harmless, and no address outside
// a frame is ever written).
__device__ __forceinline__ int lpf_store_field(bool on, uint64_t addr, uint32_t v)
{
	const uint64_t m = __ballot(on);
	if (!m)
		return 0;
	const int f = __ffsll((long long)m) - 1;
	const uint64_t a = on ? addr : readlane64(addr, f);
	const uint32_t x = on ? v : (uint32_t)__builtin_amdgcn_readlane((int)v, f);
	if (__ballot(on && (addr & 1))) {
		asm volatile("global_store_byte %0, %1, off" ::"v"(a), "v"(x) : "memory");
		asm volatile("global_store_byte %0, %1, off offset:1" ::"v"(a), "v"(x >> 8) : "memory");
		return 2;
	}
	asm volatile("global_store_short %0, %1, off" ::"v"(a), "v"(x) : "memory");
	return 1;
}

// A step's pending field stores: fp bit 0 the IP field (fv's low half to fa),
// bit 1 the L4 field (fv's high half to fb).
__device__ __forceinline__ int lpf_store_fields(uint32_t fp, uint64_t fa, uint64_t fb, uint32_t fv)
{
	return lpf_store_field(fp & 1, fa, fv & 0xffffu) + lpf_store_field(fp & 2, fb, fv >> 16);
}

// --- the mixed variant's helpers (used under `if constexpr (MIXED)` only) ---
// The lane's family (the high nibble of its packet's first byte, byte q of
// header chunk 0; 0 for a lane without a packet byte) and both header decodes,
// each with its own family's lanes as the activity flag: the wave-uniform
// paths inside them (shifted, unaligned, all5, the header-length bound) consult
// only those lanes, and the other family's lanes get values nobody reads.
// Neither decoder forms a load here: header<8>() has all six header chunks
// (its fetch of chunks 4..5 is compiled for fewer than six only) and header6()
// reads registers, so no address is ever built from the other family's fields.
__device__ __forceinline__ void lpwx_headers(const uint4 (&w8)[8], const LpwStep &s, uint32_t flags, uint32_t &fam,
					     Hdr &h, Hdr6 &h6)
{
	const int qd = s.q >> 2;
	const uint32_t d0 = qd == 0 ? w8[0].x : qd == 1 ? w8[0].y : qd == 2 ? w8[0].z : w8[0].w;
	const uint32_t v = (d0 >> (8 * (s.q & 3) + 4)) & 15u;
	fam = s.ok && s.len > 0 && (v == 4 || v == 6) ? v : 0u;
	h = header<8, false>(w8, nullptr, s.nch, s.q, s.len, flags | kFlagL4Auto, fam == 4);
	h6 = header6(w8, s.q, flags, fam == 6);
}

// The lane's finish by its family: result_t<true>() (the pseudo-header by the
// packet's own ip_p) or result6() without the UDP zero skip (RFC 8200 §8.1: a
// zero UDP checksum over IPv6 is compared and comes out bad); neither family:
// CGCK_NOT_IP, no byte of a packet: CGCK_BAD_LEN.  No stores, and the counters
// are the caller's (p.bad is not passed on).  result6()'s walk of an extension
// chain reads global memory only in lanes of its activity flag.
__device__ __forceinline__ Res lpwx_result(const KParams &p, const LpwStep &s, uint32_t T, uint32_t fam, const Hdr &h,
					   const Hdr6 &h6)
{
	KParams p4 = p, p6 = p;
	p4.flags = p.flags | kFlagL4Auto;
	p4.bad = nullptr;
	p6.flags = p.flags & ~(uint32_t)CGCK_V_UDP_ZERO_SKIP;
	p6.bad = nullptr;
	const Res r4 = result_t<true>(p4, s.a0, s.len, T, h);
	const Res r6 = result6(p6, s.a0, s.len, T, h6, fam == 6);
	if (s.len <= 0)
		return Res{0, (uint32_t)CGCK_BAD_LEN};
	return fam == 4 ? r4 : fam == 6 ? r6 : Res{0, (uint32_t)CGCK_NOT_IP};
}

#if CGCK_LPW_MIXED
template <bool DESC, int C, bool W, bool DRING>
#else
template <bool DESC, int C, bool W>
#endif
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(W ? 4 : 1))) void CGCK_LPW_KERNEL(KParams p)
{
	constexpr bool IP6 = CGCK_LPW_IP6; // lpw6_kernel: the IPv6 finish (header6, result6: cgck_lane.h)
	constexpr bool FILL = CGCK_LPW_FILL; // lpf_kernel: field stores and bad counters (cgck_lpf.hip)
	constexpr bool MIXED = CGCK_LPW_MIXED; // lpwx_kernel: both finishes, chosen per lane (cgck_lpwx.hip)
#if CGCK_LPW_MIXED
	constexpr bool DR = DESC && DRING; // the descriptors travel by DMA
#else
	constexpr bool DR = DESC;
#endif
	static_assert(!(FILL && (IP6 || W)), "lpf is IPv4, one wave");
	static_assert(!(MIXED && (IP6 || FILL || W)), "lpwx decides the family per lane, stores nothing, one wave");
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	uint8_t *dring = smem + 2 * kLpwSlot; // 2 x 1 KiB descriptor slots (64 lanes x 16 B; 768 B used)
	uint32_t *so = reinterpret_cast<uint32_t *>(dring + 2 * 1024);
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

	if (W && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 1) {
		// The writer wave (as dstr_kernel's): wave 0 stages a chunk's outputs
		// and verdicts and hands them over at barrier H; this wave reads them
		// into registers, releases the staging at barrier R (wave 0 meets it
		// just before its first staging write of the next chunk) and stores
		// them, so no output store sits in wave 0's in-order vmcnt (IMIX: the
		// flush alone cost 3-7 points, profiles/r02/imix/README.md).
		const uint64_t KD = nsteps / C;
		for (uint64_t k = 0; k < KD; ++k) {
			wg_barrier(); // H_k
			const uint64_t f0 = gstep(k * C) * 64;
			const uint64_t cntp = f0 < p.n ? (p.n - f0 < (uint64_t)C * 64 ? p.n - f0 : (uint64_t)C * 64) : 0;
			uint32_t vo[C];
			uint8_t vv[C];
#pragma unroll
			for (int i = 0; i < C; ++i) {
				vo[i] = so[64 * i + l];
				vv[i] = p.verdict ? sv[64 * i + l] : 0;
			}
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			if (k + 1 < KD)
				wg_barrier(); // R_k: the staging is free
#pragma unroll
			for (int i = 0; i < C; ++i) {
				if ((uint64_t)(64 * i + l) < cntp) {
					if (p.out)
						gbl(p.out)[f0 + 64 * i + l] = vo[i];
					if (p.verdict)
						gbl(p.verdict)[f0 + 64 * i + l] = vv[i];
				}
			}
		}
		return;
	}

	LpwStep cur = lpw_step<DESC>(p, first_of(0), load_desc<DESC>(p, first_of(0) + l, p.n));
	LpwStep nxt = lpw_step<DESC>(p, first_of(1), load_desc<DESC>(p, first_of(1) + l, p.n));
	LpwStep nn = nxt;
	uint32_t kiss = 0;      // rounds issued (round k uses data slot k & 1)
	// A full chunk's outputs leave as one 16-byte store per lane (C = 4: 256
	// outputs) issued right AFTER the next DMA round, whose wait then leaves
	// it in flight (vmcnt + 1): the store has a whole round to complete before
	// a wait must cover it.  Stored at the end of its chunk instead (in front
	// of the next round in the in-order vmcnt), the flush cost IMIX 3-7 points
	// (profiles/r02/imix/README.md).  Lab mode 6: the end-of-chunk flush.
	static_assert(C % 4 == 0, "C / 4 16-byte stores per lane per chunk");
	const bool defer_ok = !W && p.out && !p.verdict && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 &&
			      p.contig != 6 && p.contig != 5;
	bool pend = false; // a chunk's outputs wait in the staging for the next round
	int sage = 0;      // waits left that may leave the chunk store in flight
	uint64_t pf0 = 0;  // its first packet
	bool pre = false;       // cur's window 0 (with step j + 2's descriptors) already issued
	// FILL: the last step's field stores, carried in plain scalars until the
	// next round is issued (or flushed where none comes), the stores issued
	// after the last round, and the step totals of the bad counters
	bool fpend = false;
	uint32_t fp = 0, fv = 0, exprev = 0, nbad_ip = 0, nbad_l4 = 0;
	uint64_t fa = 0, fb = 0;
	for (uint64_t j = 0; j < nsteps; ++j) {
		const uint64_t first = first_of(j);
		uint32_t acc = 0, corr = 0;
		Hdr h{};
		Hdr6 h6{};
		uint32_t fam = 0; // MIXED: the lane's family, 4 or 6 (0: neither, or no byte to read it from)
		if (first < p.n && cur.nwin > 0) {
			// the header's chunks, loop-carried in native vectors (an array of
			// uint4, a union type, was put in scratch)
			u32x4_t t8[8];
#pragma unroll
			for (int u = 0; u < 8; ++u)
				t8[u] = u32x4_t{0, 0, 0, 0};
			if (!pre) {
				lpw_issue<DR>(p, cur.S, cur.E, true, cur.gather, cur.cs, cur.ce, cur.dl, smem + (kiss & 1) * kLpwSlot,
						lds0 + (kiss & 1) * kLpwSlot, first_of(j + 2), first_of(j + 2) < p.n,
						ldsd + (uint32_t)((j + 2) & 1) * 1024, zero);
				++kiss;
			}
			for (uint32_t t = 0; t < cur.nwin; ++t) {
				// the next round: this step's next window, or the next step's first
				// (carrying the descriptors of step j + 3)
				const bool more = t + 1 < cur.nwin;
				const bool nx = !more && first_of(j + 1) < p.n && nxt.nwin > 0;
				const uint64_t iwb = more ? cur.S + (uint64_t)(t + 1) * kLpwWin : nxt.S;
				const uint64_t iE = more ? cur.E : nxt.E;
				lpw_issue<DR>(p, iwb, iE, more || nx, more ? cur.gather : nxt.gather, more ? cur.cs : nxt.cs,
						more ? cur.ce : nxt.ce, more ? cur.dl : nxt.dl, smem + (kiss & 1) * kLpwSlot,
						lds0 + (kiss & 1) * kLpwSlot, first_of(j + 3), !more && first_of(j + 3) < p.n,
						ldsd + (uint32_t)((j + 3) & 1) * 1024, zero);
				++kiss;
				pre = nx;
				uint32_t ex = 0; // FILL: stores issued after this round
				if (pend) {
					const __amdgpu_buffer_rsrc_t rs = out_rsrc(p.out + pf0, C * 256);
#pragma unroll
					for (int i = 0; i < C / 4; ++i)
						bstore16<kSc1>(rs, 16 * (64 * i + l), reinterpret_cast<const u32x4_t *>(so)[64 * i + l]);
					pend = false;
					sage = 2;
					if constexpr (FILL)
						ex = C / 4;
				}
				if constexpr (FILL) {
					if (fpend) { // the previous step's fields: a whole round to land
						ex += (uint32_t)lpf_store_fields(fp, fa, fb, fv);
						fpend = false;
					}
				}
				// The wait for the previous round.  A store issued after this
				// round (sage 2) or after the previous one (sage 1) may stay in
				// flight: it sits between the two rounds in the in-order count.
				if constexpr (FILL) {
					// the stores issued after this round and after the one
					// waited for (between the two rounds in the in-order
					// count) may stay in flight; any other store issued since
					// (a flush) only makes the wait cover more
					lpf_wait((int)(ex + exprev));
					exprev = ex;
				} else if (sage > 0) {
					--sage;
					asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1 + C / 4) : "memory");
				} else {
					asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kLpwDma + 1) : "memory");
				}
				// (the covering vmcnt alone orders this wave's reads behind its
				// DMA; the barrier is kept in the one-wave form as measured)
				if (!W)
					__builtin_amdgcn_s_barrier();
				if (t == 0) { // step j + 2's descriptors came with window 0 of this step
					if constexpr (DR == DESC)
						nn = lpw_step<DESC>(p, first_of(j + 2), lpw_desc_lds<DESC>(dring + ((j + 2) & 1) * 1024));
					else // (no ring: a plain load after the wait, which the compiler waits for itself)
						nn = lpw_step<DESC>(p, first_of(j + 2), load_desc<DESC>(p, first_of(j + 2) + l, p.n));
				}
				if (p.contig == 4) // lab $CGCK_LPW_NOCONS: rounds without the per-window work
					continue;
				const uint4 *win = reinterpret_cast<const uint4 *>(smem + (kiss & 1) * kLpwSlot); // round kiss - 2
				const uint64_t wb = cur.S + (uint64_t)t * kLpwWin;
				const uint64_t we = wb + kLpwWin;
				// 1. reads of single chunks: the packet's edge chunks and its
				// header chunks cs .. cs + 7 that fall in this window (kept in
				// registers across windows; the header is read once per step)
				const bool head = cur.ok && cur.nch > 0 && cur.cs >= wb && cur.cs < we;
				const bool tail = cur.ok && cur.nch > 0 && cur.ce - 1 >= wb && cur.ce - 1 < we;
				const bool dw = !__any(cur.ok && ((cur.q | cur.len) & 3) != 0);
				if (__any(head && cur.q != 0))
					corr += head && cur.q != 0 ? lead_sum(win[lpw_at((int)(cur.cs - wb))], cur.q, dw) : 0u;
				if (__any(tail && cur.e != 16))
					corr += tail && cur.e != 16 ? trail_sum(win[lpw_at((int)(cur.ce - 1 - wb))], cur.e, dw) : 0u;
				const bool hwin = cur.ok && cur.cs + 8 > wb && cur.cs < we;
				if (!(p.flags & CGCK_RAW) && __any(hwin)) {
					const u32x4_t *win4 = reinterpret_cast<const u32x4_t *>(win);
#pragma unroll
					for (int u = 0; u < 8; ++u) {
						const uint64_t c = cur.cs + u;
						const bool in = hwin && c >= wb && c < we;
						const u32x4_t c8 = win4[in ? lpw_at((int)(c - wb)) : 0];
						t8[u] = in ? c8 : t8[u];
					}
				}
				// 2. lane per chunk: every owned chunk's sum (conflict-free 16-byte
				// reads), prefix-summed over the window in lane order; the rows'
				// scans are independent, their carries added after.  The prefix is
				// written over the slot's first rows, already read.
#if CGCK_LPW_SLOTMAJOR
				static_assert(kLpwDma == 8, "slot-major windows are 64 lanes x 8 chunks");
				// lane l owns chunks [8 l, 8 l + 8): local prefix, one wave scan
				uint32_t xs[8];
				uint32_t run = 0;
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const uint4 v = win[64 * i + l];
					run += wb + 8 * l + i < cur.E ? sum4(v, 0u) : 0u;
					xs[i] = run;
				}
				const uint32_t before = wave_scan_dpp(run) - run;
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				{
					typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
					u32x4v *p4 = reinterpret_cast<u32x4v *>(pfx + 8 * l);
					p4[0] = u32x4v{before + xs[0], before + xs[1], before + xs[2], before + xs[3]};
					p4[1] = u32x4v{before + xs[4], before + xs[5], before + xs[6], before + xs[7]};
				}
#elif CGCK_LPW_PAIR
				// A lane per PAIR of chunks (2 l, 2 l + 1 of each 2 KiB row
				// pair): half the wave scans of a lane per chunk (4 a window
				// instead of 8: the scans' DPP chain was the window's largest
				// issue cost, lpw being issue-bound on the packed layout —
				// SQ_ACTIVE_INST_ANY 0.49 of its wave cycles against dstr's
				// 0.20, profiles/r06/lpwpmc/).  The two 16-byte reads of a
				// lane go first / second by bit 3 of the lane, so lanes l and
				// l + 8 (32 bytes apart x 8) never hit the same banks.
				uint32_t ya[kLpwDma / 2], yb[kLpwDma / 2];
				const int sw = (l >> 3) & 1;
#pragma unroll
				for (int r = 0; r < kLpwDma / 2; ++r) {
					const int c = 128 * r + 2 * l;
					const uint4 va = win[c + sw], vb = win[c + 1 - sw];
					const uint32_t sa = wb + (uint64_t)(c + sw) < cur.E ? sum4(va, 0u) : 0u;
					const uint32_t sb = wb + (uint64_t)(c + 1 - sw) < cur.E ? sum4(vb, 0u) : 0u;
					const uint32_t s1 = sw ? sa : sb; // chunk c + 1's sum
					const uint32_t inc = wave_scan_dpp(sa + sb);
					yb[r] = inc;
					ya[r] = inc - s1;
				}
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				uint32_t carry = 0;
#pragma unroll
				for (int r = 0; r < kLpwDma / 2; ++r) {
					typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
					*reinterpret_cast<u32x2v *>(pfx + 128 * r + 2 * l) = u32x2v{ya[r] + carry, yb[r] + carry};
					carry += __builtin_amdgcn_readlane(yb[r], 63);
				}
#else
				uint32_t xs[kLpwDma];
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					const uint4 v = win[64 * r + l];
					xs[r] = wave_scan_dpp(wb + 64 * r + l < cur.E ? sum4(v, 0u) : 0u);
				}
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every read of the slot's chunks is done
				uint32_t *pfx = reinterpret_cast<uint32_t *>(smem + (kiss & 1) * kLpwSlot);
				uint32_t carry = 0;
#pragma unroll
				for (int r = 0; r < kLpwDma; ++r) {
					pfx[64 * r + l] = xs[r] + carry;
					carry += __builtin_amdgcn_readlane(xs[r], 63);
				}
#endif
				// 3. lane per packet: its chunks in this window as a prefix difference
				const uint64_t lo = cur.cs > wb ? cur.cs : wb;
				const uint64_t hi = cur.ce < we ? cur.ce : we;
				if (cur.ok && hi > lo)
					acc += pfx[(int)(hi - 1 - wb)] - (lo > wb ? pfx[(int)(lo - 1 - wb)] : 0u);
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slots are refilled next round
			}
			if (!(p.flags & CGCK_RAW)) {
				uint4 w8[8];
#pragma unroll
				for (int u = 0; u < 8; ++u)
					w8[u] = make_uint4(t8[u].x, t8[u].y, t8[u].z, t8[u].w);
				if constexpr (MIXED)
					lpwx_headers(w8, cur, p.flags, fam, h, h6);
				else if constexpr (IP6)
					h6 = header6(w8, cur.q, p.flags, cur.ok);
				else
				h = header<8, false>(w8, reinterpret_cast<const uint4 *>(cur.a0 & ~(uint64_t)15), cur.nch, cur.q,
						     cur.len, p.flags, cur.ok);
			}
			if (!pre) { // the last round was a zero round: drained before the next issue or a fallback
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				sage = 0; // (a looser count would no longer cover a round)
				exprev = 0;
			}
		} else if (first < p.n) {
			// not chained: the lane's packet straight from global memory
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			sage = 0;
			exprev = 0;
			pre = false;
			nn = lpw_step<DESC>(p, first_of(j + 2), load_desc<DESC>(p, first_of(j + 2) + l, p.n));
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
				if constexpr (MIXED)
					lpwx_headers(w8, cur, p.flags, fam, h, h6);
				else if constexpr (IP6)
					h6 = header6(w8, cur.q, p.flags, cur.ok);
				else
				h = header<8, false>(w8, c0, cur.nch, cur.q, cur.len, p.flags, cur.ok);
			}
		}
		if (W && j % C == 0 && j > 0)
			wg_barrier(); // R: the writer has read the last chunk's staging
		if (pend) { // no round came (a fallback or an empty step): flush before the staging is reused
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			for (int i = l; i < C * 64; i += 64)
				gbl(p.out)[pf0 + i] = so[i];
			pend = false;
		}
		if constexpr (FILL) {
			if (fpend) { // no round came: the fields leave before the scalars are reused
				lpf_store_fields(fp, fa, fb, fv);
				fpend = false;
			}
		}
		if (first < p.n) {
			const uint32_t r = fold16(acc) + (0xffffu - fold16(corr));
			Res res;
			if constexpr (MIXED) {
				res = lpwx_result(p, cur, fold16(r), fam, h, h6);
				if (p.bad) { // the fill variant's scheme: step totals, added once at the end
					nbad_ip += (uint32_t)__popcll(__ballot(cur.ok && (res.verdict & CGCK_BAD_IP)));
					nbad_l4 += (uint32_t)__popcll(__ballot(cur.ok && (res.verdict & CGCK_BAD_L4)));
				}
			} else if constexpr (IP6) {
				res = result6(p, cur.a0, cur.len, fold16(r), h6, cur.ok);
			} else if constexpr (FILL) {
				// result() without its stores and atomics: the fields are
				// stored by lpf_store_fields (its own conditions, below), the
				// counters summed per step
				KParams pq = p;
				pq.flags = p.flags & ~(uint32_t)CGCK_STORE;
				pq.bad = nullptr;
				res = result(pq, cur.a0, cur.len, fold16(r), h);
				const int hl = (int)h.hd * 4;
				const bool st = cur.ok && (p.flags & CGCK_STORE) && !(p.flags & CGCK_RAW) && cur.len >= 20 &&
						cur.len >= hl;
				fp = (st && (p.flags & CGCK_IP) ? 1u : 0u) | (st && (p.flags & CGCK_L4) && h.fo >= 0 ? 2u : 0u);
				fa = cur.a0 + 10;
				fb = cur.a0 + (uint64_t)(hl + (h.fo >= 0 ? h.fo : 0));
				fv = res.out;
				fpend = __any(fp != 0);
				if (!CGCK_LPF_DEFER && fpend) {
					lpf_store_fields(fp, fa, fb, fv);
					fpend = false;
				}
				if (p.bad) {
					nbad_ip += (uint32_t)__popcll(__ballot(cur.ok && (res.verdict & CGCK_BAD_IP)));
					nbad_l4 += (uint32_t)__popcll(__ballot(cur.ok && (res.verdict & CGCK_BAD_L4)));
				}
			} else
				res = result(p, cur.a0, cur.len, fold16(r), h);
			const int slot = (int)(j % C) * 64 + l;
			so[slot] = res.out;
			if (p.verdict) // (the verdict staging is allocated only with verdicts)
				sv[slot] = (uint8_t)res.verdict;
		}
		if (W && (j + 1) % C == 0) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the chunk's outputs are in LDS
			wg_barrier();                                      // H: hand them to the writer
		} else if (!W && ((j + 1) % C == 0 || j + 1 == nsteps) && p.contig != 5) { // lab mode 5: no flush
			// flush the chunk's outputs (packets [f0, f0 + 64 C) of the batch)
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
	}
	if constexpr (FILL) {
		if (fpend) // the last step's fields
			lpf_store_fields(fp, fa, fb, fv);
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	if constexpr (FILL || MIXED) {
		// the running counters: one vector atomic per non-zero total
		if (p.bad && l == 0) {
			if (nbad_ip)
				atomicAdd(p.bad + 0, nbad_ip);
			if (nbad_l4)
				atomicAdd(p.bad + 1, nbad_l4);
		}
	}
}
