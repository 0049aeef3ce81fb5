// cgck_dense_kernel.inc - the text of dstr_kernel (cgck_dense.hip explains
// it), compiled as dstr_kernel there (CGCK_DSTR_IP6 false, IPv4) and as
// dstr6_kernel in cgck_dense6.hip (true, CGCK_IP6).  Two kernels from one
// text, each in a translation unit of its own: the IPv4 kernel then compiles
// to exactly the code it had before the IPv6 variant existed (a shared
// inlined body, and a second instantiation in its module, each changed it).

constexpr int kDsS = 6;                     // DMA instructions (KiB) per step
constexpr uint32_t kDsSlot = kDsS * 1024;   // bytes per ring slot
constexpr int kDsChunks = kDsS * 64;        // 16-byte chunks per slot
// Every chunk a lane of the reducing wave reads lies in its slot, so the
// reads need no clamp: frame g of a step starts at most 15 + 3 * 1520 bytes
// into the slot (dstr_ok: stride <= 1520), and a lane reads up to 95 chunks
// past the frame's first (16 s + gl).  (Unclamped: 1.004 of the clamped
// reads in one process, twice, bit-exact; profiles/r04/dstr_ab/.)
static_assert(((15 + 3 * 1520) >> 4) + 16 * (kDsS - 1) + 15 < kDsChunks, "a reducing lane's chunk lies in its slot");

// The six DMAs of a full step (four live frames) in ONE statement: M0 is
// saved and restored once and advanced by 1 KiB between the DMAs (the
// instruction's offset field is not used: what it does to the LDS side is
// not relied on), each write of M0 followed by its s_nop 0.  The step's
// aligned start `a` is wave-uniform (an SGPR pair), and of the step's span
// NW KiBs are whole for every lane: those take `a` as the scalar base and the
// lane's constant offset off[i] = 1024 i + 16 lane.  KiB NW is partial: `pa`
// is the lane's address, or the zero line past the step's last chunk.  The
// KiBs after it lie past the step and read the zero line (`z`, offset vz = 0).
// Always six DMAs, so the counted waits keep their meaning.  The opening
// s_nop 2 puts five wait states between whatever wrote `a` and the first DMA
// that reads it as its base.
#define CGCK_DS_OPEN "s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[slot]\n\ts_nop 2\n\t"
#define CGCK_DS_NEXT "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
#define CGCK_DS_W(i) "global_load_lds_dwordx4 %[o" #i "], %[a] nt\n\t" CGCK_DS_NEXT
#define CGCK_DS_P "global_load_lds_dwordx4 %[pa], off nt\n\t"
#define CGCK_DS_Z CGCK_DS_NEXT "global_load_lds_dwordx4 %[vz], %[z] nt\n\t"
#define CGCK_DS_ASM(body)                                                                               \
	asm volatile(CGCK_DS_OPEN body "s_mov_b32 m0, %[k]"                                              \
		     : [k] "=&s"(keep)                                                                   \
		     : [slot] "s"(slot), [a] "s"(a), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]), \
		       [o3] "v"(off[3]), [o4] "v"(off[4]), [pa] "v"(pa), [vz] "v"(vz), [z] "s"(z)        \
		     : "memory", "scc")
template <int NW>
__device__ __forceinline__ void dstr_issue_full(uint64_t a, uint32_t slot, const uint32_t (&off)[kDsS - 1], const void *pa,
						 const void *z, uint32_t vz)
{
	static_assert(NW >= 0 && NW < kDsS, "a step of four frames (<= 6091 bytes) has at most five whole KiBs");
	uint32_t keep;
	if constexpr (NW == 5)
		CGCK_DS_ASM(CGCK_DS_W(0) CGCK_DS_W(1) CGCK_DS_W(2) CGCK_DS_W(3) CGCK_DS_W(4) CGCK_DS_P);
	else if constexpr (NW == 4)
		CGCK_DS_ASM(CGCK_DS_W(0) CGCK_DS_W(1) CGCK_DS_W(2) CGCK_DS_W(3) CGCK_DS_P CGCK_DS_Z);
	else if constexpr (NW == 3)
		CGCK_DS_ASM(CGCK_DS_W(0) CGCK_DS_W(1) CGCK_DS_W(2) CGCK_DS_P CGCK_DS_Z CGCK_DS_Z);
	else if constexpr (NW == 2)
		CGCK_DS_ASM(CGCK_DS_W(0) CGCK_DS_W(1) CGCK_DS_P CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z);
	else if constexpr (NW == 1)
		CGCK_DS_ASM(CGCK_DS_W(0) CGCK_DS_P CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z);
	else
		CGCK_DS_ASM(CGCK_DS_P CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z CGCK_DS_Z);
}
#undef CGCK_DS_ASM
#undef CGCK_DS_Z
#undef CGCK_DS_P
#undef CGCK_DS_W
#undef CGCK_DS_NEXT
#undef CGCK_DS_OPEN

// IP6 (dstr6_kernel, CGCK_IP6): the same stream; the reducing wave stages
// the frame's sum, the sum of its first 8 bytes and byte 6, and the writer
// wave finishes with the no-extension identity (v6_dense, cgck_device.h): a
// frame with extension headers is finished exactly by the same lane from
// global memory, only slower.
template <int D, int C, bool W, int F>
__global__ __launch_bounds__(128) void CGCK_DSTR_KERNEL(KParams p)
{
	constexpr bool IP6 = CGCK_DSTR_IP6;
	static_assert(!IP6 || (W && F == 0), "the IPv6 variant is the product shape's: writer wave, no register frames");
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const int lane = threadIdx.x & 63, g = lane >> 4, gl = lane & 15;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t flags = p.flags;
	const bool raw = flags & CGCK_RAW;
	const int len = (int)p.ip_len;
	const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem);
	// staged outputs of a chunk (W: the sums of 2 chunks, 2 words a frame)
	uint32_t *so = reinterpret_cast<uint32_t *>(smem + D * kDsSlot);
	const uint8_t *zero = (const uint8_t *)p.zero + (blockIdx.x & 63) * 64;
	const uint64_t base = reinterpret_cast<uint64_t>(p.base) + p.l3_off;
	const uint64_t n = p.n, stride = p.stride;
	// Super-chunks of SC frames, grid-interleaved: the first 4C are wave 0's
	// C steps, the last F the writer wave's (W, F > 0: read by register loads
	// while it waits for wave 0's chunk, so more bytes are in flight per CU
	// than the LDS ring holds).
	constexpr uint32_t SC = 4 * C + F;
	const uint64_t NC = (n + SC - 1) / SC, G = gridDim.x, b = blockIdx.x;
	if (b >= NC)
		return;
	const uint32_t nsteps = (uint32_t)((NC - b + G - 1) / G * C);
#if CGCK_LAB
	const uint32_t mode = p.contig; // lab A/B modes (launch_dstr)
#else
	constexpr uint32_t mode = 0; // (the product launcher sets none: no test of it per step)
#endif
	auto cfirst = [&](uint32_t k) { return (b + (uint64_t)k * G) * SC; }; // chunk k's first frame

	// a frame's result from its folded sums (tot over the frame, ip over the
	// header, ps over src/dst), ip_hl and ip_p: result() of cgck_group.hip
	auto fin = [&](uint32_t tot, uint32_t ip, uint32_t ps, uint32_t hd, uint32_t proto) {
		const int hl = (int)hd * 4;
		uint32_t lo = 0, hi = 0;
		if (raw) {
			lo = finish(tot);
		} else if (len >= hl) { // else BAD_LEN: 0 | 0 << 16, as the group kernel
			if (flags & CGCK_IP)
				lo = finish(ip);
			if (flags & CGCK_L4) {
				uint32_t L = ocsub(tot, ip);
				if (!(flags & CGCK_L4_NOPSEUDO))
					L = fold16(L + ps + (proto << 8) + bswap16((uint32_t)(len - hl) & 0xffffu));
				hi = finish(L);
			}
		}
		return lo | (hi << 16);
	};

	// the outputs of chunk k (its 4C frames, staged at sb) to global memory
	auto flush = [&](uint32_t k, const uint32_t *sb) {
		const uint64_t first = cfirst(k);
		if (first + 4 * C <= n) {
			if (lane < C) { // one 16-byte store per lane
				const uint4 v4 = reinterpret_cast<const uint4 *>(sb)[lane];
				bstore16<kSc1>(out_rsrc(p.out + first, 16 * C), 16 * lane, u32x4_t{v4.x, v4.y, v4.z, v4.w});
			}
		} else { // the batch's last, partial chunk: per-frame stores
			for (int i = lane; i < 4 * C; i += 64)
				if (first + i < n)
					gbl(p.out)[first + i] = sb[i];
		}
	};

	// A frame read into registers by its 16 lanes (chunks c0 + 16 s + gl,
	// clamped): the same sums as wave 0 takes from LDS; lane 0 stores it.
	auto reg_frame = [&](uint64_t f, uint64_t a, int nch, const uint4 (&w)[kDsS]) __attribute__((always_inline)) {
		const int q = (int)(a & 15);
		uint32_t body = 0;
		uint4 tw = make_uint4(0, 0, 0, 0); // the frame's last chunk, in the lane holding it
		bool ht = false;
#pragma unroll
		for (int s2 = 0; s2 < kDsS; ++s2) {
			const int c = 16 * s2 + gl;
			body += c < nch ? sum4(w[s2], 0u) : 0u;
			const bool t = c == nch - 1;
			// opaque masks: a select chain over array elements would be turned
			// into a dynamically indexed (scratch) load
			const uint32_t mt = opaque(t ? ~0u : 0u);
			tw = make_uint4(pick(mt, w[s2].x, tw.x), pick(mt, w[s2].y, tw.y), pick(mt, w[s2].z, tw.z),
					pick(mt, w[s2].w, tw.w));
			ht = ht || t;
		}
		uint32_t corr = 0;
		if (gl == 0) { // the q bytes (whole dwords) before the frame
			corr = hsum(q >= 4 ? w[0].x : 0u, 0);
			corr = hsum(q >= 8 ? w[0].y : 0u, corr);
			corr = hsum(q >= 12 ? w[0].z : 0u, corr);
		}
		if (ht) { // the bytes of the last chunk after the frame
			const int e = q + len - 16 * (nch - 1);
			if ((len & 3) == 0) {
				corr = hsum(e <= 4 ? tw.y : 0u, corr);
				corr = hsum(e <= 8 ? tw.z : 0u, corr);
				corr = hsum(e <= 12 ? tw.w : 0u, corr);
			} else {
				corr = msum(tw, 0, e, 16, corr);
			}
		}
		uint32_t tot = fold16(body) + (0xffffu - fold16(corr));
		tot = fold16(gsum<16>(tot));
		// header dwords: chunk c0 (this lane) and c0 + 1 (lane gl + 1, DPP row_shl:1)
		const uint32_t n0 = __builtin_amdgcn_mov_dpp(w[0].x, 0x101, 0xF, 0xF, false);
		const uint32_t n1 = __builtin_amdgcn_mov_dpp(w[0].y, 0x101, 0xF, 0xF, false);
		const uint32_t n2 = __builtin_amdgcn_mov_dpp(w[0].z, 0x101, 0xF, 0xF, false);
		const uint32_t n3 = __builtin_amdgcn_mov_dpp(w[0].w, 0x101, 0xF, 0xF, false);
		const uint32_t d[8] = {w[0].x, w[0].y, w[0].z, w[0].w, n0, n1, n2, n3};
		const int q4 = q >> 2;
		const uint32_t m0 = opaque(q4 == 0 ? ~0u : 0u), m1 = opaque(q4 == 1 ? ~0u : 0u),
			       m2 = opaque(q4 == 2 ? ~0u : 0u);
		uint32_t h[5];
#pragma unroll
		for (int i = 0; i < 5; ++i)
			h[i] = pick(m0, d[i], pick(m1, d[i + 1], pick(m2, d[i + 2], d[i + 3])));
		const uint32_t hd = h[0] & 15;
		uint32_t ip = hsum(h[4], hsum(h[3], hsum(h[2], hsum(h[1], hsum(h[0], 0)))));
		if (gl == 0 && f < n) {
			if (hd != 5) { // options or a short header (rare): from global memory
				ip = 0;
				for (uint32_t i = 0; i < hd; ++i)
					ip = hsum(*gbl_at<const uint32_t>(a + 4 * i), ip);
			}
			const uint32_t r = fin(tot, fold16(ip), fold16(hsum(h[4], hsum(h[3], 0))), hd, (h[2] >> 8) & 0xffu);
			gbl(p.out)[f] = r;
			if (p.verdict)
				gbl(p.verdict)[f] = (uint8_t)(!raw && len < (int)hd * 4 ? CGCK_BAD_LEN : 0);
		}
	};

	if (W && wave == 1) {
		// The writer wave finishes and stores each chunk's frames, a lane per
		// frame, from the sums wave 0 staged: no store sits in the reducing
		// wave's vmcnt, where (in order) it would hold the wait for every
		// later step's DMA, and the per-frame finish leaves its VALU.  One
		// barrier per chunk (the staging is double-buffered: wave 0 refills a
		// buffer only after the next chunk's barrier, which this wave reaches
		// once it has read it); lab mode 6 adds wave 0's per-step barrier.
		for (uint32_t j = 0; j < nsteps; ++j) {
			if (mode == 6)
				wg_barrier();
			if ((j + 1) % C == 0) {
				const uint32_t k = j / C;
				// the chunk's F register frames: loads in flight across the wait
				uint4 rw[F > 0 ? F / 4 : 1][kDsS];
				uint64_t ra[F > 0 ? F / 4 : 1];
				int rn[F > 0 ? F / 4 : 1];
#pragma unroll
				for (int u = 0; u < F / 4; ++u) {
					const uint64_t f = cfirst(k) + 4 * C + 4 * u + g;
					ra[u] = base + (f < n ? f : 0) * stride;
					rn[u] = f < n ? (int)(((ra[u] & 15) + len + 15) >> 4) : 0;
					const uint4 *c0 = reinterpret_cast<const uint4 *>(ra[u] & ~(uint64_t)15);
#pragma unroll
					for (int s2 = 0; s2 < kDsS; ++s2)
						rw[u][s2] = ldc<true>(c0, 16 * s2 + gl, rn[u], p.zero);
				}
				wg_barrier(); // chunk j / C staged
				const uint32_t *sb = so + (k & 1) * 8 * C;
				const uint64_t first = cfirst(k);
				for (int i = lane; i < 4 * C; i += 64) {
					const uint32_t v0 = sb[i], v1 = sb[4 * C + i];
					const uint32_t hd = (v1 >> 16) & 15u;
					if constexpr (IP6) { // the frame's lane finishes it (v6_dense)
						uint32_t bl = 0;
						const uint32_t r6 = first + i < n ? v6_dense(base + (first + i) * stride, len, v0 & 0xffffu,
											     v0 >> 16, v1 >> 24, flags, &bl)
										  : 0u;
						if (p.verdict && first + i < n)
							gbl(p.verdict)[first + i] = (uint8_t)bl;
						if (first + 4 * C <= n)
							bstore4<kSc1>(out_rsrc(p.out + first, 16 * C), 4 * i, r6);
						else if (first + i < n)
							gbl(p.out)[first + i] = r6;
						continue;
					}
					const uint32_t r = fin(v0 & 0xffffu, v0 >> 16, v1 & 0xffffu, hd, v1 >> 24);
					if (p.verdict && first + i < n) // BAD_LEN, as the group kernel
						gbl(p.verdict)[first + i] = (uint8_t)(!raw && len < (int)hd * 4 ? CGCK_BAD_LEN : 0);
					if (first + 4 * C <= n)
						bstore4<kSc1>(out_rsrc(p.out + first, 16 * C), 4 * i, r);
					else if (first + i < n)
						gbl(p.out)[first + i] = r;
				}
#pragma unroll
				for (int u = 0; u < F / 4; ++u)
					reg_frame(cfirst(k) + 4 * C + 4 * u + g, ra[u], rn[u], rw[u]);
			}
		}
		return;
	}

	auto sfirst = [&](uint32_t j) { return cfirst(j / C) + 4 * (j % C); }; // step j's first frame
	auto issue = [&](uint32_t j) { // step j of this wave into slot j % D
		const uint64_t f0 = sfirst(j);
		const bool live = j < nsteps && f0 < n;
		const uint64_t fl = f0 + 3 < n ? f0 + 3 : n - 1;
		const uint64_t a = (base + f0 * stride) & ~(uint64_t)15;
		const uint64_t e = (base + fl * stride + len - 1) & ~(uint64_t)15; // the step's last chunk
		const uint32_t slot = lds0 + (j % D) * kDsSlot;
#pragma unroll
		for (int i = 0; i < kDsS; ++i) {
			const uint64_t s0 = a + 1024 * i, src = s0 + 16 * lane;
			if (live && s0 + 1008 <= e) // the whole KiB lies in the step (wave-uniform)
				glds16_nt(reinterpret_cast<const void *>(src), slot + 1024 * i);
			else
				glds16_nt(live && src <= e ? reinterpret_cast<const void *>(src) : zero, slot + 1024 * i);
		}
	};
	// The geometry of a step is the same for every step of every wave.
	// dstr_ok: base + l3_off and stride are multiples of 4.  Chunks start at
	// multiples of SC, steps at multiples of 4 inside them, so a step's first
	// frame f0 is a multiple of 4 and f0 * stride one of 16.  Hence
	// (base + f0 * stride) & 15 == base & 15 =: al, the step's aligned start
	// is a = base + f0 * stride - al, and frame g of the step lies al + g *
	// stride bytes into the slot whatever the step.  Everything a lane derives
	// from that (its chunk offsets in the slot, which dwords of its first and
	// last chunk lie outside the frame, which of its six chunks lie inside) is
	// computed here once, not per step, and the selects become multipliers of
	// the v_dot2 sums (hsum_sel) or masks: no multiply and no compare on them
	// remains in the loop.  (opaque: each value in a register of its own,
	// not re-derived in the loop.)
	static_assert(SC % 4 == 0, "a step's first frame is a multiple of 4");
	static_assert(D < C, "the prologue's steps lie in the first chunk");
	const int al = (int)(base & 15);
	const int o = al + g * (int)stride; // frame g's byte offset in the slot
	const int q = o & 15, c0 = o >> 4;
	const int nch = (q + len + 15) >> 4;
	const int e = q + len - 16 * (nch - 1); // bytes of the last chunk in the frame
	const uint32_t rd_w = opaque(16u * (uint32_t)(c0 + gl));      // the lane's chunks: + 256 s
	[[maybe_unused]] const uint32_t rd_t = opaque(16u * (uint32_t)(c0 + nch - 1)); // the frame's last chunk
	[[maybe_unused]] const uint32_t rd_h = opaque((uint32_t)o);                    // the header
	uint32_t bmul[kDsS]; // chunk s of the lane lies in the frame
#pragma unroll
	for (int s = 0; s < kDsS; ++s)
		bmul[s] = opaque(16 * s + gl < nch ? kHsumAll : 0u);
	// group lane 0: the q bytes (whole dwords) of the first chunk before the
	// frame, and the bytes of the last chunk after it (whole dwords when len is
	// a multiple of 4, else byte masks)
	const uint32_t lm1 = opaque(gl == 0 && q >= 4 ? kHsumAll : 0u), lm2 = opaque(gl == 0 && q >= 8 ? kHsumAll : 0u),
		       lm3 = opaque(gl == 0 && q >= 12 ? kHsumAll : 0u);
#if CGCK_DSTR_REGHDR
	const bool tl = true; // (the lane holding the last chunk, chosen per step)
#else
	const bool tl = gl == 0;
#endif
	const uint32_t tm0 = opaque(tl ? dmask(0, 0, e, 16) : 0u), tm1 = opaque(tl ? dmask(0, 1, e, 16) : 0u),
		       tm2 = opaque(tl ? dmask(0, 2, e, 16) : 0u), tm3 = opaque(tl ? dmask(0, 3, e, 16) : 0u);

	// A full step (four live frames) spans span + 16 bytes from its aligned
	// start, the same for every full step: nw of its KiBs are whole, KiB nw is
	// partial (lanes past the span read the zero line), the rest read the zero
	// line.  The first jfull steps of the wave are full: all of them, unless
	// its last chunk is the batch's last, partial one.
	const uint32_t span = ((uint32_t)al + 3 * (uint32_t)stride + (uint32_t)len - 1) & ~15u;
	const uint32_t nw = (span + 16) >> 10; // KiBs i with 1024 i + 1008 <= span: at most 5
	uint32_t off[kDsS - 1];
#pragma unroll
	for (int i = 0; i < kDsS - 1; ++i)
		off[i] = opaque(1024u * i + 16u * lane);
	const uint32_t poff = 1024 * nw + 16 * lane;
	const uint32_t pmask = opaque(poff <= span ? ~0u : 0u);
	const uint32_t vz = opaque(0u);
	const uint32_t klast = nsteps / C - 1;
	const uint64_t lrem = (n - cfirst(klast)) / 4;
	const uint32_t jfull = klast * C + (lrem < (uint64_t)C ? (uint32_t)lrem : (uint32_t)C);
	// the aligned start of the step to issue next (j + D), advanced by four
	// frames inside a chunk and by the jump to the wave's next chunk at its end
	const uint64_t step4 = 4 * stride, cjump = (G * SC - 4 * (C - 1)) * stride;
	uint64_t ia = base - (uint64_t)al + (cfirst(0) + 4 * D) * stride;
	uint32_t slot_off = 0; // (j % D) * kDsSlot

#pragma unroll
	for (int d = 0; d < D; ++d)
		issue(d);
	// One step.  NW >= 0: step j + D is full and has NW whole KiBs (the first
	// loop below); NW < 0: the general issue() (the wave's last steps, and the
	// refills past them).
	auto step = [&](uint32_t j, auto nwc) __attribute__((always_inline)) {
		constexpr int NW = decltype(nwc)::value;
		// Wait for step j's DMA.  Issued after it: the D - 1 later steps' DMA
		// and (without the writer wave) the last chunk flush's store when it
		// came after step j's DMA.
		if (!W && j >= (uint32_t)C && (j % C) <= (uint32_t)(D - 1))
			asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kDsS * (D - 1) + 1) : "memory");
		else
			asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kDsS * (D - 1)) : "memory");
		// The covering vmcnt alone orders this wave's own ds_reads behind its
		// LDS-DMA (MI355X_MICROARCH.md: a barrier is needed only for other
		// waves' reads), so no barrier per step.
		if (!W || mode == 6)
			wg_barrier();
		uint32_t *sc = so + (W ? ((j / C) & 1) * 8 * C : 0); // this chunk's staging
		auto refill = [&]() __attribute__((always_inline)) { // step j + D into the slot of step j
			if constexpr (NW >= 0) {
				const uint32_t slot = lds0 + slot_off;
				const uint64_t pl = ia + poff;
				const uint64_t zl = reinterpret_cast<uint64_t>(zero);
				const void *pa = reinterpret_cast<const void *>(
					(uint64_t)pick(pmask, (uint32_t)pl, (uint32_t)zl) |
					(uint64_t)pick(pmask, (uint32_t)(pl >> 32), (uint32_t)(zl >> 32)) << 32);
				dstr_issue_full<NW>(ia, slot, off, pa, zero, vz);
				ia += ((j + D + 1) % C) == 0 ? cjump : step4;
			} else {
				issue(j + D);
			}
		};
		if (mode == 3) { // lab: the DMA pipeline alone
			refill();
		} else {
			const uint8_t *sl = smem + slot_off;
			uint4 w[kDsS];
#pragma unroll
			for (int s = 0; s < kDsS; ++s)
				w[s] = *reinterpret_cast<const uint4 *>(sl + rd_w + 256 * s);
#if CGCK_DSTR_REGHDR
			// (lab A/B) only the six chunk reads before the refill: the last
			// chunk is the register of the lane holding it, the header dwords
			// come from w[0] of this lane and the next (DPP row_shl:1)
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			refill();
			const uint64_t f0 = sfirst(j);
			uint4 wt = make_uint4(0, 0, 0, 0);
			bool ht = false;
#pragma unroll
			for (int s = 0; s < kDsS; ++s) {
				const bool t = 16 * s + gl == nch - 1;
				const uint32_t mt = opaque(t ? ~0u : 0u);
				wt = make_uint4(pick(mt, w[s].x, wt.x), pick(mt, w[s].y, wt.y), pick(mt, w[s].z, wt.z),
						pick(mt, w[s].w, wt.w));
				ht = ht || t;
			}
			const uint32_t n0 = __builtin_amdgcn_mov_dpp(w[0].x, 0x101, 0xF, 0xF, false);
			const uint32_t n1 = __builtin_amdgcn_mov_dpp(w[0].y, 0x101, 0xF, 0xF, false);
			const uint32_t n2 = __builtin_amdgcn_mov_dpp(w[0].z, 0x101, 0xF, 0xF, false);
			const uint32_t n3 = __builtin_amdgcn_mov_dpp(w[0].w, 0x101, 0xF, 0xF, false);
			const uint32_t dd[8] = {w[0].x, w[0].y, w[0].z, w[0].w, n0, n1, n2, n3};
			const int q4 = q >> 2;
			const uint32_t m0 = opaque(q4 == 0 ? ~0u : 0u), m1 = opaque(q4 == 1 ? ~0u : 0u),
				       m2 = opaque(q4 == 2 ? ~0u : 0u);
			uint32_t hh[5];
#pragma unroll
			for (int i = 0; i < 5; ++i)
				hh[i] = pick(m0, dd[i], pick(m1, dd[i + 1], pick(m2, dd[i + 2], dd[i + 3])));
			const uint32_t h1 = hh[1], h2 = hh[2], h3 = hh[3], h4 = hh[4];
			const uint32_t hd = hh[0] & 15;
			uint32_t ip = IP6 ? hsum(h1, hsum(hh[0], 0)) : hsum(h4, hsum(h3, hsum(h2, hsum(h1, hsum(hh[0], 0)))));
			if (!IP6 && gl == 0 && hd != 5 && f0 + g < n) { // options or a short header (rare): global memory
				const uint64_t fa = base + (f0 + g) * stride;
				ip = 0;
				for (uint32_t i = 0; i < hd; ++i)
					ip = hsum(*gbl_at<const uint32_t>(fa + 4 * i), ip);
			}
#else
			const uint4 wt = *reinterpret_cast<const uint4 *>(sl + rd_t); // the last chunk
			const uint32_t *hw = reinterpret_cast<const uint32_t *>(sl + rd_h);
			const uint32_t h0 = hw[0], h1 = hw[1], h2 = hw[2], h3 = hw[3], h4 = hw[4];
			const uint32_t hd = h0 & 15;
			// (IP6: the sum of the first 8 bytes, which the L4 sum leaves out)
			uint32_t ip = IP6 ? hsum(h1, hsum(h0, 0)) : hsum(h4, hsum(h3, hsum(h2, hsum(h1, hsum(h0, 0)))));
			if (!IP6 && hd != 5) { // options or a short header (exec-masked, rare)
				ip = 0;
				for (uint32_t i = 0; i < hd; ++i)
					ip = hsum(hw[i], ip);
			}
			// The slot's bytes are in registers: refill it now, so D steps stay
			// in flight while this one is reduced.
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			refill();
#endif

			// independent per-chunk chains (no dependent v_dot2 wait states);
			// a chunk past the frame counts 0 by its multiplier
			uint32_t cs[kDsS];
#pragma unroll
			for (int s = 0; s < kDsS; ++s)
				cs[s] = sum4_sel(w[s], bmul[s], 0);
			uint32_t body = 0;
#pragma unroll
			for (int s = 0; s < kDsS; ++s)
				body += cs[s];
			// group lane 0 (the multipliers and masks are 0 in the other lanes):
			// the bytes of the first chunk before the frame and of the last
			// chunk after it
			const uint32_t lead = hsum_sel(w[0].z, lm3, hsum_sel(w[0].y, lm2, hsum_sel(w[0].x, lm1, 0)));
#if CGCK_DSTR_REGHDR
			const uint32_t tsel = ht ? ~0u : 0u;
#else
			constexpr uint32_t tsel = ~0u;
#endif
			const uint32_t tail = hsum(wt.w & tm3 & tsel, hsum(wt.z & tm2 & tsel, hsum(wt.y & tm1 & tsel, hsum(wt.x & tm0 & tsel, 0))));
			const uint32_t corr = lead + tail;
			uint32_t tot = fold16(body) + (0xffffu - fold16(corr));
			tot = fold16(gsum<16>(tot));

			const uint32_t proto = IP6 ? (h1 >> 16) & 0xffu : (h2 >> 8) & 0xffu; // IP6: nh, byte 6
			const uint32_t ps = fold16(hsum(h4, hsum(h3, 0)));
			if (W) { // the writer wave finishes: stage the sums
				if (gl == 0) {
					sc[4 * (j % C) + g] = tot | (fold16(ip) << 16);
					sc[4 * C + 4 * (j % C) + g] = ps | (hd << 16) | (proto << 24);
				}
			} else if (gl == 0) {
				sc[4 * (j % C) + g] = fin(tot, fold16(ip), ps, hd, proto);
			}
		}
		slot_off = slot_off + kDsSlot == D * kDsSlot ? 0 : slot_off + kDsSlot;
		if ((j + 1) % C == 0) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the chunk's outputs are in LDS
			if (W)
				wg_barrier(); // hand the chunk to the writer wave
			else if (mode != 2) // lab mode 2: no output flush
				flush(j / C, sc);
		}
	};
	// The steps whose refill (step j + D) is full, then the rest.  Loops of
	// their own, so the first holds no general issue() (none of its 64-bit
	// multiplies, compares and branches), and one per nw, which never changes
	// during a launch, so it holds no test of nw either.
	const uint32_t jhot = (jfull > (uint32_t)D ? jfull : (uint32_t)D) - D;
	uint32_t j = 0;
	auto hot = [&](auto nwc) __attribute__((always_inline)) {
		for (; j < jhot; ++j)
			step(j, nwc);
	};
	switch (nw) {
	case 5: hot(std::integral_constant<int, 5>{}); break;
	case 4: hot(std::integral_constant<int, 4>{}); break;
	case 3: hot(std::integral_constant<int, 3>{}); break;
	case 2: hot(std::integral_constant<int, 2>{}); break;
	case 1: hot(std::integral_constant<int, 1>{}); break;
	default: hot(std::integral_constant<int, 0>{}); break;
	}
	for (; j < nsteps; ++j)
		step(j, std::integral_constant<int, -1>{});
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
