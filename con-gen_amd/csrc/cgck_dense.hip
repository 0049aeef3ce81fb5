// cgck_dense.hip — dense strided batches of large frames (the 1500 B config)
// streamed through LDS by DMA: dstr_kernel.
//
// What round 2 measured first (profiles/r02/dma/str*, lpd/): the LDS-DMA
// read alone reaches 88 % of 8 TB/s once the grid sweeps one window of the
// batch, against the register-load ceiling (78-81 %) the group kernel sits
// on, but the first stream kernel (cgck_stream.hip, lab) lost that with its
// consumer (78.8 % vs group 81.7 %).  Its pipeline drained at every window
// end (vmcnt(0) before a per-window output flush, then a fresh prologue),
// and its reduce ran the chunk corrections and the header in exec-masked
// branches.  This kernel keeps lpd_kernel's structure, which does pay at
// 64 B (cgck_lane.hip):
//
//  * A step = 4 consecutive frames: the chunks from the first frame's
//    16-byte-aligned start to the fourth frame's last chunk (<= 6 KiB when
//    stride, ip_len <= 1520), moved by 6 contiguous 1 KiB
//    global_load_lds_dwordx4 ... nt into a ring of D slots of the wave (one
//    wave per workgroup).  Lanes past the step's last chunk read the zero
//    line, so the only bytes read twice are one shared chunk per step.  A
//    step's slot is refilled as soon as its bytes are in registers, before
//    the reduce, so D steps are in flight through the arithmetic too.
//  * Steps come in chunks of C, chunks grid-interleaved (wave b takes chunks
//    b, b + G, ...): the grid sweeps one window of the batch.  The ring runs
//    across chunk boundaries without a drain: a chunk's 4C outputs are
//    staged in LDS and leave as ONE 16-byte store per lane (sc1) while the
//    next steps' DMA is in flight; the counted vmcnt for step j includes that
//    store when it was issued after step j's DMA.
//  * The reduce is branch-free per lane: lane (g = lane / 16, gl) sums region
//    chunks c0_g + 16 s + gl, s = 0..5, of frame g (chunks past the frame
//    select 0), and the group's lane 0 subtracts the bytes of its first chunk
//    before the frame (dword-aligned frames: whole dwords) and of its last
//    chunk after it (read once more from LDS as a broadcast).  The header
//    words are broadcast reads; every lane computes the frame's result (the
//    cost is per wave either way) and lane 0 of the group stages it.
//
//  * A step's geometry is the same for every step (base, stride multiples of
//    4 and steps of 4 frames: the step's start keeps base & 15), so the
//    lanes' slot offsets and selects are computed once per wave, and while
//    the step to issue is full (four live frames) its six DMAs are one asm
//    statement off a scalar cursor, in a loop of its own per number of whole
//    KiBs; the general issue() serves a wave's last steps
//    (cgck_dense_kernel.inc, profiles/dstr_geom/).
//
// Scope (dstr_ok): strided batches, base / stride / l3_off multiples of 4,
// 20 <= ip_len <= 1520, stride <= 1520, flags RAW or any of IP / L4 /
// L4_NOPSEUDO (no field zeroing, verify or in-place store), an output array
// (16-byte aligned), optional verdicts (BAD_LEN only, with these flags) and
// no bad counters.  Everything else takes cgck_group.hip.
// Arithmetic: subr.c:127-223 as restated in cgck_device.h (one's-complement
// sums of 16-bit words in any order, folded; reduce's 0 -> 0xFFFF).
#include "cgck_device.h"

#include <stdlib.h>

namespace cgck {

#define CGCK_DSTR_KERNEL dstr_kernel
#define CGCK_DSTR_IP6 false
#include "cgck_dense_kernel.inc"
#undef CGCK_DSTR_KERNEL
#undef CGCK_DSTR_IP6

hipError_t launch_dstr6(const KParams &p, unsigned blocks, hipStream_t st);

#if CGCK_LAB
static int env_int(const char *name, int dflt)
{
	const char *e = getenv(name);
	return e && *e ? atoi(e) : dflt;
}
#endif

hipError_t launch_dstr(const KParams &p, int num_cus, hipStream_t st)
{
	KParams q = p;
	q.contig = 0;
#if CGCK_LAB
	// $CGCK_DSTR_D (ring slots 2 | 3 | 4), $CGCK_DSTR_C (steps per chunk 8 |
	// 16 | 32), $CGCK_DSTR_W (1: the writer wave), $CGCK_DSTR_F (frames per
	// chunk the writer reads by register loads: 0 | 4 | 8), $CGCK_DSTR_WPC (workgroups
	// per CU), $CGCK_DSTR_MODE (2 no output flush, 3 the DMA alone; results
	// then undefined; 6 a barrier per step in both waves): A/B knobs of the
	// lab build, read once
	static const int D = env_int("CGCK_DSTR_D", 3), C = env_int("CGCK_DSTR_C", 16),
			 Wr = env_int("CGCK_DSTR_W", 1), wpc = env_int("CGCK_DSTR_WPC", 8),
			 Fr = env_int("CGCK_DSTR_F", 0);
	static const int mode = env_int("CGCK_DSTR_MODE", 0);
	q.contig = mode;
	const uint64_t NC = (p.n + 4 * C + Fr - 1) / (4 * C + Fr);
	const uint64_t waves = (uint64_t)num_cus * wpc;
	const dim3 g((unsigned)(NC < waves ? NC : waves));
#define CGCK_DSTR(DD, CC, WW, FF)                                                                       \
	if (D == DD && C == CC && (Wr == 1 || p.verdict) == WW && Fr == FF) {                           \
		CGCK_NOTE_KERNEL("dstr_kernel<%d, %d, %s, %d>", DD, CC, tf(WW), FF);                     \
		hipLaunchKernelGGL((dstr_kernel<DD, CC, WW, FF>), g, dim3((WW) ? 128 : 64),               \
				   (DD) * kDsSlot + ((WW) ? 64 : 16) * (CC), st, q);                        \
		return hipGetLastError();                                                               \
	}
	if (!(p.flags & CGCK_IP6)) { // (the IPv6 variant has the product shape only)
		CGCK_DSTR(3, 16, true, 4) CGCK_DSTR(3, 16, true, 8) CGCK_DSTR(3, 32, true, 8) CGCK_DSTR(3, 32, true, 4)
		CGCK_DSTR(3, 32, true, 0) CGCK_DSTR(3, 8, true, 0) CGCK_DSTR(2, 32, true, 0) CGCK_DSTR(4, 16, true, 0)
		CGCK_DSTR(3, 16, false, 0) CGCK_DSTR(3, 32, false, 0) CGCK_DSTR(2, 32, false, 0)
	}
#undef CGCK_DSTR
#else
	// 8 workgroups (a reducing wave + the writer wave) per CU: 19 KiB of LDS
	// each (three 6 KiB slots + two chunks of staged sums)
	const uint64_t NC = (p.n + 63) / 64;
	const uint64_t waves = (uint64_t)num_cus * 8;
	const dim3 g((unsigned)(NC < waves ? NC : waves));
#endif
	if (p.flags & CGCK_IP6) // the product shape only (cgck_dense6.hip)
		return launch_dstr6(q, g.x, st);
	CGCK_NOTE_KERNEL("dstr_kernel<3, 16, true, 0>");
	hipLaunchKernelGGL((dstr_kernel<3, 16, true, 0>), g, dim3(128), 3 * kDsSlot + 64 * 16, st, q);
	return hipGetLastError();
}

} // namespace cgck
