// cgck_internal.h — shared between the kernels and the host C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgck_params.h" // KParams, the flag bits, enum Family, the measured defaults
#include "cgck_route.h"  // the burst server's constants and routing predicates

// Run-time A/B knobs ($CGCK_KERNEL, $CGCK_LPW_WPC, ...) exist only in the lab
// build (libcgck_lab.so, -DCGCK_LAB): there CGCK_ENV reads the environment;
// in the product library it is a null pointer, so every knob takes its
// measured default and its name is not even in the binary.  $CGCK_DEVICE
// (the drop-in symbols' device) is the product's one environment variable.
#if CGCK_LAB
#include <stdlib.h>
#define CGCK_ENV(name) getenv(name)
#else
#define CGCK_ENV(name) ((const char *)nullptr)
#endif

namespace cgck {

constexpr uint32_t kImixCycleBytes = 4252; // 7*64 + 4*576 + 1500

// Zeroed device bytes per context: 64 lines of 64 B, so dummy loads can be
// spread over L2 channels instead of all hitting one line.
constexpr uint32_t kZeroBytes = 64 * 64;

// Mailbox of the burst server (cgck_group.hip), in host-coherent pinned
// memory.  Two request slots, so one request can be in flight while the host
// posts the next (the pipelined RX / TX windows): request seq lives in slot
// seq & 1 — its block at stage + (seq & 1) * cap, its outputs at resp +
// (seq & 1) * burst_resp_slot(max_pkts), its mailbox word req[seq & 1] =
// seq | n << 32, stored (release) after the block.  Seqs run 1, 2, ... by
// burst_next (never 0, parity alternating through the wrap), and the server
// serves them strictly in that order: its leader workgroup polls the slot of
// the seq after the last it served and relays each request to the others
// through device memory, so each learns the packet count, and with it its
// share, from its poll.  Workgroup j of the W = burst_wgs(n, K) that serve a
// request answers with done[j] = seq (release) once its outputs are visible;
// a workgroup that refuses its slice (burst_hdr_ok / desc_inside) first
// stores refused[seq & 1] = seq.
// (kBurstMaxWG, kBurstOneWG, kBurstPerWG, burst_wgs, kBurstFirst: cgck_route.h)
struct BurstBox {
	uint64_t req[2];     // host -> device: seq | n << 32 of the request in slot seq & 1
	uint32_t stop;       // host -> device: exit now
	uint32_t bad_req;    // device -> host: slices refused by the server's checks (a count)
	uint64_t idle_ticks; // 100 MHz ticks without a request before the server exits
	uint32_t refused[2]; // device -> host: seq of the last refused request in each slot
	uint64_t lab_cyc;    // lab build: workgroup 0's shader clocks (s_memtime) over the compute phase
	uint64_t lab_body;   // lab build: thread 0's shader clocks over the one-workgroup body call alone
	uint32_t pad[2];
	uint32_t done[kBurstMaxWG]; // device -> host: the last request workgroup j served
	uint8_t alive[kBurstMaxWG]; // host sets 1 at launch; workgroup j clears its byte on exit
	uint64_t lab_t[4];   // lab build: workgroup 0's s_memrealtime at seen / read / computed / published
};
static_assert(sizeof(BurstBox) == 64 + 5 * kBurstMaxWG + 32, "mailbox line, the done lines, the alive lines, lab");

// The seq after s: 1, 2, ..., 0xfffffffe, 1, ...: never 0 (the relay's
// "nothing posted"), and s & 1 alternates through the wrap.
__host__ __device__ constexpr uint32_t burst_next(uint32_t s) { return s >= 0xfffffffeu ? 1u : s + 1u; }

// Header of a request block (the first 64 bytes of the burst staging), then
// the n descriptors at d_off = 64, then (base == 0) the packet bytes.  A
// request served by one workgroup is copied into device scratch with one wide
// read of the block's first kBurstFirst bytes — every thread's loads in
// flight together, one host round trip for a small request's header,
// descriptors and packet bytes — and the rest of a larger block in a second
// pass.  Workgroup j of a wider request reads the header and its own slice of
// the descriptors in one round trip and the packet bytes where they lie.
struct BurstReq {
	uint32_t n;       // packets
	uint32_t flags;   // CGCK_* flags
	uint32_t max_len; // longest ip_len (picks the lane shape)
	uint32_t bytes;   // size of the request block, this header included
	uint64_t base;    // device view of packets read in place (registered memory); 0: in the block
	uint32_t d_off;   // descriptors: offset in the block
	uint32_t p_off;   // packet bytes (base == 0): offset in the block
	uint64_t range;   // base != 0: bytes readable from base; the server refuses a descriptor past it
	uint32_t n1;      // 0 < n1 < n: descriptors [n1, n) take flags2 (a receive burst and a TX
	uint32_t flags2;  // fill sharing one request); 0: every descriptor takes flags
	uint32_t pad[4];
};
static_assert(sizeof(BurstReq) == kBurstReqBytes, "one header line");

// Outputs of a server request of n packets, host-coherent and packed by n
// (not by the server's capacity), so a small request's outputs share one
// page: [out u32 x n | meta u32 x n | verdict u8 x n], each part 64-byte
// aligned.  (With the verdicts at a capacity-sized offset, 16 KiB away, a
// one-packet request took 36.8 us instead of 9.5: tools/txburst dropin.)
__host__ __device__ constexpr uint32_t burst_meta_off(uint32_t n) { return (4 * n + 63) & ~63u; }
__host__ __device__ constexpr uint32_t burst_ver_off(uint32_t n) { return 2 * burst_meta_off(n); }
// Bytes of one slot's outputs for requests of up to max_pkts packets.
__host__ __device__ constexpr uint32_t burst_resp_slot(uint32_t max_pkts)
{
	return (burst_ver_off(max_pkts) + max_pkts + 63) & ~63u;
}
// req: slot 0's block (slot 1's at req + cap); resp: slot 0's outputs (slot
// 1's at resp + burst_resp_slot(max_pkts)); dcmd: 24 bytes of uncached device
// memory, the leader's relay words (one per slot, then the exit word), zeroed
// here on the launch stream before the launch; start_seq: the last request
// completed (the server serves burst_next(start_seq) first); epoch: nonzero,
// new for every launch; opts: lab A/B bits (0 in the product).
// door: the two mailbox words the leader polls (box->req in host memory, or
// the device-memory doorbell the host writes through the large BAR); stopw:
// the stop word it polls with them (box->stop, or beside the doorbell); vblk:
// the device-memory request slots of small blocks (kBurstFirst bytes each,
// nullptr: none), used by a request whose mailbox word has kBurstVram set in
// its count.
hipError_t launch_burst_server(BurstBox *box, const uint64_t *door, const uint32_t *stopw, const uint8_t *req,
			       const uint8_t *vblk, uint8_t *scratch, uint8_t *resp, uint64_t *dcmd, const void *zero,
			       uint32_t cap, uint32_t max_pkts, uint32_t wgs, uint32_t per_wg, uint32_t start_seq,
			       uint32_t epoch, uint32_t opts, hipStream_t st);
// In the mailbox word's count (bits 32-63): the request's block is in the
// device-memory slot (vblk) of its parity, not in the host staging.
constexpr uint32_t kBurstVram = 1u << 31;

// Batched Toeplitz hash over dense 12-byte tuples: 0 two-group loop, 2 A/B
// pipelined (cgck_rss.hip).
constexpr int kDefaultRssVariant = 2;

// Toeplitz RSS hash (cgck_rss.hip; subr.c:482-530).  `tab` = cnt x 256 u32
// byte tables derived from the key on the host (rss_tables in cgck_api.cpp).
constexpr uint32_t kRssLdsMaxCnt = 36; // tables up to 36 KiB are staged in LDS
// launch_toeplitz's geometry (cgck_test_rss_pass reports it from the same names):
constexpr int kRssPassBlocksPerCu = 8; // toeplitz_kernel: at most this many 256-record blocks per CU, then it strides
constexpr int kRssX4BlocksPerCu = 1;   // toeplitz12x4_ab_kernel: blocks per CU
constexpr int kRssX4Depth = 12;        // and 4-record groups per lane in its register ring

struct RssParams {
	const uint8_t *data;
	uint64_t n;
	uint64_t stride;
	uint32_t cnt;
	uint32_t mask;
	const uint32_t *tab;
	uint32_t *out;
};

// dst-cache build (cgck_rss.hip; con-gen.c:291-360).
struct DstParams {
	uint32_t laddr_min, faddr_min;
	uint32_t nf;             // faddr count (t_ip_faddr_max - t_ip_faddr_min + 1), nonzero
	uint32_t n;              // tuple count, u32 as con-gen.c:314-315 computes it
	uint32_t q64, r64;       // 64 / nf, 64 % nf
	uint32_t fport_be;       // t_port as stored (network order)
	uint32_t hconst;         // the fport bytes' share of the hash
	uint32_t filter;         // RSS filter on (con-gen.c:337)
	uint32_t cap;            // t_dst_cache_size (> 0)
	uint32_t ntiles;         // ceil(n / (256 * iters))
	uint32_t iters;          // per-wave iterations of 64 tuples per tile (dst_iters)
	uint64_t pass_lo, pass_hi; // bit h set: (h % t_rss_queue_num) == t_rss_queue_id, h in 0..127
	const uint32_t *tab;     // 12 x 256 byte tables of the key
	void *out;               // cgck_dst_entry_t[cap]
	uint32_t *ctl;           // [0] ticket, [1] done, [2] timeout; zeroed per launch
	uint32_t *count;         // entries written (con-gen.c:356); set by the kernel when n > 0
	uint64_t *status;        // one look-back word per tile; zeroed per launch
};

// Per-frame hash of a receive burst (cgck_rssf.hip; include/cgck.h, section 3).
// desc != nullptr: descriptors, else frame k at base + k * stride + l3_off with
// ip_len bytes.  `tab` = the 36 x 256 byte tables; `zero` = the context's zero
// chunk (loads of lanes without a frame byte to read).
struct RssfParams {
	const uint8_t *base;
	const void *desc;
	uint64_t n;
	uint64_t stride;
	uint32_t l3_off, ip_len;
	uint32_t mask, hf, queue_num;
	const uint32_t *tab;
	const void *zero;
	uint32_t *hash;
	uint8_t *kind;
	uint8_t *queue;
	uint32_t *qcount;
};

// Stable partition of a burst by queue id (cgck_steer.hip; include/cgck.h,
// section 3).  tile and tiles are steer_plan()'s (cgck_steer_plan.h); hist is the
// caller's workspace, u32[queue_num + 1][tiles], unused with one tile; nbits
// (the bits of a bin) and per_wave (frames per wave of a tile) are set by
// launch_steer.
struct SteerParams {
	const uint8_t *queue;
	uint64_t n;
	uint32_t queue_num;
	uint32_t tile, tiles;
	uint32_t nbits, per_wave;
	const void *desc_in;
	uint32_t *qoff;
	uint32_t *perm;
	uint32_t *slot;
	void *desc_out;
	uint32_t *hist;
};

// Classify and trim a raw Ethernet burst (cgck_l2d.hip; include/cgck.h, section
// 3).  raw: the transport's descriptors; `zero` = the context's zero chunk; each
// output may be nullptr.
struct L2dParams {
	const uint8_t *base;
	const void *raw;
	uint64_t n;
	const void *zero;
	void *desc_out;
	uint8_t *cls;
	uint32_t *count;
};

hipError_t launch_l2d(const L2dParams &p, int num_cus, hipStream_t st);

// Per-frame TCP / UDP segment records (cgck_l4d.hip; include/cgck.h, section 3).
// desc: the burst's descriptors; `zero` = the context's zero chunk; each output
// may be nullptr.
struct L4dParams {
	const uint8_t *base;
	const void *desc;
	uint64_t n;
	const void *zero;
	void *seg;
	uint8_t *cls;
	uint32_t *hash;
	uint32_t *count;
};

// Frames from segment records (cgck_l4b.hip; include/cgck.h, section 3).  slot:
// where the frames go; cls, fidx and each output may be nullptr.
struct L4bParams {
	uint8_t *base;
	const void *slot;
	const void *seg;
	const uint8_t *cls;
	const void *flow;
	const uint32_t *fidx;
	uint64_t n;
	uint32_t nflow;
	uint32_t ip_id0, ip_off;
	void *raw_out;
	void *desc_out;
	uint8_t *cls_out;
	uint32_t *count;
};

// Per-frame connection lookup (cgck_pcb.hip; include/cgck.h, section 3).  PcbTable
// is what the build and the lookup share: the caller's arrays, the table, mask =
// pcb_slots(nconn) - 1 (cgck_pcb_probe.h) and chain, cgck_test_pcb_mode's bit 0.
struct PcbTable {
	const void *conn;
	const void *flow;
	void *table;
	uint32_t nconn, nflow;
	uint32_t mask, chain;
};

struct PcbbParams {
	PcbTable t;
	uint32_t *stat; // zeroed by the launcher; may be nullptr
};

// desc, seg: the burst; cls and bound may be nullptr, and each output.
struct PcblParams {
	const uint8_t *base;
	const void *desc;
	const void *seg;
	const uint8_t *cls;
	uint64_t n;
	const void *zero;
	PcbTable t;
	const uint32_t *bound;
	uint32_t *idx;
	uint32_t *fidx;
	uint8_t *kind;
	uint32_t *count;
};

// tagged: 8-byte slots {idx, tag} (pcbb_kernel<true>, pcbl_kernel<.., true>), else
// 4-byte slots of the index alone.  launch_pcbb initialises the table and stat.
hipError_t launch_pcbb(const PcbbParams &p, bool tagged, hipStream_t st);
hipError_t launch_pcbl(const PcblParams &p, bool tagged, int num_cus, hipStream_t st);

// tcp_respond's RSTs for a burst (cgck_l4r.hip; include/cgck.h, section 3).  desc,
// seg: the burst; the four selectors, at and each output may be nullptr.  link: the
// first four dwords of the caller's flow template (MACs, vlan_tci, flags, ttl).
struct L4rParams {
	const uint8_t *base;
	const void *desc;
	const void *seg;
	const uint8_t *cls, *kind, *verdict, *l2cls;
	const uint32_t *at;
	uint64_t n;
	const void *zero;
	uint32_t link[4];
	uint32_t vmask, flags;
	void *seg_out;
	void *flow_out;
	uint8_t *cls_out;
	uint8_t *queue;
	uint32_t *count;
};

// turned: under `at`, seg and flow leave turned through LDS (l4r_kernel<.., 2>), else
// from their own lanes (<.., 1>); without `at` they always leave turned (<.., 0>).
hipError_t launch_l4r(const L4rParams &p, bool turned, int num_cus, hipStream_t st);

// Frames that the workgroups one launch of rssf_kernel, l2d_kernel, l4d_kernel,
// l4b_kernel, pcbl_kernel or l4r_kernel runs at most cover per pass (cgck_frame.h).
uint64_t frame_pass_frames(int num_cus);
hipError_t launch_l4d(const L4dParams &p, int num_cus, hipStream_t st);
// turned: the header's whole 16-byte granules leave through LDS (l4b_kernel<.., true>)
hipError_t launch_l4b(const L4bParams &p, bool turned, int num_cus, hipStream_t st);
// Rules 1 to 3 and the header lengths of cgck_l4_build from a flow's flags, a class
// byte and a seg's opt (cgck_l4_build_hdr_bytes): h | iph << 8 | l4h << 16, or 0
// when the frame is refused.
constexpr uint32_t l4b_lengths(uint32_t flow_flags, uint32_t cls, uint32_t opt)
{
	const uint32_t c = cls & 15u;
	if (c > 1u || (flow_flags & ~3u) != 0 || (c == 0 && (opt & ~7u) != 0))
		return 0;
	const uint32_t h = (flow_flags & 2u) ? 18u : 14u, iph = (flow_flags & 1u) ? 40u : 20u;
	const uint32_t l4h = c == 1u ? 8u : 20u + 4u * (opt & 1u) + 2u * (opt & 2u) + 3u * (opt & 4u);
	return h | iph << 8 | l4h << 16;
}
hipError_t launch_rssf(const RssfParams &p, int num_cus, hipStream_t st);
hipError_t launch_steer(const SteerParams &p, hipStream_t st);
hipError_t launch_toeplitz(const RssParams &p, int num_cus, hipStream_t st);
hipError_t launch_dst_cache(const DstParams &p, int num_cus, hipStream_t st);
uint32_t dst_iters(uint32_t n, uint32_t cap, bool filter, uint64_t pass_lo, uint64_t pass_hi, int num_cus);

hipError_t launch_cksum(const KParams &p, uint32_t len_hint, int num_cus, int kernel, hipStream_t st);

// The kernel a launcher just launched, by the name rocprofv3 reports (without
// namespace and argument list); cgck_ctx_last_kernel reads it back.  Each
// launch site interns its name once (CGCK_NOTE_KERNEL) and stores the pointer.
extern thread_local const char *t_kernel;
const char *intern(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define CGCK_NOTE_KERNEL(...)                                                   \
	do {                                                                    \
		static const char *const note_ = ::cgck::intern(__VA_ARGS__);    \
		::cgck::t_kernel = note_;                                       \
	} while (0)
constexpr const char *tf(bool b) { return b ? "true" : "false"; }
hipError_t launch_synth_fill(uint8_t *base, uint64_t nbytes, uint64_t seed, int num_cus, hipStream_t st);
hipError_t launch_synth_stamp(uint8_t *base, uint64_t n, uint64_t stride, uint32_t len, int num_cus,
			      hipStream_t st);
hipError_t launch_synth_stamp6(uint8_t *base, uint64_t n, uint64_t stride, uint32_t len, uint32_t nh, int num_cus,
			       hipStream_t st);
hipError_t launch_probe_read(const void *src, uint64_t bytes, uint32_t *sink, int num_cus, int variant,
			     hipStream_t st);
hipError_t launch_synth_imix(uint8_t *base, uint32_t *desc, uint64_t n, int num_cus, hipStream_t st);
hipError_t launch_synth_ring(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off, int num_cus,
			     hipStream_t st);
hipError_t launch_synth_imix6(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off,
			      uint32_t nh, int num_cus, hipStream_t st);
hipError_t launch_synth_dual(uint8_t *base, uint32_t *desc, uint64_t n, uint64_t stride, uint32_t l3_off, int num_cus,
			     hipStream_t st);
// cgck_synth_eth: flag |= 1 when a descriptor's l3_off is below 18; then the framing.
hipError_t launch_synth_eth_check(const uint32_t *desc, uint64_t n, uint32_t *flag, int num_cus, hipStream_t st);
hipError_t launch_synth_eth(uint8_t *base, const uint32_t *desc, uint32_t *raw, uint64_t n, uint32_t vlan_every,
			    uint64_t seed, int num_cus, hipStream_t st);

} // namespace cgck
