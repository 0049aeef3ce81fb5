// cgck_params.h — what the kernel choice (cgck_choose.cpp) reads: a batch's
// parameters, the internal flag bits, the kernel families, the measured
// defaults.  No HIP: <stdint.h> and the public header.  Part of cgck_internal.h.
#pragma once
#include <stdint.h>

#include "../../include/cgck.h"

#ifndef CGCK_LAB
#define CGCK_LAB 0 // 1: libcgck_lab.so
#endif
namespace cgck {

// Internal flag (never part of the public enum): skip the BAD_LEN rule so the
// drop-in udp_cksum keeps the pure-function semantics of subr.c:212-223 even
// for malformed headers.
constexpr uint32_t kFlagNoLenCheck = 1u << 15;
// Internal flag of the RX window (cgck_rx_begin): the L4 result of each
// packet follows its own protocol, as the stack's verifiers do — ICMP (ip_p 1)
// is in_cksum(ip + hl, len - hl) with its field at +2 (ip_icmp.c:187-189),
// everything else udp_cksum with the pseudo-header (tcp_input.c:75-78,
// udp_usrreq.c:86-89).  Group kernel only.
constexpr uint32_t kFlagL4Auto = 1u << 14;
// Internal flag of the RX window: descriptor ip_len is the bytes the frame
// holds after l3_off (ip_input's `len`); the group kernel itself decides, as
// cgck_rx_begin's host walk used to, which calls the stack can make on the
// frame (ip_input.c:28-44, 76; tcp_input.c:67; udp_usrreq.c:65;
// ip_icmp.c:177; gbtcp/inet.c:282-314) and covers min(ntohs(ip_len), len)
// bytes.  Per frame it writes KParams.meta: kRxOkIp | kRxOkL4 | kRxIcmp,
// ip_hl * 4 in bits 8-15, ntohs(ip_len) - ip_hl * 4 in bits 16-31.
constexpr uint32_t kFlagRx = 1u << 13;
constexpr uint32_t kRxOkIp = 1, kRxOkL4 = 2, kRxIcmp = 4;
// Internal flag: a host-resident region bound by PCIe round trips (the
// drop-in symbols' one region): take the group kernel, whose one block reads
// the region at once, whatever the lane kernels' preconditions say (lpd for
// a 20-byte in_cksum read its DMA steps over the fabric: 31 vs 14 us).
constexpr uint32_t kFlagGroup = 1u << 12;

// The flag sets of the windows' requests (cgck_dropin.cpp): every frame of a
// receive burst (its meta word, both results by ip_p, fields read as zero),
// and a transmit fill's headers and segments (both fields read as zero;
// kFlagL4Auto too when the fill holds ICMP messages).  The burst server's
// one-workgroup body is compiled for each (burst_body_spec, cgck_group.hip).
constexpr uint32_t kRxFlags = CGCK_IP | CGCK_L4 | CGCK_ZERO_FIELDS | kFlagL4Auto | kFlagRx;
constexpr uint32_t kTxFlags = CGCK_IP | CGCK_L4 | CGCK_ZERO_FIELDS;

struct KParams {
	const uint8_t *base;
	const cgck_desc_t *desc; // nullptr: strided batch
	uint64_t n;
	uint64_t stride;
	uint32_t l3_off;
	uint32_t ip_len;
	uint32_t flags;
	uint32_t *out;
	uint8_t *verdict;
	uint32_t *bad;
	uint32_t contig; // set by the launcher: contiguous block ranges
	const void *zero; // kZeroBytes zero bytes of device memory (safe target for clamped loads)
	uint32_t *meta;   // kFlagRx only: one word per packet (see kFlagRx)
};

// Kernel families: cgck_ctx_set_kernel pins one by name; the lab build's
// $CGCK_KERNEL, tools/sweep.py, tools/probe.py and tools/lpd_check.py pass the
// numbers, so the values never move.  libcgck.so carries the families the
// automatic choice reaches; "lab" ones are compiled only into libcgck_lab.so
// (-DCGCK_LAB, tools/Makefile).  The rules over them: choose(), cgck_choose.cpp.
enum Family : int {
	kAuto = 0,   // the automatic choice; a pinned family this build lacks means the same
	kGroup = 1,  // G lanes per packet (cgck_group.hip): typical length >= 1 KiB where dstr does not
		     // apply, the drop-in and window calls (internal flags), the full IPv6 semantics
		     // (cksum6_kernel); what every batch another family refuses ends on
	kLpp = 2,    // lane per packet: small unaligned or descriptor packets (<= kLppUpToLen); IPv4
	kSlot = 3,   // lab: lane per 128-byte slot
	kLppp = 4,   // lab: software-pipelined lane per packet
	kLpp1 = 5, kLpp2 = 6, kLpp3 = 7, kLpp0 = 8, // lab: lpp shapes 1, 2 (= kLpp), 3, 0 (launch_lpp)
	kSlot2 = 9,  // lane per 128-byte slot pipelined two deep: mid-size packets that do not stream; IPv4
	kLpa = 10,   // lane per packet for aligned fixed-length strided 20..64-byte packets, A/B
		     // pipelined (lpa_ok; lpa6_kernel for CGCK_IP6 with IP / L4 flags only)
	kDstr = 11,  // dense strided frames streamed through LDS by DMA, four per step, with a writer
		     // wave (cgck_dense.hip; dstr6_kernel): strided batches of >= 1 KiB frames it
		     // accepts (dstr_ok).  Lab with kStrOld: the first stream kernel (cgck_stream.hip)
	kSpan = 12,  // lab: the packed span (coalesced register stream + prefix sums, cgck_span.hip)
	kLpd = 13,   // lpa's batches fed by LDS-DMA with staged output runs (lpd6_kernel for CGCK_IP6): the
		     // default there without verdicts, counters or stores and with stride <= 64 (lpd_ok)
	kSlotd = 14, // lab: lane per slot fed by LDS-DMA
	kLpw = 15,   // lane per packet over DMA'd windows of a step's span: strided or descriptor batches
		     // of typical length kLpwFromLen up to kGroupFromLen.  Three kernels under the one
		     // name and number: lpw_kernel (IPv4, lpw_ok), lpw6_kernel (CGCK_IP6, lpw6_ok) and
		     // lpf_kernel (IPv4 with CGCK_STORE or a `bad` pointer, lpf_ok)
};
// The names cgck_ctx_set_kernel takes; the lab build also "lpp<N>" and bare numbers (family_of).
constexpr struct { const char *name; Family family; bool lab_only; } kFamilyNames[] = {
	{"auto", kAuto, false}, {"group", kGroup, false}, {"lpp", kLpp, false},   {"slot2", kSlot2, false},
	{"lpa", kLpa, false},   {"dstr", kDstr, false},   {"lpd", kLpd, false},   {"lpw", kLpw, false},
	{"slot", kSlot, true},  {"str", kDstr, true},     {"span", kSpan, true},  {"slotd", kSlotd, true},
};

// launch_cksum's `kernel` = Family (bits 0-3) | kNT nontemporal loads | kContig
// contiguous block ranges | kExplicit take those two as given instead of the
// measured defaults | kPacked the context's layout hint is CGCK_LAYOUT_PACKED |
// kStrOld $CGCK_STR_OLD is set (lab build).  The defaults (tools/sweep.py;
// profiles/r01): the group kernel streams whole lines per wave-instruction, so
// nontemporal loads + contiguous block ranges win (1500 B: 5.79 -> 6.18 TB/s);
// the lane kernels re-touch each line from several instructions, so they want
// cached loads (NT: -30..-50 %).
constexpr int kFamilyMask = 15, kNT = 16, kContig = 32, kExplicit = 64, kPacked = 128, kStrOld = 256;
constexpr uint32_t kGroupFromLen = 1024; // typical length from which the group kernel is used
constexpr uint32_t kLppUpToLen = 128;    // lane-per-packet up to here, lane-per-slot above
constexpr uint32_t kLpwFromLen = 256;    // back-to-back frames from here stream through LDS (lpw)
constexpr int kDefaultLppShape = 2;       // see launch_lpp (6 chunks up front, predicated: best on 64 B)
constexpr bool kDefaultGroupNT = true, kDefaultGroupContig = true;
constexpr bool kDefaultLaneNT = false, kDefaultLaneContig = false;

} // namespace cgck
