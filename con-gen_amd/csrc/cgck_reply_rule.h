// cgck_reply_rule.h — the rule of cgck_l4_reply (include/cgck.h, section 3):
// tcp_respond's RST for a segment that found no PCB (bsd44/tcp_input.c:128-129,
// 881-899; tcp_subr.c:93-123), with tp == NULL, as one inline function over
// dwords.  l4r_kernel (cgck_l4r.hip) compiles it for the device over the chunks
// it realigned; cgck_l4_reply_rule (cgck_reply_rule.cpp) compiles the same text
// for the host over the caller's bytes.  Plain C++: no HIP header is needed to
// read it.
//
// Dwords.  A record is its memory read as little-endian dwords: S[0..8) a
// cgck_seg_t (S[0] seq, S[1] ack, S[4] sport | dport << 16, S[6] l4_off |
// pay_len << 16, S[7] th_flags | hdr_len << 8 | wscale << 16 | opt << 24), F[0..12)
// a cgck_flow_t (F[0..3) the MACs, F[3] vlan_tci | flags << 16 | ttl << 24, F[4..8)
// laddr, F[8..12) faddr), B[0..12) the frame's bytes [0, 48).  Bytes of B at or
// past ip_len may hold anything: a length is compared before a byte is consulted.
#pragma once
#include <cstdint>

#include "cgck.h"

#if defined(__HIPCC__)
#define CGCK_RPL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CGCK_RPL_HD inline
#endif

namespace cgck {

// The class byte is cgck_l4_build's in.cls: an RST is a TCP segment to build,
// every other class a value its rule 1 skips, and the family flag is the same bit.
static_assert((int)CGCK_RPL_RST == (int)CGCK_SEG_TCP, "an RST's class byte must build as TCP");
static_assert((int)CGCK_RPL_SKIP > (int)CGCK_SEG_UDP && (int)CGCK_RPL_NOTMISS > (int)CGCK_SEG_UDP &&
		      (int)CGCK_RPL_DROPPED > (int)CGCK_SEG_UDP && (int)CGCK_RPL_NONE > (int)CGCK_SEG_UDP &&
		      (int)CGCK_RPL_QUIET > (int)CGCK_SEG_UDP && (int)CGCK_RPL_NCLASS <= 16,
	      "every class but RST must be one cgck_l4_build skips");
static_assert((int)CGCK_RPL_IP6 == (int)CGCK_SEG_IP6 && (int)CGCK_RPL_IP6 == (int)CGCK_BLD_IP6, "one family flag");
static_assert(CGCK_RPL_NCOUNT == CGCK_RPL_NCLASS + 1, "a counter a class and one for the IPv6 RSTs");
static_assert(sizeof(cgck_seg_t) == 32 && sizeof(cgck_flow_t) == 48, "the records as dwords");

constexpr uint32_t kRplFlags = CGCK_RPL_NO_RST | CGCK_RPL_NO_MCAST;
constexpr uint32_t kRplLinkBits = CGCK_FLOW_IP6 | CGCK_FLOW_VLAN; // what link.flags may hold

// c: cls[k] & 15 (or CGCK_SEG_TCP), kd: kind[k] (or CGCK_PCB_MISS), vd: verdict[k]
// (or 0), lc: l2cls[k] (or 0); link: the template's first four dwords.  Returns
// class | CGCK_RPL_IP6 and fills r and f: the reply for an RST, zeros otherwise.
CGCK_RPL_HD uint32_t reply_rule(const uint32_t (&S)[8], uint32_t c, uint32_t kd, uint32_t vd, uint32_t vmask,
				uint32_t lc, uint32_t flags, const uint32_t (&B)[12], uint32_t ip_len,
				const uint32_t (&link)[4], uint32_t (&r)[8], uint32_t (&f)[12])
{
	const uint32_t v = (B[0] & 255u) >> 4;
	const bool six = v == 6;
	const uint32_t fam = ip_len != 0 && six ? (uint32_t)CGCK_RPL_IP6 : 0u;
	const uint32_t thf = S[7] & 255u;
	uint32_t cl;
	if (c != CGCK_SEG_TCP)
		cl = CGCK_RPL_SKIP; // rule 1
	else if (kd != CGCK_PCB_MISS)
		cl = CGCK_RPL_NOTMISS; // rule 2
	else if (vd & vmask)
		cl = CGCK_RPL_DROPPED; // rule 3
	else if (ip_len == 0 || !((v == 4 && ip_len >= 20) || (six && ip_len >= 40)))
		cl = CGCK_RPL_NONE; // rule 4: cgck_pcb_lookup's rule 2
	else {
		// rule 5: 4.4BSD's test, which tcp_input.c:887-890 has commented out
		const bool mcast = (lc & (CGCK_L2_BCAST | CGCK_L2_MCAST)) != 0 || (six ? (B[6] & 255u) == 255u : (B[4] & 0xF0u) == 0xE0u);
		const bool quiet = ((flags & CGCK_RPL_NO_RST) && (thf & 0x04u)) || ((flags & CGCK_RPL_NO_MCAST) && mcast);
		cl = quiet ? (uint32_t)CGCK_RPL_QUIET : (uint32_t)CGCK_RPL_RST;
	}
	const bool rst = cl == CGCK_RPL_RST;
	const uint32_t m = rst ? ~0u : 0u;
	// tcp_input.c:891-897: an ACK is answered at its own ack; anything else is
	// acknowledged, a SYN counting one
	const bool ack = (thf & 0x10u) != 0;
	r[0] = m & (ack ? S[1] : 0u);
	r[1] = m & (ack ? 0u : S[0] + (S[6] >> 16) + ((thf >> 1) & 1u));
	r[2] = r[3] = r[5] = r[6] = 0; // win, opt and pay_len 0 (tcp_subr.c:115-116)
	r[4] = m & (S[4] >> 16 | S[4] << 16); // tcp_subr.c:108-110: the ports swapped
	r[7] = m & (ack ? 0x04u : 0x14u);
	// tcp_subr.c:104-107: the addresses swapped; the link header is the caller's
	// (ip_output.c:67-68 sends from configured MACs, not the frame's)
	f[0] = m & link[0];
	f[1] = m & link[1];
	f[2] = m & link[2];
	f[3] = m & ((link[3] & 0xFF00FFFFu) | ((link[3] >> 16 & (uint32_t)CGCK_FLOW_VLAN) | (six ? (uint32_t)CGCK_FLOW_IP6 : 0u)) << 16);
	f[4] = m & (six ? B[6] : B[4]);
	f[8] = m & (six ? B[2] : B[3]);
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (int i = 1; i < 4; ++i) {
		f[4 + i] = m & (six ? B[6 + i] : 0u);
		f[8 + i] = m & (six ? B[2 + i] : 0u);
	}
	return cl | fam;
}

} // namespace cgck
