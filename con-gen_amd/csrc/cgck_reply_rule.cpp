// cgck_reply_rule.cpp — cgck_l4_reply_rule (no device, no context): the rule of
// cgck_reply_rule.h over one frame in host memory, the text l4r_kernel compiles.
// What a host-resident burst uses in place of a hand-written RST loop.
#include <errno.h>
#include <string.h>

#include "cgck_reply_rule.h"

extern "C" int cgck_l4_reply_rule(const cgck_seg_t *s, uint8_t cls, uint8_t kind, uint8_t verdict, uint8_t vmask,
				  uint8_t l2cls, uint32_t flags, const uint8_t *ip, uint32_t ip_len, const cgck_flow_t *link,
				  cgck_seg_t *r, cgck_flow_t *f)
{
	// the refusals cgck_l4_reply makes for the same arguments
	if (!s || !link || !r || !f || (ip_len && !ip) || (flags & ~cgck::kRplFlags) || (link->flags & ~cgck::kRplLinkBits))
		return -EINVAL;
	uint32_t S[8], B[12] = {}, K[4], R[8], F[12];
	memcpy(S, s, sizeof(S));
	memcpy(K, link, sizeof(K));
	if (ip_len)
		memcpy(B, ip, ip_len < sizeof(B) ? ip_len : sizeof(B)); // ip_len bounds every read
	const uint32_t c = cgck::reply_rule(S, cls & 15u, kind, verdict, vmask, l2cls, flags, B, ip_len, K, R, F);
	memcpy(r, R, sizeof(R));
	memcpy(f, F, sizeof(F));
	return (int)c;
}
