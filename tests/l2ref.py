"""Referee for cgck_l2_desc: the contract of include/cgck.h (section 3, "Classify
and trim a raw Ethernet burst") restated in plain Python, one frame at a time,
with byte indexing only.  It follows the reference's receive path by line:

  bsd44/if_ether.c:152-183  bsd_eth_in: the broadcast / multicast flags (:163-168,
                            counted as if_imcasts :169-171) and the switch on the
                            ethertype (:172-182): IP, ARP, anything else dropped;
  bsd44/ip_input.c:28-44    ips_toosmall, ips_badvers, ips_badhlen (both forms);
  bsd44/ip_input.c:63-79    ips_badlen (ip_len < hlen), ips_tooshort (len < ip_len).

The VLAN walk, the IPv6 rules and RUNT are the header's own (the reference has
neither).  Nothing here calls the library under test or shares code with the
kernel."""
import numpy as np

IP4, IP6, ARP, OTHER, RUNT, TOOSMALL, BADVERS, BADHLEN, BADLEN, TOOSHORT = range(10)
NCLASS, NCOUNT = 10, 12
VLAN, BCAST, MCAST = 1 << 4, 1 << 6, 1 << 7
NAMES = ("IP4", "IP6", "ARP", "OTHER", "RUNT", "TOOSMALL", "BADVERS", "BADHLEN", "BADLEN", "TOOSHORT")
TPIDS = (0x8100, 0x88A8)
DROPS = (TOOSMALL, BADVERS, BADHLEN, BADLEN, TOOSHORT)
DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")])


def one(e, L, l3_off=0):
    """(class, flags, off, ip_len_out) of the frame e[:L] whose Ethernet header
    lies at offset l3_off of its slot.  off: where the walk stopped (14, 18, 22)."""
    if L < 14:                                          # rule 1
        return RUNT, 0, 14, 0
    flags = 0
    if all(int(e[i]) == 0xFF for i in range(6)):        # rule 3, if_ether.c:163-165
        flags |= BCAST
    elif int(e[0]) & 1:                                 # if_ether.c:166-167
        flags |= MCAST
    et, off, tags = int(e[12]) << 8 | int(e[13]), 14, 0
    while et in TPIDS and tags < 2:                     # rule 2
        if L < off + 4:
            return RUNT, flags | (VLAN if tags else 0), off, 0
        et = int(e[off + 2]) << 8 | int(e[off + 3])
        off += 4
        tags += 1
    if tags:
        flags |= VLAN
    if l3_off + off > 65535:                            # rule 8
        return RUNT, flags, off, 0
    if et in TPIDS:                                     # a third tag
        return OTHER, flags, off, 0
    avail = L - off                                     # rule 4
    b = e[off:L]
    if et == 0x0800:                                    # rule 5, if_ether.c:174-175
        if avail < 20:                                  # ip_input.c:28-31
            return TOOSMALL, flags, off, 0
        if int(b[0]) >> 4 != 4:                         # :32-35
            return BADVERS, flags, off, 0
        hl = (int(b[0]) & 15) * 4
        if hl < 20 or hl > avail:                       # :36-44
            return BADHLEN, flags, off, 0
        total = int(b[2]) << 8 | int(b[3])
        if total < hl:                                  # :63-67
            return BADLEN, flags, off, 0
        if avail < total:                               # :76-79
            return TOOSHORT, flags, off, 0
        return IP4, flags, off, total
    if et == 0x86DD:                                    # rule 6
        if avail < 40:
            return TOOSMALL, flags, off, 0
        if int(b[0]) >> 4 != 6:
            return BADVERS, flags, off, 0
        total = 40 + (int(b[4]) << 8 | int(b[5]))
        if avail < total:
            return TOOSHORT, flags, off, 0
        return IP6, flags, off, total
    if et == 0x0806:                                    # rule 7, if_ether.c:177-178
        return ARP, flags, off, 0
    return OTHER, flags, off, 0                         # if_ether.c:180-181


def expect(buf, raw):
    """(desc_out DESC_DTYPE[n], cls u8[n], count u32[12]: what one call adds) of
    the raw descriptors `raw` (DESC_DTYPE: frame_off, the Ethernet header's offset,
    the bytes delivered) over the byte array buf."""
    n = len(raw)
    out = np.zeros(n, DESC_DTYPE)
    cls = np.zeros(n, np.uint8)
    count = np.zeros(NCOUNT, np.uint32)
    for k in range(n):
        fo, l3, L = int(raw["frame_off"][k]), int(raw["l3_off"][k]), int(raw["ip_len"][k])
        c, flags, off, ip_len = one(buf[fo + l3:fo + l3 + L], L, l3)
        assert 0 <= ip_len <= 65535
        out[k] = (fo, l3 if c == RUNT else l3 + off, ip_len)
        cls[k] = c | flags
        count[c] += 1
        if flags & (BCAST | MCAST):                     # if_ether.c:169-171
            count[10] += 1
        if flags & VLAN:
            count[11] += 1
    return out, cls, count
