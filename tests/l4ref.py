"""Referee for cgck_l4_desc: the contract of include/cgck.h (section 3, "Per-frame
TCP / UDP segment records") restated in plain Python, one frame at a time, with
byte indexing only.  It follows the reference's receive path by line:

  bsd44/tcp_input.c:67        tcps_rcvshort (a segment below a TCP header);
  bsd44/tcp_input.c:91-95     tcps_rcvbadoff (th_off below 5 words or past the segment);
  gbtcp/inet.c:123-131        the same two, where an offset past the segment counts
                              as tcps_rcvshort: hence TCP_BADOFF and TCP_OFFLONG;
  bsd44/tcp_input.c:107-110   seq, ack, win in host order;
  bsd44/tcp_input.c:925-996   tcp_dooptions: EOL, NOP, MSS / window scale on a SYN,
                              timestamps; here bounded by the option area;
  bsd44/udp_usrreq.c:65-79    udps_hdrops (below a UDP header), udps_badlen (uh_ulen
                              past the datagram); gbtcp/inet.c:154-156 likewise;
  subr.h:179-180              SO_HASH(faddr, lport, fport), in_pcb.c:175 its user.

The IP layer is cgck_rss_desc's (tests/rssref.py: the IPv4 rules restated here
byte for byte, the IPv6 chain through rssref.walk6 itself).  Nothing here calls the
library under test or shares code with the kernel."""
import numpy as np

import rssref

TCP, UDP, ICMP, OTHER, FRAG, NONE, TCP_SHORT, TCP_BADOFF, TCP_OFFLONG, UDP_SHORT, UDP_BADLEN = range(11)
NCLASS, NCOUNT = 11, 12
IP6 = 1 << 4
MSS, WS, TS, OPT_BAD = 1, 2, 4, 0x80
NAMES = ("TCP", "UDP", "ICMP", "OTHER", "FRAG", "NONE", "TCP_SHORT", "TCP_BADOFF", "TCP_OFFLONG", "UDP_SHORT",
         "UDP_BADLEN")
TH_SYN = 0x02
SEG_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"),
                      ("sport", "<u2"), ("dport", "<u2"), ("win", "<u2"), ("mss", "<u2"),
                      ("l4_off", "<u2"), ("pay_len", "<u2"), ("th_flags", "u1"), ("hdr_len", "u1"),
                      ("wscale", "u1"), ("opt", "u1")])
DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")])
FIELDS = SEG_DTYPE.names


def be(b, i, n):
    v = 0
    for j in range(n):
        v = v << 8 | int(b[i + j])
    return v


def le(b, i, n):
    return sum(int(b[i + j]) << (8 * j) for j in range(n))


def bswap16(v):
    return ((v & 255) << 8) | ((v >> 8) & 255)


def so_hash(faddr, lport, fport):
    """subr.h:179-180 on a little-endian host: the arguments are the network-order
    fields as the host loads them; ntohs swaps the 16-bit XOR of the ports."""
    return (faddr ^ (faddr >> 16) ^ bswap16((lport ^ fport) & 0xFFFF)) & 0xFFFFFFFF


def options(o, syn):
    """tcp_dooptions (tcp_input.c:925-996) over the option area o, never past it:
    (opt bits, mss, wscale, ts_val, ts_ecr)."""
    cnt, i = len(o), 0
    opt = mss = ws = tsv = tse = 0
    while i < cnt:
        kind = int(o[i])
        if kind == 0:                                   # TCPOPT_EOL, :938-939
            break
        if kind == 1:                                   # TCPOPT_NOP, :940-941
            i += 1
            continue
        if i + 1 >= cnt:                                # the length byte lies past the area
            opt |= OPT_BAD
            break
        ln = int(o[i + 1])
        if ln == 0:                                     # :944-945
            opt |= OPT_BAD
            break
        if i + ln > cnt:                                # the option ends past the area
            opt |= OPT_BAD
            break
        if kind == 2 and ln == 4 and syn:               # TCPOPT_MAXSEG, :952-960
            mss = be(o, i + 2, 2)
            opt |= MSS
        elif kind == 3 and ln == 3 and syn:             # TCPOPT_WINDOW, :962-968 (TCP_MAX_WINSHIFT 14)
            ws = min(int(o[i + 2]), 14)
            opt |= WS
        elif kind == 8 and ln == 10:                    # TCPOPT_TIMESTAMP, :970-989
            tsv, tse = be(o, i + 2, 4), be(o, i + 6, 4)
            opt |= TS
        i += ln
    return opt, mss, ws, tsv, tse


def ip_layer(b, n):
    """Step 1: (status, family bit, l4_off, proto, F); status None (the class is
    NONE), "frag" or "ok"."""
    if n == 0:
        return None, 0, 0, 0, 0
    v = int(b[0]) >> 4
    if v == 4:
        hl = (int(b[0]) & 15) * 4
        if n < 20 or hl < 20 or n < hl:
            return None, 0, 0, 0, 0
        if ((int(b[6]) << 8 | int(b[7])) & 0x3FFF) != 0:
            return "frag", 0, hl, 0, 0
        return "ok", 0, hl, int(b[9]), le(b, 12, 4)
    if v == 6:
        off, nh, st = rssref.walk6(b, n)
        if st == rssref.BADLEN:
            return None, IP6, 0, 0, 0
        if st == rssref.FRAG:
            return "frag", IP6, off, 0, 0
        return "ok", IP6, off, nh, le(b, 8, 4) ^ le(b, 12, 4) ^ le(b, 16, 4) ^ le(b, 20, 4)
    return None, 0, 0, 0, 0


def one(b):
    """(class | family bit, record as a dict of SEG_DTYPE's fields, hash) of the
    frame b (all of it: len(b) is ip_len)."""
    n = len(b)
    r = dict.fromkeys(FIELDS, 0)
    st, fam, off, proto, F = ip_layer(b, n)
    if st is None:
        return NONE | fam, r, 0
    m = n - off
    t = b[off:]
    r["l4_off"], r["pay_len"] = off, m
    if st == "frag":
        return FRAG | fam, r, 0
    if proto == 6:
        if m < 20:                                      # tcp_input.c:67, inet.c:123-125
            return TCP_SHORT | fam, r, 0
        th = (int(t[12]) >> 4) * 4
        if th < 20:                                     # tcp_input.c:91-92, inet.c:127-128
            return TCP_BADOFF | fam, r, 0
        if th > m:                                      # tcp_input.c:92 (rcvbadoff), inet.c:129-131 (rcvshort)
            return TCP_OFFLONG | fam, r, 0
        r["sport"], r["dport"] = le(t, 0, 2), le(t, 2, 2)
        r["seq"], r["ack"], r["win"] = be(t, 4, 4), be(t, 8, 4), be(t, 14, 2)     # tcp_input.c:107-110
        r["th_flags"], r["hdr_len"], r["pay_len"] = int(t[13]), th, m - th
        r["opt"], r["mss"], r["wscale"], r["ts_val"], r["ts_ecr"] = options(t[20:th], bool(int(t[13]) & TH_SYN))
        return TCP | fam, r, so_hash(F, r["dport"], r["sport"])
    if proto == 17:
        if m < 8:                                       # udp_usrreq.c:65-70 (udps_hdrops)
            return UDP_SHORT | fam, r, 0
        ulen = be(t, 4, 2)
        if ulen > m or ulen < 8:                        # udp_usrreq.c:75-79 (udps_badlen); ulen < 8: the header's own
            return UDP_BADLEN | fam, r, 0
        r["sport"], r["dport"], r["hdr_len"], r["pay_len"] = le(t, 0, 2), le(t, 2, 2), 8, ulen - 8
        return UDP | fam, r, so_hash(F, r["dport"], r["sport"])
    if proto == (58 if fam else 1):
        return ICMP | fam, r, 0
    return OTHER | fam, r, 0


def expect(buf, desc):
    """(seg SEG_DTYPE[n], cls u8[n], hash u32[n], count u32[12]: what one call adds)
    of the descriptors `desc` (DESC_DTYPE) over the byte array buf."""
    n = len(desc)
    seg = np.zeros(n, SEG_DTYPE)
    cls = np.zeros(n, np.uint8)
    hsh = np.zeros(n, np.uint32)
    for k in range(n):
        o = int(desc["frame_off"][k]) + int(desc["l3_off"][k])
        c, r, h = one(buf[o:o + int(desc["ip_len"][k])])
        cls[k], hsh[k] = c, h
        seg[k] = tuple(r[f] for f in FIELDS)
    return seg, cls, hsh, counts(cls)


def counts(cls):
    """The counters a call adds, from its class bytes."""
    cls = np.asarray(cls)
    c = np.zeros(NCOUNT, np.uint32)
    c[:NCLASS] = np.bincount(cls & 15, minlength=NCLASS)[:NCLASS]
    c[11] = np.count_nonzero(cls & IP6)
    return c
