"""Referee for cgck_l4_build: the contract of include/cgck.h (section 3, "Frames from
segment records") restated in plain Python, one frame at a time, a byte at a time.
It follows the reference's transmit path by line:

  bsd44/tcp_output.c:255-302  the option area: MSS, window scale, timestamps, in that
                              order and padding;
  bsd44/tcp_output.c:359-418  the TCP header fields and tcp_cksum over them;
  bsd44/tcp_subr.c:52-123     tcp_template / tcp_respond: header-only segments;
  bsd44/ip_output.c:42-68     ip_v, ip_hl, ip_id, ip_off, ip_ttl, ip_cksum, the
                              Ethernet header;
  gbtcp/tcp.c:381-450         tcp_fill: the same fields with ip_off 0.

Nothing here calls the library under test or shares code with the kernel."""
import numpy as np

TCP, UDP, SKIP, BADFLOW, BADSEG, NOROOM = range(6)
NCLASS, NCOUNT = 6, 8
IP6, PAYLOAD = 1 << 4, 1 << 5
NAMES = ("TCP", "UDP", "SKIP", "BADFLOW", "BADSEG", "NOROOM")
FLOW_IP6, FLOW_VLAN = 1, 2
SEG_TCP, SEG_UDP = 0, 1
MSS, WS, TS, OPT_BAD = 1, 2, 4, 0x80
SEG_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"),
                      ("sport", "<u2"), ("dport", "<u2"), ("win", "<u2"), ("mss", "<u2"),
                      ("l4_off", "<u2"), ("pay_len", "<u2"), ("th_flags", "u1"), ("hdr_len", "u1"),
                      ("wscale", "u1"), ("opt", "u1")])
FLOW_DTYPE = np.dtype([("eth_dst", "u1", (6,)), ("eth_src", "u1", (6,)), ("vlan_tci", "<u2"), ("flags", "u1"),
                       ("ttl", "u1"), ("laddr", "u1", (16,)), ("faddr", "u1", (16,))])
DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")])
CONSULTED = ("sport", "dport", "seq", "ack", "win", "th_flags", "opt", "mss", "wscale", "ts_val", "ts_ecr", "pay_len")


def be(v, n):
    return [(v >> (8 * (n - 1 - i))) & 255 for i in range(n)]


def le16(v):
    return [v & 255, (v >> 8) & 255]


def cksum(b):
    """The header's `out` rule over the bytes b: S = the little-endian 16-bit words
    (an odd last byte is a low byte); the u16 the call sites store as it is."""
    s = 0
    for i in range(0, len(b) - 1, 2):
        s += int(b[i]) | int(b[i + 1]) << 8
    if len(b) & 1:
        s += int(b[-1])
    m = s % 65535
    return 0xFFFF if m == 0 else 0xFFFF - m


def pseudo(six, src, dst, proto, l4len):
    if six:                                             # RFC 8200 section 8.1
        return list(src) + list(dst) + be(l4len, 4) + [0, 0, 0, proto]
    return list(src) + list(dst) + [0, proto] + be(l4len, 2)      # subr.c:197-210


def lengths(flow_flags, c, opt):
    """(h, iph, l4h) by rule 4, for a class byte and flags that rules 1 to 3 let pass."""
    h = 18 if flow_flags & FLOW_VLAN else 14
    iph = 40 if flow_flags & FLOW_IP6 else 20
    l4h = 8 if c == SEG_UDP else 20 + 4 * bool(opt & MSS) + 4 * bool(opt & WS) + 12 * bool(opt & TS)
    return h, iph, l4h


def hdr_bytes(flow_flags, cls, opt):
    """cgck_l4_build_hdr_bytes."""
    c = cls & 15
    if c not in (SEG_TCP, SEG_UDP) or flow_flags & ~(FLOW_IP6 | FLOW_VLAN):
        return 0
    if c == SEG_TCP and opt & ~(MSS | WS | TS):
        return 0
    return sum(lengths(flow_flags, c, opt))


def one(s, fl, c, ip_id, ip_off, cap, l3):
    """(class | flags, header bytes or None, h, total) of one frame: s a seg record,
    fl its flow record or None (rule 2's index test failed), c the class byte."""
    c &= 15
    if c not in (SEG_TCP, SEG_UDP):                     # rule 1
        return SKIP, None, 0, 0
    if fl is None or int(fl["flags"]) & ~(FLOW_IP6 | FLOW_VLAN):          # rule 2
        return BADFLOW, None, 0, 0
    ff = int(fl["flags"])
    six = bool(ff & FLOW_IP6)
    fam = IP6 if six else 0
    opt, pay = int(s["opt"]), int(s["pay_len"])
    if c == SEG_TCP:                                    # rule 3
        if opt & ~(MSS | WS | TS) or (opt & WS and int(s["wscale"]) > 14):
            return BADSEG | fam, None, 0, 0
    elif pay > 65527:
        return BADSEG | fam, None, 0, 0
    h, iph, l4h = lengths(ff, c, opt)                   # rule 4
    total = iph + l4h + pay
    if h + total > cap or l3 + h > 65535:
        return NOROOM | fam, None, 0, 0
    proto = 6 if c == SEG_TCP else 17
    eth = list(fl["eth_dst"]) + list(fl["eth_src"])
    if ff & FLOW_VLAN:
        eth += [0x81, 0x00] + be(int(fl["vlan_tci"]), 2)
    eth += [0x86, 0xDD] if six else [0x08, 0x00]
    if six:
        src, dst = list(fl["laddr"]), list(fl["faddr"])
        ip = [0x60, 0, 0, 0] + be(l4h + pay, 2) + [proto, int(fl["ttl"])] + src + dst
    else:
        src, dst = list(fl["laddr"][:4]), list(fl["faddr"][:4])
        ip = [0x45, 0] + be(total, 2) + be(ip_id & 0xFFFF, 2) + be(ip_off, 2) + [int(fl["ttl"]), proto, 0, 0] + src + dst
        ip[10:12] = le16(cksum(ip))                     # ip_output.c:60-63
    ports = le16(int(s["sport"])) + le16(int(s["dport"]))
    if c == SEG_TCP:
        l4 = ports + be(int(s["seq"]), 4) + be(int(s["ack"]), 4) + [(l4h // 4) << 4, int(s["th_flags"])] + \
            be(int(s["win"]), 2) + [0, 0, 0, 0]
        if opt & MSS:                                   # tcp_output.c:262-267
            l4 += [2, 4] + be(int(s["mss"]), 2)
        if opt & WS:                                    # :271-276
            l4 += [1, 3, 3, int(s["wscale"])]
        if opt & TS:                                    # :290-298
            l4 += [1, 1, 8, 10] + be(int(s["ts_val"]), 4) + be(int(s["ts_ecr"]), 4)
        at = 16
    else:
        l4 = ports + be(8 + pay, 2) + [0, 0]
        at = 6
    assert len(l4) == l4h
    if pay == 0:
        l4[at:at + 2] = le16(cksum(pseudo(six, src, dst, proto, l4h) + l4))
    hdr = [int(x) for x in eth + ip + l4]
    assert len(hdr) == h + iph + l4h
    return c | fam | (PAYLOAD if pay else 0), hdr, h, total


def build(buf, slot, seg, flow, cls=None, fidx=None, ip_id0=0, ip_off=0):
    """cgck_l4_build over host arrays: writes the headers into buf (a uint8 array)
    and returns (raw_out, desc_out, cls u8[n], count u32[8]: what one call adds)."""
    n = len(slot)
    raw, desc = np.zeros(n, DESC_DTYPE), np.zeros(n, DESC_DTYPE)
    out = np.zeros(n, np.uint8)
    for k in range(n):
        fo, l3, cap = int(slot["frame_off"][k]), int(slot["l3_off"][k]), int(slot["ip_len"][k])
        f = k if fidx is None else int(fidx[k])
        c = SEG_TCP if cls is None else int(cls[k])
        r, hdr, h, total = one(seg[k], flow[f] if f < len(flow) else None, c, ip_id0 + k, ip_off, cap, l3)
        out[k] = r
        if hdr is None:
            raw[k] = desc[k] = (fo, l3, 0)
        else:
            buf[fo + l3:fo + l3 + len(hdr)] = hdr
            raw[k] = (fo, l3, h + total)
            desc[k] = (fo, l3 + h, total)
    return raw, desc, out, counts(out)


def counts(cls):
    """The counters a call adds, from its class bytes."""
    cls = np.asarray(cls)
    c = np.zeros(NCOUNT, np.uint32)
    c[:NCLASS] = np.bincount(cls & 15, minlength=NCLASS)[:NCLASS]
    built = (cls & 15) <= UDP
    c[6] = np.count_nonzero(built & ((cls & IP6) != 0))
    c[7] = np.count_nonzero(built & ((cls & PAYLOAD) != 0))
    return c


def fill(buf, desc, cls):
    """What cgck_desc(CGCK_L4 | CGCK_ZERO_FIELDS | CGCK_STORE [| CGCK_IP6]) does to the
    built frames with payload: the transport sum over header and payload."""
    for k in range(len(desc)):
        if (int(cls[k]) & 15) > UDP or not int(cls[k]) & PAYLOAD:
            continue
        o, n = int(desc["frame_off"][k]) + int(desc["l3_off"][k]), int(desc["ip_len"][k])
        six = bool(int(cls[k]) & IP6)
        iph = 40 if six else 20
        ip = buf[o:o + n]
        src, dst = (ip[8:24], ip[24:40]) if six else (ip[12:16], ip[16:20])
        proto = int(ip[6]) if six else int(ip[9])
        at = iph + (16 if proto == 6 else 6)
        ip[at:at + 2] = 0
        ip[at:at + 2] = le16(cksum(pseudo(six, src, dst, proto, n - iph) + [int(x) for x in ip[iph:]]))
