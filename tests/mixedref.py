"""Referee for the CGCK_MIXED tests: the semantics of include/cgck.h restated
in Python.  A batch is split by v, the high nibble of each packet's first byte:
IPv4 packets go through the oracle's batch referee (port.batch_desc) with the
given flags, those with ip_p == 1 with `| L4_NOPSEUDO`; IPv6 packets through
ip6ref.expect without V_UDP_ZERO_SKIP; the rest get NOT_IP, and ip_len 0 gets
BAD_LEN.  expect_pure() is the same split with the IPv4 semantics written out
over an oracle's in_cksum / udp_cksum alone, so it also runs on the reference's
compiled functions (oracle.reference(), tools/make_mixed_golden.py).  Nothing
here calls the library under test."""
import numpy as np

import ip6ref

RAW, IP, L4, L4_NOPSEUDO, ZERO_FIELDS, STORE, VERIFY = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6
V_IP_ZERO_IS_FFFF, V_UDP_ZERO_SKIP, IP6, MIXED = 1 << 7, 1 << 8, 1 << 9, 1 << 10
BAD_IP, BAD_L4, BAD_LEN, NOT_IP = 1, 2, 4, 8
DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")])


def family(buf, offs, lens):
    """Per packet: 4, 6, 0 (neither) or -1 (ip_len 0)."""
    fam = np.zeros(len(offs), np.int64)
    for i, (o, ln) in enumerate(zip(offs, lens)):
        v = int(buf[int(o)]) >> 4 if ln > 0 else -1
        fam[i] = v if v in (4, 6, -1) else 0
    return fam


def is_icmp4(buf, offs, lens, fam):
    """IPv4 packets that hold ip_p and name ICMP.  (A packet too short to hold
    byte 9 is BAD_LEN under either rule.)"""
    return np.array([f == 4 and ln > 9 and int(buf[int(o) + 9]) == 1 for o, ln, f in zip(offs, lens, fam)], bool)


def _finish(flags, fam, lens, out, ver):
    ver[fam == 0] = NOT_IP
    ver[fam == -1] = BAD_LEN
    out[(fam == 0) | (fam == -1)] = 0
    return out, ver


def expect(port, buf, offs, lens, flags):
    """(out u32, verdict u8) of a CGCK_MIXED batch: packet i is
    buf[offs[i] : offs[i] + lens[i]]; `flags` with or without MIXED."""
    flags &= ~MIXED
    assert not flags & (RAW | IP6 | L4_NOPSEUDO | STORE)
    offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
    n = len(offs)
    out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    fam = family(buf, offs, lens)
    icmp = is_icmp4(buf, offs, lens, fam)
    for sel, fl in (((fam == 4) & ~icmp, flags), ((fam == 4) & icmp, flags | L4_NOPSEUDO)):
        idx = np.nonzero(sel)[0]
        if len(idx):
            d = np.zeros(len(idx), DESC_DTYPE)
            d["frame_off"] = offs[idx]
            d["ip_len"] = lens[idx]
            out[idx], ver[idx] = port.batch_desc(buf.copy(), d.view(np.uint8), len(idx), fl)
    idx = np.nonzero(fam == 6)[0]
    if len(idx):
        out[idx], ver[idx], _ = ip6ref.expect(port, buf, offs[idx], lens[idx], (flags & ~V_UDP_ZERO_SKIP) | IP6)
    return _finish(flags, fam, lens, out, ver)


def v4_one(obj, p, ln, flags):
    """(out, verdict) of one IPv4 packet p[:ln] under CGCK_MIXED, from
    obj.in_cksum / obj.udp_cksum alone (include/cgck.h: CGCK_IP, CGCK_L4,
    CGCK_L4_NOPSEUDO for ip_p 1, CGCK_ZERO_FIELDS, CGCK_VERIFY and its two
    modifiers, CGCK_BAD_LEN)."""
    hl = (int(p[0]) & 15) * 4
    if ln < 20 or ln < hl:
        return 0, BAD_LEN
    proto = int(p[9])
    fo = {1: 2, 6: 16, 17: 6}.get(proto)
    if fo is not None and hl + fo + 2 > ln:
        fo = None
    q = np.array(p[:ln], np.uint8)
    stored_ip = int(p[10]) | int(p[11]) << 8
    stored_l4 = int(p[hl + fo]) | int(p[hl + fo + 1]) << 8 if fo is not None else 0
    if flags & (ZERO_FIELDS | VERIFY):
        q[10:12] = 0
        if fo is not None:
            q[hl + fo:hl + fo + 2] = 0
    lo = hi = ver = 0
    if flags & IP:
        lo = obj.in_cksum(q, 0, hl)
    if flags & L4:
        hi = obj.in_cksum(q, hl, ln - hl) if proto == 1 else obj.udp_cksum(q, 0, ln - hl)
    if flags & VERIFY:
        want = 0xFFFF if flags & V_IP_ZERO_IS_FFFF and stored_ip == 0 else stored_ip
        if flags & IP and lo != want:
            ver |= BAD_IP
        if flags & L4 and fo is not None and not (flags & V_UDP_ZERO_SKIP and proto == 17 and stored_l4 == 0) \
                and hi != stored_l4:
            ver |= BAD_L4
    return lo | hi << 16, ver


def expect_pure(obj, buf, offs, lens, flags):
    """expect() from obj.in_cksum / obj.udp_cksum alone."""
    flags &= ~MIXED
    offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
    n = len(offs)
    out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    fam = family(buf, offs, lens)
    for i in np.nonzero(fam == 4)[0]:
        o, ln = int(offs[i]), int(lens[i])
        out[i], ver[i] = v4_one(obj, buf[o:o + ln], ln, flags)
    idx = np.nonzero(fam == 6)[0]
    if len(idx):
        out[idx], ver[idx], _ = ip6ref.expect(obj, buf, offs[idx], lens[idx], (flags & ~V_UDP_ZERO_SKIP) | IP6)
    return _finish(flags, fam, lens, out, ver)


def counters(ver):
    """What a batch adds to bad[0], bad[1]."""
    return int(np.count_nonzero(ver & BAD_IP)), int(np.count_nonzero(ver & BAD_L4))
