"""Referee for cgck_l4_reply, cgck_l4_reply_packed and cgck_l4_reply_rule: the contract
of include/cgck.h (section 3, "The first reply either stack sends") restated in plain
Python over bytes, a frame at a time.  It follows the reference by line:

  bsd44/tcp_input.c:128-129   no PCB: dropwithreset;
  bsd44/tcp_input.c:881-899   an ACK is answered at its ack with RST, anything else is
                              acknowledged (a SYN counts one) with RST | ACK; the
                              RST and multicast tests of 4.4BSD are commented out (:887-890);
  bsd44/tcp_subr.c:93-123     tcp_respond with tp == NULL: addresses and ports swapped,
                              win 0, no options, no payload;
  bsd44/ip_output.c:67-68     the MACs are the configured ones, not the frame's.

Nothing here calls the library under test or shares code with the kernel."""
import numpy as np

RST, SKIP, NOTMISS, DROPPED, NONE_, QUIET = 0, 2, 3, 4, 5, 6
NAMES = {RST: "RST", SKIP: "SKIP", NOTMISS: "NOTMISS", DROPPED: "DROPPED", NONE_: "NONE", QUIET: "QUIET"}
CLASSES = tuple(NAMES)
NCLASS, NCOUNT = 7, 8
IP6 = 1 << 4
NO_RST, NO_MCAST = 1, 2
SEG_TCP = 0
PCB_MISS = 2
L2_BCAST, L2_MCAST = 1 << 6, 1 << 7
FLOW_IP6, FLOW_VLAN = 1, 2
BAD_IP, BAD_L4, BAD_LEN = 1, 2, 4
TH_SYN, TH_RST, TH_ACK = 0x02, 0x04, 0x10
SEG_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"),
                      ("sport", "<u2"), ("dport", "<u2"), ("win", "<u2"), ("mss", "<u2"),
                      ("l4_off", "<u2"), ("pay_len", "<u2"), ("th_flags", "u1"), ("hdr_len", "u1"),
                      ("wscale", "u1"), ("opt", "u1")])
FLOW_DTYPE = np.dtype([("eth_dst", "u1", (6,)), ("eth_src", "u1", (6,)), ("vlan_tci", "<u2"), ("flags", "u1"),
                       ("ttl", "u1"), ("laddr", "u1", (16,)), ("faddr", "u1", (16,))])


def vmask(ip_in, tcp_in):
    """The drop mask of a checksum policy (t_ip_do_incksum, t_tcp_do_incksum):
    ip_input.c:50-57 returns on a bad header sum whenever it checks, tcp_input.c:77-85
    drops only above 1."""
    return BAD_LEN | (BAD_IP if ip_in else 0) | (BAD_L4 if tcp_in > 1 else 0)


def classify(s, c, kd, vd, vm, lc, flags, b):
    """The class of one frame by rules 1 to 6: s its record, c / kd / vd / lc the
    selector bytes (None: the array is NULL), b the ip_len bytes."""
    c = SEG_TCP if c is None else int(c) & 15
    kd = PCB_MISS if kd is None else int(kd)
    vd = 0 if vd is None else int(vd)
    lc = 0 if lc is None else int(lc)
    n = len(b)
    if c != SEG_TCP:
        return SKIP
    if kd != PCB_MISS:
        return NOTMISS
    if vd & vm:
        return DROPPED
    if n == 0:
        return NONE_
    v = int(b[0]) >> 4
    if not ((v == 4 and n >= 20) or (v == 6 and n >= 40)):
        return NONE_
    th = int(s["th_flags"])
    if flags & NO_RST and th & TH_RST:
        return QUIET
    if flags & NO_MCAST:
        if lc & (L2_BCAST | L2_MCAST) or (v == 4 and int(b[16]) >> 4 == 14) or (v == 6 and int(b[24]) == 0xFF):
            return QUIET
    return RST


def one(s, c, kd, vd, vm, lc, flags, b, link):
    """(class byte, reply record, reply flow) of one frame."""
    cl = classify(s, c, kd, vd, vm, lc, flags, b)
    six = len(b) > 0 and int(b[0]) >> 4 == 6
    r, f = np.zeros(1, SEG_DTYPE)[0], np.zeros(1, FLOW_DTYPE)[0]
    if cl == RST:
        th = int(s["th_flags"])
        r["sport"], r["dport"] = s["dport"], s["sport"]                 # tcp_subr.c:108-110
        if th & TH_ACK:                                                 # tcp_input.c:891-892
            r["seq"], r["th_flags"] = s["ack"], TH_RST
        else:                                                           # :893-897
            r["ack"] = (int(s["seq"]) + int(s["pay_len"]) + (1 if th & TH_SYN else 0)) & 0xFFFFFFFF
            r["th_flags"] = TH_RST | TH_ACK
        f["eth_dst"], f["eth_src"], f["vlan_tci"], f["ttl"] = link["eth_dst"], link["eth_src"], link["vlan_tci"], link["ttl"]
        f["flags"] = (int(link["flags"]) & FLOW_VLAN) | (FLOW_IP6 if six else 0)
        if six:                                                         # tcp_subr.c:104-107
            f["laddr"], f["faddr"] = b[24:40], b[8:24]
        else:
            f["laddr"][:4], f["faddr"][:4] = b[16:20], b[12:16]
    return cl | (IP6 if six else 0), r, f


def counts(cls):
    """The counters a call adds, from its class bytes."""
    cls = np.asarray(cls)
    c = np.zeros(NCOUNT, np.uint32)
    c[:NCLASS] = np.bincount(cls & 15, minlength=NCLASS)[:NCLASS]
    c[7] = np.count_nonzero(cls == (RST | IP6))
    return c


def frame_bytes(buf, desc, k):
    o = int(desc["frame_off"][k]) + int(desc["l3_off"][k])
    b = buf[o:o + int(desc["ip_len"][k])]
    assert len(b) == int(desc["ip_len"][k]), "a descriptor past the buffer"
    return b


def per_frame(buf, desc, seg, link, cls=None, kind=None, verdict=None, l2cls=None, vm=0, flags=0):
    """(cls u8[n], seg SEG_DTYPE[n], flow FLOW_DTYPE[n]) in arrival order."""
    n = len(desc)
    oc, os_, of = np.zeros(n, np.uint8), np.zeros(n, SEG_DTYPE), np.zeros(n, FLOW_DTYPE)
    sel = lambda a, k: None if a is None else a[k]
    for k in range(n):
        oc[k], os_[k], of[k] = one(seg[k], sel(cls, k), sel(kind, k), sel(verdict, k), vm, sel(l2cls, k), flags,
                                   frame_bytes(buf, desc, k), link)
    return oc, os_, of


def reply(buf, desc, seg, link, cls=None, kind=None, verdict=None, l2cls=None, vm=0, flags=0, at=None, before=None):
    """cgck_l4_reply over host arrays: {seg, flow, cls, queue, count}.  With `at`, seg,
    flow and cls are `before`'s arrays (what the outputs held) with frame k's at index
    at[k] where at[k] < n; the targets must be distinct."""
    n = len(desc)
    oc, os_, of = per_frame(buf, desc, seg, link, cls, kind, verdict, l2cls, vm, flags)
    out = {"queue": np.where((oc & 15) == RST, 0, 0xFF).astype(np.uint8), "count": counts(oc)}
    if at is None:
        out.update(seg=os_, flow=of, cls=oc)
        return out
    at = np.asarray(at, np.int64)
    hit = at < n
    assert len(set(at[hit].tolist())) == int(hit.sum()), "two frames with one target"
    for x, a in (("seg", os_), ("flow", of), ("cls", oc)):
        o = before[x].copy()
        o[at[hit]] = a[hit]
        out[x] = o
    return out


def packed(buf, desc, seg, link, cls=None, kind=None, verdict=None, l2cls=None, vm=0, flags=0):
    """cgck_l4_reply_packed over host arrays: reply()'s dict with the RSTs first, in
    arrival order, then the rest in arrival order; and at u32[n], qoff u32[3]."""
    n = len(desc)
    oc, os_, of = per_frame(buf, desc, seg, link, cls, kind, verdict, l2cls, vm, flags)
    rst = (oc & 15) == RST
    order = np.concatenate([np.nonzero(rst)[0], np.nonzero(~rst)[0]]).astype(np.int64)
    at = np.zeros(n, np.uint32)
    at[order] = np.arange(n, dtype=np.uint32)
    R = int(rst.sum())
    return {"seg": os_[order], "flow": of[order], "cls": oc[order], "queue": np.where(rst, 0, 0xFF).astype(np.uint8),
            "count": counts(oc), "at": at, "qoff": np.array([0, R, n], np.uint32)}
