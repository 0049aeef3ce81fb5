"""Referee for cgck_pcb_build and cgck_pcb_lookup: the contract of include/cgck.h
(section 3, "Per-frame connection lookup") restated in plain Python, a frame at a
time, with a dict keyed by the whole tuple in which the lowest index stays.  It
follows the reference by line:

  bsd44/in_pcb.c:167-192   in_pcblookup(proto, laddr, lport, faddr, fport): the exact
                           match first, then the socket bound to a port below
                           EPHEMERAL_MIN, whatever its protocol;
  bsd44/tcp_input.c:118    in_pcblookup(IPPROTO_TCP, ip_dst, th_dport, ip_src, th_sport);
  bsd44/udp_usrreq.c:97    the same for UDP;
  subr.h:62                EPHEMERAL_MIN 5000.

brute() is the same contract as a scan over the connections, without the dict.
Nothing here calls the library under test or shares code with the kernel."""
import numpy as np

HIT, BOUND, MISS, SKIP, NONE_ = range(5)
NAMES = ("HIT", "BOUND", "MISS", "SKIP", "NONE")
NCLASS, NCOUNT, NBOUND = 5, 6, 5000
NOIDX = 0xFFFFFFFF
FLOW_IP6, FLOW_VLAN = 1, 2
SEG_TCP, SEG_UDP = 0, 1
CONN_DTYPE = np.dtype([("flow", "<u4"), ("lport", "<u2"), ("fport", "<u2"), ("proto", "u1"), ("rsv", "u1", (3,))])


def bswap16(v):
    return ((v & 255) << 8) | ((v >> 8) & 255)


def conn_key(c, flow):
    """The key of connection record c, or "unused" / "bad" when it has none."""
    if int(c["proto"]) == 0:
        return "unused"
    f = int(c["flow"])
    if f >= len(flow):
        return "bad"
    fl = flow[f]
    ff = int(fl["flags"])
    if ff & ~(FLOW_IP6 | FLOW_VLAN):
        return "bad"
    w = 16 if ff & FLOW_IP6 else 4
    return (bool(ff & FLOW_IP6), int(c["proto"]), bytes(fl["laddr"][:w]), bytes(fl["faddr"][:w]), int(c["lport"]),
            int(c["fport"]))


def table(conn, flow):
    """(dict key -> lowest valid index, stat u32[4]) of cgck_pcb_build."""
    t, stat = {}, np.zeros(4, np.uint32)
    for j in range(len(conn)):
        k = conn_key(conn[j], flow)
        if k == "unused":
            stat[2] += 1
        elif k == "bad":
            stat[3] += 1
        elif k in t:
            stat[1] += 1
        else:
            t[k] = j
            stat[0] += 1
    return t, stat


def frame_key(b, c, s):
    """Rules 1 and 2 for the ip_len bytes b, the class byte c (None: TCP) and the
    record s: SKIP, NONE_, or the frame's key."""
    c = SEG_TCP if c is None else int(c) & 15
    if c not in (SEG_TCP, SEG_UDP):
        return SKIP
    n = len(b)
    if n == 0:
        return NONE_
    v = int(b[0]) >> 4
    proto = 6 if c == SEG_TCP else 17
    if v == 4 and n >= 20:
        return (False, proto, bytes(b[16:20]), bytes(b[12:16]), int(s["dport"]), int(s["sport"]))
    if v == 6 and n >= 40:
        return (True, proto, bytes(b[24:40]), bytes(b[8:24]), int(s["dport"]), int(s["sport"]))
    return NONE_


def resolve(key, s, find, conn, bound):
    """(kind, idx, fidx) by rules 3 to 5; find(key) is the lowest valid index or None."""
    j = find(key)
    if j is not None:
        return HIT, j, int(conn["flow"][j])
    if bound is not None:
        p = bswap16(int(s["dport"]))
        if p < NBOUND and int(bound[p]) != NOIDX:
            return BOUND, int(bound[p]), NOIDX
    return MISS, NOIDX, NOIDX


def _run(buf, desc, seg, cls, conn, bound, find):
    n = len(desc)
    idx, fidx = np.full(n, NOIDX, np.uint32), np.full(n, NOIDX, np.uint32)
    kind = np.zeros(n, np.uint8)
    count = np.zeros(NCOUNT, np.uint32)
    for k in range(n):
        o = int(desc["frame_off"][k]) + int(desc["l3_off"][k])
        b = buf[o:o + int(desc["ip_len"][k])]
        assert len(b) == int(desc["ip_len"][k]), "a descriptor past the buffer"
        key = frame_key(b, None if cls is None else cls[k], seg[k])
        if isinstance(key, int):
            kind[k] = key
        else:
            kind[k], idx[k], fidx[k] = resolve(key, seg[k], find, conn, bound)
            if kind[k] == HIT and key[0]:
                count[5] += 1
        count[kind[k]] += 1
    return idx, fidx, kind, count


def lookup(buf, desc, seg, cls, conn, flow, bound=None):
    """cgck_pcb_lookup over host arrays: (idx u32[n], fidx u32[n], kind u8[n],
    count u32[6]: what one call adds)."""
    t, _ = table(conn, flow)
    return _run(buf, desc, seg, cls, conn, bound, t.get)


def brute(buf, desc, seg, cls, conn, flow, bound=None):
    """The same by a scan of conn[] per frame."""
    keys = [conn_key(conn[j], flow) for j in range(len(conn))]

    def find(key):
        for j, k in enumerate(keys):
            if k == key:
                return j
        return None
    return _run(buf, desc, seg, cls, conn, bound, find)


def true_hit(b, c, s, conn, flow, j):
    """Connection j is valid and its key is the frame's (the check of a HIT reported
    from a table the library did not build)."""
    key = frame_key(b, c, s)
    return not isinstance(key, int) and 0 <= j < len(conn) and conn_key(conn[j], flow) == key
