"""Inputs for the cgck_pcb_build / cgck_pcb_lookup tests: a deterministic corpus of
connection tables and, per table, a burst of received frames that hit, miss by
exactly one field, fall to a bound port, are skipped by class and are refused by
each length rule.  The frames are built by cgck_l4_build's referee (tests/l4bref.py)
from the peer's point of view and read back by cgck_l4_desc's (tests/l4ref.py), so
the records are the ones the receive pipeline would hand over.  Expectations come
from tests/pcbref.py; nothing here calls the library."""
import numpy as np

import l4bref as B
import l4ref
import pcbref as R

SLOT = 128
FADDR = bytes([10, 1, 0, 1])
ONE_FIELD = ("laddr", "faddr", "lport", "fport", "proto", "family")
DUP_DISTANCES = (1, 64, 256, 4096)


def be16(p):
    """The u16 a port number is stored as (be16_t on a little-endian host)."""
    return R.bswap16(p)


def flow_rec(rng, six, laddr, faddr, junk=True):
    """A flow record of the table: laddr / faddr the wire bytes (4 or 16); with junk,
    the bytes an IPv4 key ignores and everything outside the key are random."""
    f = np.zeros(1, B.FLOW_DTYPE)
    if junk:
        f.view(np.uint8)[:] = rng.integers(0, 256, f.nbytes, dtype=np.uint8)
    f["flags"] = (B.FLOW_IP6 if six else 0) | (B.FLOW_VLAN if junk and rng.integers(0, 2) else 0)
    f["laddr"][0, :len(laddr)] = list(laddr)
    f["faddr"][0, :len(faddr)] = list(faddr)
    return f[0]


class Table:
    def __init__(self, name, conn, flow, bound):
        self.name, self.bound = name, bound
        self.conn = np.array(conn, R.CONN_DTYPE)
        self.flow = np.array(flow, B.FLOW_DTYPE) if len(flow) else np.zeros(0, B.FLOW_DTYPE)

    def spec(self, j):
        """(six, proto, laddr, faddr, lport, fport) of valid connection j."""
        k = R.conn_key(self.conn[j], self.flow)
        assert not isinstance(k, str), (self.name, j, k)
        return k


def bound_ports(nconn):
    """bound[]: ports 80 and 4999 name sockets (80 one past the table: the index is the
    caller's own), every other port none."""
    b = np.full(R.NBOUND, R.NOIDX, np.uint32)
    b[80], b[4999] = nconn, 7
    return b


def dst_table(rng, nladdr):
    """A dst-cache-shaped table (con-gen.c:291-360): one faddr, lports from 5000 up,
    one fport, under nladdr local addresses; a flow per connection."""
    per = {1: 96, 3: 32, 64: 5}[nladdr]
    conn, flow = [], []
    for a in range(nladdr):
        for i in range(per):
            conn.append((len(flow), be16(5000 + i), be16(80), 6, (0, 0, 0)))
            flow.append(flow_rec(rng, False, bytes([10, 0, a // 250, 1 + a % 250]), FADDR))
    return Table(f"dst-cache x{nladdr}", conn, flow, bound_ports(len(conn)))


def sohash_table(rng):
    """Every entry has one SO_HASH (subr.h:179-180): one faddr, port pairs of one XOR."""
    conn, flow = [], [flow_rec(rng, False, bytes([10, 0, 0, 1]), FADDR)]
    x = 0x1F90 ^ 0x2345
    for i in range(200):
        lp = 5000 + 3 * i
        conn.append((0, be16(lp), be16(lp ^ x), 6, (0, 0, 0)))
    return Table("one SO_HASH", conn, flow, bound_ports(len(conn)))


def dup_table(rng):
    """Equal keys at distances 1, 64, 256 and 4096 inside a table of distinct tuples;
    the copy names another flow record with the same addresses."""
    n = 4096 + 600
    flow = [flow_rec(rng, False, bytes([10, 0, 0, 1]), FADDR), flow_rec(rng, False, bytes([10, 0, 0, 1]), FADDR)]
    conn = [(0, be16(5000 + j), be16(80), 6, (0, 0, 0)) for j in range(n)]
    pairs = []
    for d, j in zip(DUP_DISTANCES, (10, 100, 200, 500)):
        conn[j + d] = (1,) + conn[j][1:]
        pairs.append((j, j + d))
    t = Table("duplicates", conn, flow, bound_ports(n))
    t.pairs = pairs
    return t


def mixed_table(rng):
    """IPv4 flows that differ only in address bytes 4..15 (equal keys), the same tuple
    as TCP and as UDP (different keys), an IPv4 and an IPv6 flow with equal first four
    address bytes, unused and bad entries, a port below 5000 that is both a connection
    and bound, a protocol that no frame carries."""
    l4, f4 = bytes([192, 168, 1, 1]), bytes([192, 168, 1, 2])
    l6, f6 = l4 + bytes(range(12)), f4 + bytes(range(12, 24))
    flow = [flow_rec(rng, False, l4, f4), flow_rec(rng, False, l4, f4),      # 0, 1: equal IPv4 keys, other junk
            flow_rec(rng, True, l6, f6),                                        # 2: IPv6, the same first four bytes
            flow_rec(rng, True, l6[:15] + b"\xEE", f6),                         # 3: IPv6, another last byte
            flow_rec(rng, False, l4, f4), flow_rec(rng, False, l4, f4)]         # 4, 5: refused flags
    flow[4]["flags"], flow[5]["flags"] = 0x04, 0x81
    assert bytes(flow[0]["laddr"][4:]) != bytes(flow[1]["laddr"][4:])
    c = [(0, be16(6000), be16(443), 6), (1, be16(6000), be16(443), 6),          # 0, 1: equal keys through flows 0 and 1
         (0, be16(6000), be16(443), 17),                                        # 2: the same tuple as UDP
         (2, be16(6000), be16(443), 6), (2, be16(6000), be16(443), 17),         # 3, 4: the IPv6 flow
         (3, be16(6000), be16(443), 6),                                         # 5
         (0, be16(6001), be16(443), 0),                                         # 6: unused
         (9, be16(6002), be16(443), 6), (0xFFFFFFFF, be16(6002), be16(443), 6), # 7, 8: flow past nflow
         (4, be16(6003), be16(443), 6), (5, be16(6003), be16(443), 17),         # 9, 10: refused flags
         (0, be16(6002), be16(443), 6), (0, be16(6003), be16(443), 6),          # 11, 12: the tuples 7..10 would have had
         (0, be16(80), be16(999), 6),                                           # 13: below 5000, and bound
         (0, be16(6004), be16(443), 1),                                         # 14: ICMP's number: valid, never looked up
         (0, be16(6001), be16(443), 6)]                                         # 15: the tuple of the unused entry 6
    conn = [x + ((1, 2, 3),) for x in c]                                        # rsv is ignored
    return Table("mixed", conn, flow, bound_ports(len(conn)))


def tables(rng):
    return [dst_table(rng, 1), dst_table(rng, 3), dst_table(rng, 64), sohash_table(rng), dup_table(rng), mixed_table(rng)]


# -- frames -------------------------------------------------------------------------------

def other(v, six=None):
    """Another value of a key field: the last byte of an address, or a port, changed."""
    if isinstance(v, bytes):
        return v[:-1] + bytes([v[-1] ^ 0x40])
    return v ^ 0x0100


def as_family(a, six):
    return a + bytes(12) if six else a[:4]


def specs_for(t, rng, nhit=48):
    """[(tag, (six, proto, laddr, faddr, lport, fport), mod)] for table t: hits, one-field
    misses, falls to bound[], SKIP by class, NONE by each length rule."""
    valid = [j for j in range(len(t.conn)) if not isinstance(R.conn_key(t.conn[j], t.flow), str)
             and int(t.conn["proto"][j]) in (6, 17)]
    pick = sorted(set(valid[:8] + valid[-8:] + [int(x) for x in rng.choice(valid, min(nhit, len(valid)), replace=False)]
                      + [j for p in getattr(t, "pairs", []) for j in p]))
    out = [("hit", t.spec(j), None) for j in pick]
    base = [t.spec(j) for j in pick[:2] + pick[-1:]]          # the last one has no twin of the other protocol
    for six, proto, la, fa, lp, fp in base:
        out += [("miss:laddr", (six, proto, other(la), fa, lp, fp), None), ("miss:faddr", (six, proto, la, other(fa), lp, fp), None),
                ("miss:lport", (six, proto, la, fa, be16(be16(lp) + 20000), fp), None),
                ("miss:fport", (six, proto, la, fa, lp, other(fp)), None),
                ("miss:proto", (six, 23 - proto, la, fa, lp, fp), None),
                ("miss:family", (not six, proto, as_family(la, not six), as_family(fa, not six), lp, fp), None)]
    six, proto, la, fa, lp, fp = base[0]
    out += [("bound", (six, proto, other(la), fa, be16(80), fp), None), ("bound", (six, 17, la, fa, be16(4999), fp), None),
            ("bound", (True, proto, bytes(16), bytes(16), be16(80), fp), None),             # neither proto nor family compared
            ("miss:unbound", (six, proto, other(la), fa, be16(81), fp), None),                # below 5000, nobody bound
            ("miss:unbound", (six, proto, other(la), fa, be16(5000 + 4999), other(fp)), None)]
    s0 = base[0]
    s6 = (True, 6, bytes(range(16)), bytes(range(16, 32)), be16(6000), be16(443))
    s4 = (False, 6, bytes([1, 2, 3, 4]), bytes([5, 6, 7, 8]), be16(6000), be16(443))
    out += [("skip", s0, ("cls", c)) for c in (2, 5, 10, 15, 0x12)]
    out += [("none:len0", s0, ("len", 0)), ("none:v4short", s4, ("len", 19)), ("none:v6short", s6, ("len", 39)),
            ("none:v6as20", s6, ("len", 20)), ("none:version", s0, ("ver", 0x55)), ("none:version", s0, ("ver", 0x0F)),
            ("hit", s0, ("len", 40 if s0[0] else 20)),                                     # exactly the addresses: still looked up
            ("hit", s0, ("clsflags", 0xE0))]                                                # only the low nibble of cls counts
    return out


class Burst:
    """buf, desc, seg, cls and the tag of each frame."""


def burst(specs, rng, align=None):
    """The received frames of `specs` in SLOT-byte slots: each is built by l4bref from
    the peer's flow (its source is the connection's faddr) and read back by l4ref.
    align: every frame's IP header starts at that offset mod 16."""
    n = len(specs)
    flow = np.zeros(n, B.FLOW_DTYPE)
    seg = np.zeros(n, B.SEG_DTYPE)
    cls = np.zeros(n, np.uint8)
    slot = np.zeros(n, B.DESC_DTYPE)
    for k, (_, (six, proto, la, fa, lp, fp), _) in enumerate(specs):
        flow[k] = flow_rec(rng, six, fa, la)
        tag = bool(int(flow[k]["flags"]) & B.FLOW_VLAN)
        seg[k]["sport"], seg[k]["dport"] = fp, lp
        seg[k]["seq"], seg[k]["ack"], seg[k]["win"] = rng.integers(0, 2 ** 32), rng.integers(0, 2 ** 32), rng.integers(0, 65536)
        seg[k]["th_flags"], seg[k]["opt"] = (0x02, int(rng.integers(0, 8))) if k % 3 == 0 else (0x10, int(rng.integers(0, 2)) * B.TS)
        cls[k] = B.SEG_TCP if proto == 6 else B.SEG_UDP
        h = 18 if tag else 14
        l3 = 0 if align is None else (align - h) % 16
        slot[k] = (k * SLOT, l3, SLOT - l3)
    buf = rng.integers(0, 256, n * SLOT, dtype=np.uint8)
    _, desc, bcls, _ = B.build(buf, slot, seg, flow, cls, None, int(rng.integers(0, 65536)), 0x4000)
    assert np.all((bcls & 15) <= B.UDP)
    for k, (_, _, mod) in enumerate(specs):
        if mod and mod[0] == "ver":
            buf[int(desc["frame_off"][k]) + int(desc["l3_off"][k])] = mod[1]
    sg, c4, _, _ = l4ref.expect(buf, desc)
    out = Burst()
    for k, (_, _, mod) in enumerate(specs):
        if mod is None:
            assert int(c4[k]) & 15 == int(cls[k]), (k, c4[k])
            cls[k] = c4[k]                              # with l4ref's family flag, as cgck_l4_desc hands it over
        elif mod[0] == "cls":
            cls[k] = mod[1]
        elif mod[0] == "clsflags":
            cls[k] |= mod[1]
        elif mod[0] == "len":
            desc["ip_len"][k] = mod[1]
        if mod is None or mod[0] != "ver":
            assert (int(sg["sport"][k]), int(sg["dport"][k])) == (int(seg["sport"][k]), int(seg["dport"][k]))
        sg[k]["sport"], sg[k]["dport"] = seg["sport"][k], seg["dport"][k]       # a frame l4ref refuses keeps its ports
    out.buf, out.desc, out.seg, out.cls, out.tags = buf, desc, sg, cls, [s[0] for s in specs]
    if align is not None:
        assert np.all(((desc["frame_off"].astype(np.int64) + desc["l3_off"]) & 15) == align)
    return out


class Case:
    def __init__(self, t, b):
        self.table, self.burst, self.name = t, b, t.name


def corpus(seed=51):
    """One Case per table class."""
    rng = np.random.default_rng(seed)
    return [Case(t, burst(specs_for(t, rng), rng)) for t in tables(rng)]


def tiled(b, n):
    """Burst b repeated to n frames: (buf, desc, seg, cls)."""
    m = len(b.desc)
    k = np.arange(n)
    desc = b.desc[k % m].copy()
    desc["frame_off"] = (k // m) * len(b.buf) + b.desc["frame_off"][k % m]
    return np.tile(b.buf, -(-n // m)), desc, b.seg[k % m].copy(), b.cls[k % m].copy()


def tail_burst(t, align, six, rng):
    """Three frames whose last is a hit that starts at `align` mod 16, has ip_len 20
    (40 for IPv6) and ends the buffer: its last address byte is the allocation's last."""
    want = [j for j in range(len(t.conn)) if not isinstance(R.conn_key(t.conn[j], t.flow), str)
            and R.conn_key(t.conn[j], t.flow)[0] == six and int(t.conn["proto"][j]) in (6, 17)]
    specs = [("hit", t.spec(want[0]), None), ("miss:lport", t.spec(want[0])[:4] + (be16(61000), be16(1)), None),
             ("hit", t.spec(want[-1]), None)]
    b = burst(specs, rng, align)
    n = 40 if six else 20
    b.desc["ip_len"][2] = n
    b.buf = b.buf[:int(b.desc["frame_off"][2]) + int(b.desc["l3_off"][2]) + n].copy()
    return b


def write_model_file(path, t, b, use_cls=True, use_bound=True):
    """The corpus file tools/pcb_model reads: a header of nine u32 (magic, nconn, nflow,
    n, bound present, cls present, buffer bytes, 0, 0), then conn, flow, bound, desc,
    seg, cls, buf."""
    bound = t.bound if use_bound else None
    hdr = np.array([0x42435043, len(t.conn), len(t.flow), len(b.desc), bound is not None, use_cls, len(b.buf), 0, 0], np.uint32)
    with open(path, "wb") as f:
        for a in (hdr, t.conn, t.flow, bound, b.desc, b.seg, b.cls if use_cls else None, b.buf):
            if a is not None:
                f.write(np.ascontiguousarray(a).tobytes())


def read_model_file(path, n):
    """(stat, idx, fidx, kind, count) as tools/pcb_model writes them."""
    raw = np.fromfile(path, np.uint8)
    assert len(raw) == 16 + 4 * n + 4 * n + n + 24, len(raw)
    u = lambda a, b: raw[a:b].copy().view(np.uint32)
    return u(0, 16), u(16, 16 + 4 * n), u(16 + 4 * n, 16 + 8 * n), raw[16 + 8 * n:16 + 9 * n].copy(), u(16 + 9 * n, 40 + 9 * n)
