"""CPU tests of the cgck_l4_desc test infrastructure (no GPU): the class corpus
covers what the contract names, the referee (tests/l4ref.py) answers hand-written
frames as each rule says, it agrees with the reference stack's replay
(oracle/stack_replay.c) where the two overlap, its hash is the dst-cache entry's,
and the binding's constants are the header's."""
import ctypes
import os
import re
import socket

import numpy as np

import cgck
import l2ref
import l4batches as LB
import l4ref
import rxcorpus
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = l4ref


def test_corpus_covers_required():
    items = LB.classes(np.random.default_rng(11))
    seen = set()
    for it in items:
        seen |= LB.tags(it)
    assert not LB.REQUIRED - seen, sorted(LB.REQUIRED - seen)
    assert len(items) < 400
    # every class of both families also lies in the 128-byte slots of the tiled bursts
    buf, desc, m = LB.tiled(items, 1)
    assert m > 200
    seg, cls, hsh, count = l4ref.expect(*LB.tiled(items, m)[:2])
    assert {int(c) for c in cls} >= {c | f for c in range(R.NCLASS) for f in (0, R.IP6)}
    assert np.array_equal(count, LB.counts(cls)) and int(count[:R.NCLASS].sum()) == m
    assert np.count_nonzero(seg["l4_off"].astype(int) + seg["hdr_len"] > 80) > 20       # headers past the first 80 bytes


def test_corpus_option_rules():
    """Every labelled item reads as its rule's row says, whatever lies behind it."""
    items = LB.classes(np.random.default_rng(11))
    seen = {}
    for f, tail, label in items:
        if label is None:
            continue
        flags, opts, opt, mss, ws, ts = LB.OPTION_RULES[label]
        c, r, h = l4ref.one(f)
        assert c & 15 == R.TCP and r["th_flags"] == flags and r["hdr_len"] == 20 + len(opts), label
        assert (r["opt"], r["mss"], r["wscale"]) == (opt, mss, ws), (label, r)
        want = (l4ref.be(ts, 0, 4), l4ref.be(ts, 4, 4)) if ts else (0, 0)
        assert (r["ts_val"], r["ts_ecr"]) == want, label
        # the same frame with its tail appended as payload reads the same options
        if tail is not None:
            r2 = l4ref.one(np.concatenate((f, np.array(tail, np.uint8))))[1]
            assert all(r2[x] == r[x] for x in ("opt", "mss", "wscale", "ts_val", "ts_ecr")), label
        seen[label] = seen.get(label, 0) + 1
    assert set(seen) == set(LB.OPTION_RULES) and all(v == 8 for v in seen.values())


# -- the rule table ----------------------------------------------------------------------

SRC, DST = (10, 0, 0, 1), (10, 0, 0, 2)
F4 = 0x0100000A                                   # b[12..16) loaded little-endian
PORTS = (0x12, 0x34, 0x00, 0x50)                  # sport 0x1234, dport 80 on the wire
SP, DP = 0x3412, 0x5000                           # as stored
H4 = 0x0100136E                                   # F4 ^ F4 >> 16 ^ bswap16(DP ^ SP), by hand


def fr(*parts):
    return np.array([b for p in parts for b in p], np.uint8)


def v4(proto, hl=5, frag=0, b0=None):
    h = [0x40 | hl if b0 is None else b0, 0, 0, 0, 0, 0, frag >> 8, frag & 255, 64, proto, 0, 0, *SRC, *DST]
    return tuple(h + [0x99] * (4 * hl - 20))


def v6(nh, b0=0x60):
    return (b0, 0, 0, 0, 0, 0, nh, 64) + tuple(range(1, 17)) + tuple(range(101, 117))


F6 = 0x04030201 ^ 0x08070605 ^ 0x0C0B0A09 ^ 0x100F0E0D
H6 = F6 ^ (F6 >> 16) ^ 0x1264


def th(off, flags=0x10, ports=PORTS):
    return tuple(ports) + (1, 2, 3, 4, 5, 6, 7, 8, (off // 4) << 4 | 0x0F, flags, 0x10, 0x00, 0xAB, 0xCD, 0, 9)


def uh(ulen):
    return tuple(PORTS) + (ulen >> 8, ulen & 255, 0xAB, 0xCD)


TCPF = dict(sport=SP, dport=DP, seq=0x01020304, ack=0x05060708, win=0x1000, th_flags=0x10, hdr_len=20)
SYNF = dict(TCPF, th_flags=0x02)
PAD = (0x77,) * 40
RULES = (
    # (rule, frame, class | family bit, the non-zero fields, hash)
    ("1: ip_len 0", fr(), R.NONE, {}, 0),
    ("1: version 5", fr(v4(6, b0=0x55), th(20)), R.NONE, {}, 0),
    ("1: v4 ip_len 19", fr(v4(6))[:19], R.NONE, {}, 0),
    ("1: v4 hl 16", fr(v4(6, b0=0x44), th(20)), R.NONE, {}, 0),
    ("1: v4 ip_len below hl", fr(v4(6, hl=6))[:23], R.NONE, {}, 0),
    ("1: v4 MF", fr(v4(6, frag=0x2000), th(20)), R.FRAG, dict(l4_off=20, pay_len=20), 0),
    ("1: v4 offset 1", fr(v4(17, hl=6, frag=1), uh(8)), R.FRAG, dict(l4_off=24, pay_len=8), 0),
    ("1: v4 DF alone is no fragment", fr(v4(6, frag=0x4000), th(20)), R.TCP, dict(TCPF, l4_off=20), H4),
    ("1: v4 reserved bit alone is no fragment (ip_input.c:94 drops it)", fr(v4(6, frag=0x8000), th(20)), R.TCP,
     dict(TCPF, l4_off=20), H4),
    ("1: v6 ip_len 39 keeps the family bit", fr(v6(6), th(20))[:39], R.NONE | R.IP6, {}, 0),
    ("1: v6 chain cut", fr(v6(0), (6,)), R.NONE | R.IP6, {}, 0),
    ("1: v6 l4_off past ip_len", fr(v6(0), (6, 1, 0, 0, 0, 0, 0, 0)), R.NONE | R.IP6, {}, 0),
    ("1: v6 ninth extension header", fr(v6(0), (60, 0, 0, 0, 0, 0, 0, 0) * 8, (6, 0, 0, 0, 0, 0, 0, 0), th(20)),
     R.NONE | R.IP6, {}, 0),
    ("1: v6 eight extension headers", fr(v6(0), (60, 0, 0, 0, 0, 0, 0, 0) * 7, (6, 0, 0, 0, 0, 0, 0, 0), th(20)),
     R.TCP | R.IP6, dict(TCPF, l4_off=104), H6),
    ("1: v6 Fragment header", fr(v6(44), (6, 0, 0, 0, 0, 0, 0, 1), th(20)), R.FRAG | R.IP6, dict(l4_off=40, pay_len=28), 0),
    ("1: v6 Fragment header behind AH", fr(v6(51), (44, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (6, 0, 0, 0, 0, 0, 0, 1)),
     R.FRAG | R.IP6, dict(l4_off=52, pay_len=8), 0),
    ("3: m 19 (tcp_input.c:67)", fr(v4(6), th(20))[:39], R.TCP_SHORT, dict(l4_off=20, pay_len=19), 0),
    ("3: m 0", fr(v4(6)), R.TCP_SHORT, dict(l4_off=20), 0),
    ("3: m 20", fr(v4(6), th(20)), R.TCP, dict(TCPF, l4_off=20), H4),
    ("3: off 16 (tcp_input.c:91-92)", fr(v4(6), th(16), PAD), R.TCP_BADOFF, dict(l4_off=20, pay_len=60), 0),
    ("3: off m + 4 (tcp_input.c:92 badoff, inet.c:129-131 rcvshort)", fr(v4(6), th(24)), R.TCP_OFFLONG,
     dict(l4_off=20, pay_len=20), 0),
    ("3: off == m", fr(v4(6), th(24), (1, 1, 1, 0)), R.TCP, dict(TCPF, l4_off=20, hdr_len=24), H4),
    ("3: off 60 past m 59", fr(v4(6), th(60), PAD)[:79], R.TCP_OFFLONG, dict(l4_off=20, pay_len=59), 0),
    ("3: off 60", fr(v4(6), th(60), (1,) * 40, (5, 5)), R.TCP, dict(TCPF, l4_off=20, hdr_len=60, pay_len=2), H4),
    ("3: payload", fr(v6(6), th(20), (9,) * 7), R.TCP | R.IP6, dict(TCPF, l4_off=40, pay_len=7), H6),
    ("3: behind IPv4 options", fr(v4(6, hl=15), th(20), (9,)), R.TCP, dict(TCPF, l4_off=60, pay_len=1), H4),
    ("3o: EOL first", fr(v4(6), th(28, 2), (0, 2, 4, 5, 0xB4, 1, 1, 1)), R.TCP, dict(SYNF, l4_off=20, hdr_len=28), H4),
    ("3o: NOPs, MSS on a SYN", fr(v4(6), th(28, 2), (1, 1, 1, 1, 2, 4, 5, 0xB4)), R.TCP,
     dict(SYNF, l4_off=20, hdr_len=28, mss=1460, opt=R.MSS), H4),
    ("3o: MSS without SYN", fr(v4(6), th(24), (2, 4, 5, 0xB4)), R.TCP, dict(TCPF, l4_off=20, hdr_len=24), H4),
    ("3o: WS without SYN", fr(v4(6), th(24), (3, 3, 7, 1)), R.TCP, dict(TCPF, l4_off=20, hdr_len=24), H4),
    ("3o: MSS with len 3", fr(v4(6), th(24, 2), (2, 3, 5, 1)), R.TCP, dict(SYNF, l4_off=20, hdr_len=24), H4),
    ("3o: WS 15 is 14", fr(v4(6), th(24, 2), (3, 3, 15, 1)), R.TCP, dict(SYNF, l4_off=20, hdr_len=24, wscale=14, opt=R.WS), H4),
    ("3o: WS 0 still sets the bit", fr(v4(6), th(24, 2), (3, 3, 0, 0)), R.TCP, dict(SYNF, l4_off=20, hdr_len=24, opt=R.WS), H4),
    ("3o: timestamps", fr(v4(6), th(32), (1, 1, 8, 10, 0, 0, 1, 0, 0xFF, 0, 0, 2)), R.TCP,
     dict(TCPF, l4_off=20, hdr_len=32, ts_val=256, ts_ecr=0xFF000002, opt=R.TS), H4),
    ("3o: the later timestamp wins", fr(v4(6), th(40), (8, 10, 0, 0, 0, 1, 0, 0, 0, 2, 8, 10, 0, 0, 0, 3, 0, 0, 0, 4)), R.TCP,
     dict(TCPF, l4_off=20, hdr_len=40, ts_val=3, ts_ecr=4, opt=R.TS), H4),
    ("3o: len 0", fr(v4(6), th(28, 2), (2, 4, 5, 0xB4, 6, 0, 3, 3)), R.TCP,
     dict(SYNF, l4_off=20, hdr_len=28, mss=1460, opt=R.MSS | R.OPT_BAD), H4),
    ("3o: len 1 advances one byte", fr(v4(6), th(28, 2), (5, 1, 2, 4, 5, 0xB4, 1, 1)), R.TCP,
     dict(SYNF, l4_off=20, hdr_len=28, mss=1460, opt=R.MSS), H4),
    ("3o: a kind as the area's last byte, its option behind it", fr(v4(6), th(24, 2), (1, 1, 1, 2), (4, 5, 0xB4)), R.TCP,
     dict(SYNF, l4_off=20, hdr_len=24, pay_len=3, opt=R.OPT_BAD), H4),
    ("3o: an option one byte past the area", fr(v4(6), th(32), (1, 1, 1, 8, 10, 0, 0, 0, 1, 0, 0, 0), (2,)), R.TCP,
     dict(TCPF, l4_off=20, hdr_len=32, pay_len=1, opt=R.OPT_BAD), H4),
    ("3o: an option that ends the area", fr(v4(6), th(24, 2), (2, 4, 5, 0xB4), (2, 4, 9, 9)), R.TCP,
     dict(SYNF, l4_off=20, hdr_len=24, pay_len=4, mss=1460, opt=R.MSS), H4),
    ("3o: forty NOPs", fr(v6(6), th(60, 2), (1,) * 40), R.TCP | R.IP6, dict(SYNF, l4_off=40, hdr_len=60), H6),
    ("4: m 7 (udp_usrreq.c:65-68)", fr(v4(17), uh(8))[:27], R.UDP_SHORT, dict(l4_off=20, pay_len=7), 0),
    ("4: m 8", fr(v4(17), uh(8)), R.UDP, dict(sport=SP, dport=DP, l4_off=20, hdr_len=8), H4),
    ("4: ulen 7 (no counterpart)", fr(v4(17), uh(7), (1, 2)), R.UDP_BADLEN, dict(l4_off=20, pay_len=10), 0),
    ("4: ulen m + 1 (udp_usrreq.c:75-78)", fr(v4(17), uh(11), (1, 2)), R.UDP_BADLEN, dict(l4_off=20, pay_len=10), 0),
    ("4: ulen m", fr(v6(17), uh(10), (1, 2)), R.UDP | R.IP6, dict(sport=SP, dport=DP, l4_off=40, hdr_len=8, pay_len=2), H6),
    ("4: ulen below m", fr(v4(17), uh(9), (1, 2)), R.UDP, dict(sport=SP, dport=DP, l4_off=20, hdr_len=8, pay_len=1), H4),
    ("5: ICMP", fr(v4(1), (8, 0, 0, 0)), R.ICMP, dict(l4_off=20, pay_len=4), 0),
    ("5: ICMPv6", fr(v6(58), (128, 0, 0, 0)), R.ICMP | R.IP6, dict(l4_off=40, pay_len=4), 0),
    ("5: 58 under IPv4", fr(v4(58), (128, 0, 0, 0)), R.OTHER, dict(l4_off=20, pay_len=4), 0),
    ("5: 1 under IPv6", fr(v6(1), (8, 0, 0, 0)), R.OTHER | R.IP6, dict(l4_off=40, pay_len=4), 0),
    ("5: GRE", fr(v4(47, hl=6)), R.OTHER, dict(l4_off=24), 0),
    ("5: No Next Header", fr(v6(59)), R.OTHER | R.IP6, dict(l4_off=40), 0),
)


def test_referee_rules():
    """One hand-written frame per rule; behind each frame lie bytes that would read
    as further options."""
    assert H4 == F4 ^ (F4 >> 16) ^ socket.ntohs(DP ^ SP) and H4 == l4ref.so_hash(F4, DP, SP)
    for what, f, c, fields, h in RULES:
        got = l4ref.one(f)
        want = dict.fromkeys(l4ref.FIELDS, 0)
        want.update(fields)
        assert got == (c, want, h), (what, got)
        buf = np.concatenate((np.full(9, 0x45, np.uint8), f, np.array(LB.OPTLIKE, np.uint8)))
        desc = np.array([(2, 7, len(f))], l4ref.DESC_DTYPE)
        seg, cls, hsh, count = l4ref.expect(buf, desc)
        assert cls[0] == c and hsh[0] == h and all(int(seg[x][0]) == want[x] for x in l4ref.FIELDS), what
        exp = np.zeros(12, np.uint32)
        exp[c & 15] = 1
        exp[11] = bool(c & R.IP6)
        assert np.array_equal(count, exp), what


def test_against_reference_replay(port):
    """bsd44's ip_input / tcp_input / udp_input as the oracle replays them (both
    checksum flags 0: no frame is dropped on a sum) against the referee, on the
    receive corpus behind the referee of cgck_l2_desc."""
    rng = np.random.default_rng(12)
    frames = rxcorpus.corpus(rng, port, 600, clean=False)
    buf, desc = rxcorpus.ring(frames)
    fns = port.fn_pointers()
    res, _ = port.replay_rx(fns[0], fns[1], buf.copy(), desc.view(np.uint8), len(desc), 0, 0, 0)
    raw = desc.copy()
    raw["l3_off"] = 0
    raw["ip_len"] = desc["ip_len"] + 14
    d2 = l2ref.expect(buf, raw)[0]
    seg, cls, hsh, count = l4ref.expect(buf, d2)
    accepted = short = badlen = 0
    for k, p in enumerate(frames):
        c = int(cls[k])
        assert not c & R.IP6
        m = int(d2["ip_len"][k]) - int(seg["l4_off"][k])
        if res[k] == port.R_ACCEPT and int(p[9]) == 6:
            accepted += 1
            assert c in (R.TCP, R.TCP_BADOFF, R.TCP_OFFLONG), (k, c)      # tcps_rcvbadoff is past the replay's end
        if c in (R.TCP_SHORT, R.UDP_SHORT):
            short += 1
            assert res[k] == port.R_DROP, (k, c, int(res[k]))
        if c == R.UDP_BADLEN and (int(p[seg["l4_off"][k] + 4]) << 8 | int(p[seg["l4_off"][k] + 5])) > m:
            badlen += 1
            assert res[k] == port.R_DROP, (k, c, int(res[k]))
        if c in (R.TCP, R.UDP):
            assert int(seg["pay_len"][k]) + int(seg["hdr_len"][k]) <= m
    assert accepted > 100 and short > 3
    assert all(count[c] > 0 for c in (R.TCP, R.UDP, R.ICMP, R.OTHER, R.FRAG, R.NONE, R.TCP_SHORT))


def test_hash_is_the_dst_cache_entry_hash(port):
    """The reply to a dst-cache tuple hashes to the entry's own SO_HASH: the entries
    of the oracle's thread_init_dst_cache, and SO_HASH restated from subr.h:179-180."""
    key = np.frombuffer(bytes.fromhex(load_golden("rss.json")["keys"]["freebsd"]), np.uint8).copy()
    ent = port.dst_cache(0x0A000001, 0x0A000003, 0x0A010001, 0x0A010002, socket.htons(80), 4, 1, key, 300)
    assert len(ent) > 100
    for k, e in enumerate(ent[::7]):
        raw = np.array([e]).view(np.uint8)                      # laddr, faddr, lport, fport as they lie in memory
        proto = (6, 17)[k % 2]
        l4 = fr(raw[10:12], raw[8:10], (0, 0, 0, 8, 0, 0, 0, 0, 0x50, 0x10, 0, 0, 0, 0, 0, 0)) if proto == 6 else \
            fr(raw[10:12], raw[8:10], (0, 8, 0, 0))
        p = fr(v4(proto)[:12], raw[4:8], raw[0:4], l4)              # from faddr:fport to laddr:lport
        c, r, h = l4ref.one(p)
        assert c == (R.TCP, R.UDP)[k % 2] and (r["sport"], r["dport"]) == (int(e["fport"]), int(e["lport"]))
        so = int(e["faddr"]) ^ (int(e["faddr"]) >> 16) ^ socket.ntohs(int(e["lport"]) ^ int(e["fport"]))
        assert h == int(e["hash"]) == so, (k, hex(h), hex(int(e["hash"])))


def test_constants_and_exports():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    for i, x in enumerate(l4ref.NAMES + ("NCLASS",)):
        m = re.search(rf"\bCGCK_SEG_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == i == getattr(cgck, f"SEG_{x}"), x
        if x != "NCLASS":
            assert getattr(l4ref, x) == i
    m = re.search(r"\bCGCK_SEG_IP6 = 1u << (\d+)", hdr)
    assert m and 1 << int(m.group(1)) == cgck.SEG_IP6 == l4ref.IP6 == 16
    for x, v in (("MSS", 1), ("WS", 2), ("TS", 4), ("OPT_BAD", 0x80)):
        m = re.search(rf"\bCGCK_SEG_{x} = (0x[0-9A-Fa-f]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == v == getattr(cgck, f"SEG_{x}") == getattr(l4ref, x), x
    m = re.search(r"#define CGCK_SEG_NCOUNT (\d+)", hdr)
    assert m and int(m.group(1)) == cgck.SEG_NCOUNT == l4ref.NCOUNT == 12
    # sizeof(cgck_seg_t) == 32 == SEG_DTYPE.itemsize, field by field as the header declares them
    body = re.search(r"typedef struct cgck_seg \{(.*?)\} cgck_seg_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    off, names = 0, []
    for typ, ids in re.findall(r"(uint\d+_t) ([a-z_0-9, ]+);", body):
        for name in ids.split(","):
            name = name.strip()
            assert off % size[typ] == 0
            assert cgck.SEG_DTYPE.fields[name][1] == off and cgck.SEG_DTYPE.fields[name][0].itemsize == size[typ], name
            names.append(name)
            off += size[typ]
    assert off == 32 == cgck.SEG_DTYPE.itemsize == l4ref.SEG_DTYPE.itemsize
    assert tuple(names) == cgck.SEG_DTYPE.names == l4ref.SEG_DTYPE.names
    assert ctypes.sizeof(cgck.L4Res) == 4 * ctypes.sizeof(ctypes.c_void_p)
    L = cgck.load()
    for name in ("cgck_l4_desc", "cgck_test_l4_pass"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert "#define CGCK_ABI_VERSION 2" in hdr and L.cgck_abi_version() == 2
