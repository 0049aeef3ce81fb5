"""Inputs for the cgck_l4_reply tests: a deterministic corpus of received frames with
the records, class bytes, lookup kinds, verdicts and L2 class bytes the stages before
the reply rule would hand over, the (vmask, flags) pairs it runs under, and the IPv4
burst that goes through the reference stack's replay.  The frames are written here
byte by byte (IPv4 options and an IPv6 extension chain included) and read back by
cgck_l4_desc's referee (tests/l4ref.py), so the records are the receive pipeline's.
Expectations come from tests/l4rref.py; nothing here calls the library."""
import numpy as np

import l4bref
import l4ref
import l4rref as R
import rxcorpus

DESC_DTYPE = l4bref.DESC_DTYPE
V4_SRC, V4_DST = bytes([10, 9, 0, 7]), bytes([10, 0, 0, 2])
V6_SRC = bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(range(1, 13))
V6_DST = bytes([0xfd, 0x00]) + bytes(range(101, 115))
V4_MCAST, V6_MCAST = bytes([224, 0, 0, 251]), bytes([0xFF, 0x02]) + bytes(13) + bytes([0xFB])
PAY_MAX = 65495                                         # 65535 - 20 - 20: the longest IPv4 TCP payload
# (vmask, flags) of the calls the corpus runs under: both policies at 2, the two flags apart and together
CONFIGS = ((7, 0), (4, R.NO_RST), (5, R.NO_MCAST), (0, R.NO_RST | R.NO_MCAST), (6, 0))
LINK = np.zeros(1, R.FLOW_DTYPE)[0]
LINK["eth_dst"], LINK["eth_src"], LINK["vlan_tci"], LINK["ttl"] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2), 0x2345, 64
LINK["flags"] = R.FLOW_VLAN | R.FLOW_IP6                # the template's IP6 bit is ignored
LINK["laddr"], LINK["faddr"] = 0xAA, 0xBB               # and so are its addresses


def be(v, n):
    return [(v >> (8 * (n - 1 - i))) & 255 for i in range(n)]


def tcp_hdr(rng, sport, dport, seq, ack, th, off=5):
    t = be(sport, 2) + be(dport, 2) + be(seq, 4) + be(ack, 4) + [off << 4, th] + be(int(rng.integers(0, 65536)), 2) + [0] * 4
    return t + [1] * (4 * off - 20)                     # NOPs


def frame(rng, six, th, seq, ack, pay, src=None, dst=None, opts=False, sport=40000, dport=81):
    """The bytes of one TCP datagram: IPv4 (opts: ihl 7) or IPv6 (opts: a Hop-by-Hop and
    a Destination Options header in front of TCP); TCP with th_off 6 under opts."""
    t = tcp_hdr(rng, sport, dport, seq, ack, th, 6 if opts else 5) + [int(x) for x in rng.integers(0, 256, pay)]
    if six:
        src, dst = src or V6_SRC, dst or V6_DST
        ext = [60, 0, 1, 4, 0, 0, 0, 0, 6, 0, 1, 4, 0, 0, 0, 0] if opts else []      # HbH -> DstOpts -> TCP, PadN
        ip = [0x60, 0, 0, 0] + be(len(ext) + len(t), 2) + [0 if opts else 6, 64] + list(src) + list(dst) + ext
    else:
        src, dst = src or V4_SRC, dst or V4_DST
        ihl = 7 if opts else 5
        ip = [0x40 | ihl, 0] + be(4 * ihl + len(t), 2) + be(int(rng.integers(0, 65536)), 2) + [0x40, 0, 64, 6, 0, 0] + \
            list(src) + list(dst) + [1] * (4 * ihl - 20)
    return np.array(ip + t, np.uint8)


def specs(rng):
    """[(tag, frame kwargs, modifiers)]: modifiers name a selector byte (cls, kind, verdict,
    l2cls), the descriptor's ip_len (len) or the version byte (ver) to override."""
    out = []
    rnd = lambda: int(rng.integers(0, 2 ** 32))
    for six in (False, True):
        for i, th in enumerate((0x02, 0x10, 0x12, 0x18, 0x04, 0x14, 0x00, 0x11, 0x03, 0x29)):
            out.append((f"flags {th:#04x}", dict(six=six, th=th, seq=rnd(), ack=rnd(), pay=(0, 1, 40)[i % 3]), {}))
        out += [("wrap", dict(six=six, th=0x02, seq=0xFFFFFFF0, ack=rnd(), pay=40), {}),
                ("wrap to 0", dict(six=six, th=0x00, seq=0xFFFFFFD8, ack=rnd(), pay=40), {}),
                ("options", dict(six=six, th=0x02, seq=rnd(), ack=rnd(), pay=3, opts=True), {}),
                ("options, ACK", dict(six=six, th=0x10, seq=rnd(), ack=rnd(), pay=0, opts=True), {})]
        base = dict(six=six, th=0x12, seq=rnd(), ack=rnd(), pay=0)
        syn = dict(six=six, th=0x02, seq=rnd(), ack=rnd(), pay=2)
        out += [("skip", base, {"cls": c}) for c in (1, 2, 5, 6, 15, 0x11)]
        out += [("clsflags", syn, {"clsor": 0xE0})]                                    # only the low nibble of cls counts
        out += [("notmiss", base, {"kind": kd}) for kd in (0, 1, 3, 4, 0xFF)]
        out += [("verdict", syn, {"verdict": vd}) for vd in (1, 2, 4, 8, 3, 7, 0xF8)]
        out += [("l2 mcast", base, {"l2cls": 0x80 | int(six)}), ("l2 bcast", syn, {"l2cls": 0x40 | int(six)}),
                ("l2 vlan", syn, {"l2cls": 0x10 | int(six)}),
                ("mcast dst", dict(base, dst=V6_MCAST if six else V4_MCAST), {}),
                ("mcast dst, RST", dict(base, th=0x04, dst=V6_MCAST if six else V4_MCAST), {}),
                ("near mcast", dict(syn, dst=bytes([0xFE]) + V6_DST[1:] if six else bytes([240, 0, 0, 1])), {}),
                ("mcast src", dict(syn, src=V6_MCAST if six else V4_MCAST), {})]
        full = 40 if six else 20
        out += [("none:len0", base, {"len": 0}), ("none:short", syn, {"len": full - 1}), ("exact", syn, {"len": full}),
                ("none:version", base, {"ver": 0x55}), ("none:version", syn, {"ver": 0x0F if six else 0x75}),
                ("skip before none", base, {"len": 0, "cls": 5}), ("notmiss before dropped", base, {"kind": 0, "verdict": 7}),
                ("dropped before none", base, {"len": 3, "verdict": 4})]
    out += [("none:v6as20", dict(six=True, th=0x02, seq=rnd(), ack=rnd(), pay=0), {"len": 20}),
            ("v4 turned v6", dict(six=False, th=0x10, seq=rnd(), ack=rnd(), pay=40), {"ver": 0x60}),    # 60 bytes: v == 6 reads b[8..40)
            ("max payload", dict(six=False, th=0x02, seq=0xFFFF0000, ack=rnd(), pay=PAY_MAX), {})]
    return out


class Burst:
    """buf, desc, seg and the four selector arrays; tags names each frame."""

    def sel(self, drop=()):
        return {x: None if x in drop else getattr(self, x) for x in ("cls", "kind", "verdict", "l2cls")}


def burst(sp, rng, align=None):
    """The frames of `sp` behind one another, each IP header at a 16-byte boundary + its
    index (or + align), the bytes between them random; records and class bytes by l4ref
    over the whole frames, then the modifiers."""
    n = len(sp)
    frames = [frame(rng, **kw) for _, kw, _ in sp]
    desc = np.zeros(n, DESC_DTYPE)
    at = 0
    for k, p in enumerate(frames):
        l3 = 14 + ((k if align is None else align) - 14) % 16
        desc[k] = (at, l3, len(p))
        at += (l3 + len(p) + 15) // 16 * 16
    buf = rng.integers(0, 256, at, dtype=np.uint8)
    for k, p in enumerate(frames):
        o = int(desc["frame_off"][k]) + int(desc["l3_off"][k])
        buf[o:o + len(p)] = p
    seg, cls, _, _ = l4ref.expect(buf, desc)
    assert np.all((cls & 15) == l4ref.TCP)
    b = Burst()
    b.kind = np.full(n, R.PCB_MISS, np.uint8)
    b.verdict = np.zeros(n, np.uint8)
    b.l2cls = np.array([int(kw["six"]) for _, kw, _ in sp], np.uint8)       # L2_IP4 / L2_IP6, no flags
    for k, (_, _, mod) in enumerate(sp):
        for x, v in mod.items():
            if x == "len":
                desc["ip_len"][k] = v
            elif x == "ver":
                buf[int(desc["frame_off"][k]) + int(desc["l3_off"][k])] = v
            elif x == "clsor":
                cls[k] |= v
            elif x == "cls":
                cls[k] = v
            else:
                getattr(b, x)[k] = v
    b.buf, b.desc, b.seg, b.cls, b.tags = buf, desc, seg, cls, [s[0] for s in sp]
    return b


def corpus(seed=61):
    rng = np.random.default_rng(seed)
    return burst(specs(rng), rng)


def tiled(b, n):
    """Burst b repeated to n frames whose descriptors alias b's bytes: a Burst over b.buf."""
    k = np.arange(n) % len(b.desc)
    t = Burst()
    t.buf, t.desc, t.seg = b.buf, b.desc[k].copy(), b.seg[k].copy()
    t.cls, t.kind, t.verdict, t.l2cls = b.cls[k].copy(), b.kind[k].copy(), b.verdict[k].copy(), b.l2cls[k].copy()
    return t


def tail_burst(align, six, rng):
    """Three frames whose IP headers start at `align` mod 16; the last has ip_len 20 (40
    for IPv6) and ends the buffer: its last address byte is the allocation's last."""
    rnd = lambda: int(rng.integers(0, 2 ** 32))
    sp = [("first", dict(six=six, th=0x02, seq=rnd(), ack=rnd(), pay=1), {}),
          ("other family", dict(six=not six, th=0x10, seq=rnd(), ack=rnd(), pay=0), {}),
          ("last", dict(six=six, th=0x18, seq=rnd(), ack=rnd(), pay=5), {})]
    b = burst(sp, rng, align)
    n = 40 if six else 20
    b.desc["ip_len"][2] = n
    b.buf = b.buf[:int(b.desc["frame_off"][2]) + int(b.desc["l3_off"][2]) + n].copy()
    return b


# -- the IPv4 burst of the replay ------------------------------------------------------------

def replay_frames(rng, ck):
    """TCP-only IPv4 datagrams for addresses inside rxcorpus.LADDR, none a fragment: good
    ones of every flag mix (IP options and TCP options among them), and ones with a bad
    header sum, a bad TCP sum, both, a segment shorter than a TCP header, and a data
    offset below 5 or past the segment.  [(kind, bytes)]."""
    out = []
    for k in range(60):
        off = (5, 5, 6, 8, 15)[k % 5]
        th = (0x02, 0x10, 0x12, 0x18, 0x11, 0x00, 0x01, 0x03, 0x04, 0x14)[k % 10]
        dst = rxcorpus.LADDR[0] + k % 4
        kind = ("good", "good", "good", "bad ip", "good", "bad l4", "short", "good", "bad off", "both", "off long")[k % 11]
        l4 = 4 * off + (0, 1, 333)[k % 3]
        if kind == "short":
            l4, off = 14 + k % 6, 5
        if kind == "off long":
            l4, off = 24, 7

        def pre(p, hl, dst=dst, th=th, l4=l4, kind=kind):
            p[16:20] = [(dst >> s) & 255 for s in (24, 16, 8, 0)]
            if l4 >= 14:
                p[hl + 13] = th
            if kind == "bad off":
                p[hl + 12] = 0x40 | (int(p[hl + 12]) & 15)
        p = rxcorpus.frame(rng, ck, 6, l4, ihl=(5, 5, 7)[k % 3], tcp_off=off, pre=pre)
        hl = 4 * (int(p[0]) & 15)
        if kind in ("bad ip", "both"):
            p[8] ^= 0x10                                # ttl: not an address, not a length
        if kind in ("bad l4", "both"):
            p[hl + 4] ^= 0x01                           # seq
        out.append((kind, p))
    return out
