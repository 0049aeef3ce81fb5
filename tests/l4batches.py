"""Frames for the cgck_l4_desc tests (test_l4_cpu.py, test_gpu_l4.py,
tools/l4_ab.py): a corpus with every class under both families, every length
boundary of the contract and every rule of the option walk, in front of a plain
IP header, behind IPv4 options and behind IPv6 extension chains; layouts that put
it at a chosen start alignment between poison bytes, or tile it into 128-byte
slots; and a fuzz mix.  An item is (frame bytes, tail or None, label or None):
`tail` is written right behind the frame (what a walk that left the option area
or the frame would read: bytes that parse as a valid MSS or timestamp option),
`label` names the option rule the item stands for.  Nothing here calls the
library under test."""
import numpy as np

import ip6ref
import l4ref
import rssbatches as RB

DESC_DTYPE = l4ref.DESC_DTYPE
H, D, R, A, F = RB.H, RB.D, RB.R, RB.A, RB.F
SYN, ACK = 0x02, 0x10
TSB = (0xA1, 0xB2, 0xC3, 0xD4, 0x01, 0x02, 0x03, 0x04)        # a timestamp option's eight data bytes
TSC = (0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0x88)
# Bytes that a walk continues into happily: an MSS option, a timestamp option, a
# window scale option, NOPs.
OPTLIKE = (2, 4, 5, 0xB4, 8, 10) + TSB + (3, 3, 7, 1)
# Between the frames: the same, and the first bytes of both IP headers.
POISON = np.array(OPTLIKE + (0x45, 0x60, 4, 5, 0xB4), np.uint8)

# label: (th_flags, option area, the opt bits, mss, wscale, the timestamp's data bytes or None)
OPTION_RULES = {
    "eol_first": (SYN, (0, 2, 4, 5, 0xB4, 1, 1, 1), 0, 0, 0, None),
    "nop_run": (SYN, (1, 1, 1, 1, 2, 4, 5, 0xB4), l4ref.MSS, 1460, 0, None),
    "mss_no_syn": (ACK, (2, 4, 5, 0xB4), 0, 0, 0, None),
    "ws_no_syn": (ACK, (3, 3, 7, 1), 0, 0, 0, None),
    "mss_len3": (SYN, (2, 3, 5, 1), 0, 0, 0, None),
    "ws_15": (SYN, (3, 3, 15, 1), l4ref.WS, 0, 14, None),
    "ws_7": (SYN | ACK, (3, 3, 7, 0), l4ref.WS, 0, 7, None),
    "two_ts": (ACK, (8, 10) + TSB + (8, 10) + TSC, l4ref.TS, 0, 0, TSC),
    "mss_twice": (SYN, (2, 4, 1, 0, 2, 4, 2, 0), l4ref.MSS, 0x200, 0, None),
    "len_0": (SYN, (2, 4, 5, 0xB4, 6, 0, 3, 3), l4ref.MSS | l4ref.OPT_BAD, 1460, 0, None),
    "len_1": (SYN, (5, 1, 2, 4, 5, 0xB4, 1, 1), l4ref.MSS, 1460, 0, None),
    "kind_last": (SYN, (1, 1, 1, 2), l4ref.OPT_BAD, 0, 0, None),
    "len_last": (SYN, (1, 1, 2, 4), l4ref.OPT_BAD, 0, 0, None),
    "ends_at_off": (ACK, (1, 1, 8, 10) + TSB, l4ref.TS, 0, 0, TSB),
    "ends_past_off": (ACK, (1, 1, 1, 8, 10) + TSB[:7], l4ref.OPT_BAD, 0, 0, None),
    "ts_len_8": (ACK, (8, 8, 1, 2, 3, 4, 5, 6), 0, 0, 0, None),
    "unknown_skipped": (ACK, (30, 6, 2, 4, 5, 0xB4, 8, 10) + TSB, l4ref.TS, 0, 0, TSB),
    "nop_40": (SYN, (1,) * 40, 0, 0, 0, None),
    "all_40": (SYN, (2, 4, 0x23, 0x28, 3, 3, 9, 8, 10) + TSC + (30, 23) + (2,) * 21,
               l4ref.MSS | l4ref.WS | l4ref.TS, 0x2328, 9, TSC),
    "ts_then_bad": (ACK, (8, 10) + TSB + (4, 3), l4ref.TS | l4ref.OPT_BAD, 0, 0, TSB),
}


def tcp(rng, th=20, flags=ACK, opts=(), pay=0, n=None, paybytes=None):
    """A TCP segment: data offset th (bytes, as written: 16 and 64 - 4 are legal
    here), the option area, `pay` payload bytes; n: cut (or extend) to n bytes."""
    total = th + pay if n is None else n
    t = rng.integers(0, 256, max(total, 20 + len(opts)), dtype=np.uint8)
    t[12] = (th // 4) << 4 | (int(t[12]) & 15)
    t[13] = flags
    t[20:20 + len(opts)] = opts
    if paybytes is not None and total > th:
        t[th:total] = np.resize(np.array(paybytes, np.uint8), total - th)
    return t[:total]


def udp(rng, ulen, n):
    """A UDP datagram of n bytes whose length field says ulen."""
    u = rng.integers(0, 256, max(n, 8), dtype=np.uint8)
    u[4], u[5] = ulen >> 8, ulen & 255
    return u[:n]


def ip4(rng, l4, proto, hl=5, frag=0, n=None):
    h = rng.integers(0, 256, 4 * max(hl, 5), dtype=np.uint8)     # hl below 5: the header byte lies
    ln = len(h) + len(l4)
    h[0] = 0x40 | hl
    h[2], h[3] = ln >> 8, ln & 255
    h[6], h[7] = frag >> 8, frag & 255
    h[9] = proto
    p = np.concatenate((h, np.asarray(l4, np.uint8)))
    return p if n is None else p[:n]


def ip6(rng, l4, nh, chain=()):
    ln = 40 + sum(b for _, b in chain) + len(l4)
    p = ip6ref.packet(rng, ln, nh, chain)
    p[ln - len(l4):] = l4
    return p


def both(rng, l4, proto):
    """The transport bytes behind a plain header of each family."""
    return [(ip4(rng, l4, proto), None, None), (ip6(rng, l4, proto), None, None)]


def classes(rng):
    """The class corpus: a list of items."""
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    out = []
    # TCP and its length rules: m = 19 / 20, off = 16, 20, 60, off == m, off == m + 4
    for l4 in (tcp(rng), tcp(rng, pay=100), tcp(rng, 32, ACK, (1, 1, 8, 10) + TSB, pay=10),
               tcp(rng, n=19), tcp(rng, n=0), tcp(rng, n=1), tcp(rng, th=16, pay=24), tcp(rng, th=0, pay=40),
               tcp(rng, th=60, opts=(1,) * 40), tcp(rng, th=60, opts=(1,) * 40, pay=1), tcp(rng, th=60, n=59),
               tcp(rng, th=24, n=20), tcp(rng, th=44, n=40), tcp(rng, th=40, n=40), tcp(rng, th=28, pay=1400)):
        out += both(rng, l4, 6)
    # UDP: m = 7 / 8, ulen = 7, 8, m, m + 1
    for l4 in (udp(rng, 8, 8), udp(rng, 8, 7), udp(rng, 8, 0), udp(rng, 7, 8), udp(rng, 7, 40), udp(rng, 8, 40),
               udp(rng, 40, 40), udp(rng, 41, 40), udp(rng, 0, 40), udp(rng, 0xFFFF, 40), udp(rng, 39, 40),
               udp(rng, 1400, 1400)):
        out += both(rng, l4, 17)
    # ICMP is 1 under IPv4 and 58 under IPv6 only; other protocols
    for pr in (1, 58, 47, 132, 0xFF):
        out += [(ip4(rng, rnd(28), pr), None, None), (ip6(rng, rnd(28), pr), None, None)]
    out += [(ip4(rng, (), 1), None, None), (ip6(rng, (), 58), None, None), (ip6(rng, rnd(8), 59), None, None)]
    # fragments by rssf's definition; DF alone and the reserved bit alone are none
    for fr in (0x2000, 0x00B9, 0x3FFF, 0x6000):
        out += [(ip4(rng, tcp(rng, pay=8), 6, frag=fr), None, None), (ip4(rng, udp(rng, 16, 16), 17, 6, frag=fr), None, None)]
    for fr in (0x4000, 0x8000, 0xC000):
        out += [(ip4(rng, tcp(rng, pay=8), 6, frag=fr), None, None), (ip4(rng, udp(rng, 16, 16), 17, frag=fr), None, None)]
    out += [(ip6(rng, tcp(rng, pay=8), 6, ((F, 8),)), None, None), (ip6(rng, udp(rng, 16, 16), 17, ((H, 8), (F, 8))), None, None),
            (ip6(rng, (), 6, ((D, 16), (F, 8)))[:56], None, None)]
    # NONE: no frame, short headers, other versions, chains cut or too long
    out += [(rnd(0), None, None), (ip4(rng, tcp(rng), 6)[:19], None, None), (ip4(rng, tcp(rng), 6, hl=4), None, None),
            (ip4(rng, tcp(rng), 6, hl=0), None, None), (ip4(rng, (), 6, hl=6)[:23], None, None),
            (ip4(rng, (), 17, hl=15)[:40], None, None), (ip6(rng, tcp(rng), 6)[:39], None, None),
            (ip6(rng, tcp(rng), 6)[:1], None, None), (ip6(rng, tcp(rng), 6, ((H, 8), (D, 16)))[:49], None, None),
            (ip6(rng, tcp(rng), 6, ((H, 16),))[:50], None, None),
            (ip6(rng, tcp(rng), 6, ((H, 8),) + ((D, 8),) * 8), None, None)]
    for v in (0, 1, 5, 7, 15):
        p = ip4(rng, tcp(rng), 6)
        p[0] = v << 4 | 5
        out.append((p, None, None))
    # IPv4 options (hl 24 and 60) and IPv6 chains (one and eight headers; a ninth is above)
    for hl in (6, 15):
        out += [(ip4(rng, tcp(rng, pay=5), 6, hl), None, None), (ip4(rng, tcp(rng, 60, SYN, (1,) * 40, pay=3), 6, hl), None, None),
                (ip4(rng, tcp(rng, n=19), 6, hl), None, None), (ip4(rng, tcp(rng, th=24, n=20), 6, hl), None, None),
                (ip4(rng, udp(rng, 12, 12), 17, hl), None, None), (ip4(rng, udp(rng, 13, 12), 17, hl), None, None),
                (ip4(rng, udp(rng, 8, 7), 17, hl), None, None), (ip4(rng, rnd(8), 1, hl), None, None),
                (ip4(rng, (), 6, hl), None, None)]
    for ch in (((H, 8),), ((A, 12),), ((H, 8),) + ((D, 8),) * 7, ((R, 24), (D, 2048), (A, 1024))):
        out += [(ip6(rng, tcp(rng, pay=5), 6, ch), None, None), (ip6(rng, tcp(rng, 60, SYN, (1,) * 40, pay=3), 6, ch), None, None),
                (ip6(rng, tcp(rng, n=19), 6, ch), None, None), (ip6(rng, tcp(rng, th=16, pay=8), 6, ch), None, None),
                (ip6(rng, udp(rng, 12, 12), 17, ch), None, None), (ip6(rng, udp(rng, 7, 12), 17, ch), None, None),
                (ip6(rng, rnd(8), 58, ch), None, None), (ip6(rng, (), 17, ch), None, None)]
    # every option rule: the frame ends with the option area (the tail lies behind
    # it in memory), or option-like payload follows inside the frame; in front of
    # plain headers, behind IPv4 options and behind an IPv6 chain
    for label, (flags, opts, *_) in OPTION_RULES.items():
        assert len(opts) % 4 == 0 and len(opts) <= 40, label
        th = 20 + len(opts)
        for pay, tail in ((0, OPTLIKE), (13, None)):
            for wrap in (lambda t: ip4(rng, t, 6), lambda t: ip6(rng, t, 6), lambda t: ip4(rng, t, 6, 15),
                         lambda t: ip6(rng, t, 6, ((D, 16),))):
                out.append((wrap(tcp(rng, th, flags, opts, pay, paybytes=OPTLIKE[1:])), tail, label))
    # a header that ends the frame, option bytes behind it
    out += [(ip4(rng, tcp(rng, 20, SYN), 6), OPTLIKE, None), (ip6(rng, tcp(rng, 20, SYN), 6), OPTLIKE, None),
            (ip4(rng, udp(rng, 8, 8), 17), OPTLIKE, None)]
    return [out[i] for i in rng.permutation(len(out))]


def tags(item):
    """The classes and boundaries an item stands for, read from its bytes (the
    option rule from its label)."""
    f, tail, label = item
    n = len(f)
    c, r, h = l4ref.one(f)
    fam = "v6" if c & l4ref.IP6 else "v4" if n and int(f[0]) >> 4 == 4 else "other"
    name = l4ref.NAMES[c & 15]
    t = {f"cls_{name}_{fam}"}
    if n == 0:
        t.add("len_0")
    if (c & 15) == l4ref.NONE:
        if fam == "v6" and n >= 40:
            t.add("v6_bad_" + str(RB.bad6(f)))
        return t
    off, m = r["l4_off"], n - r["l4_off"]
    if fam == "v4":
        t.add(f"v4_hl{off}")
        fo = int(f[6]) << 8 | int(f[7])
        t |= {f"v4_fo_{fo:04x}"} & {"v4_fo_4000", "v4_fo_8000", "v4_fo_2000"}
    else:
        ext, o, nh = 0, 40, int(f[6])
        while nh in (0, 43, 60, 51) and o < off:
            if nh == 51:
                t.add("v6_ah")
            nh, o, ext = int(f[o]), o + ((int(f[o + 1]) + 2) * 4 if nh == 51 else (int(f[o + 1]) + 1) * 8), ext + 1
        t.add(f"v6_ext{ext}")
    if name.startswith("TCP"):
        t |= {f"tcp_m{m}"} & {"tcp_m0", "tcp_m19", "tcp_m20"}
        if m >= 20:
            th = (int(f[off + 12]) >> 4) * 4
            t |= {f"off_{th}"} & {"off_0", "off_16", "off_20", "off_60"}
            if th == m:
                t.add("off_eq_m")
            if th == m + 4:
                t.add("off_m_plus4")
            if name == "TCP":
                t.add("tcp_first_round" if off + th <= 80 else "tcp_second_round")
                if r["opt"] & l4ref.OPT_BAD:
                    t.add("opt_bad")
                if tail is not None and th == m:
                    t.add("area_ends_frame_tail")
        if label:
            t.add(f"opt_{label}")
    if name.startswith("UDP"):
        t |= {f"udp_m{m}"} & {"udp_m0", "udp_m7", "udp_m8"}
        if m >= 8:
            ulen = int(f[off + 4]) << 8 | int(f[off + 5])
            t |= {f"ulen_{ulen}"} & {"ulen_0", "ulen_7", "ulen_8", "ulen_65535"}
            if ulen == m:
                t.add("ulen_m")
            if ulen == m + 1:
                t.add("ulen_m_plus1")
            if 8 <= ulen < m:
                t.add("ulen_below_m")
            if name == "UDP":
                t.add("udp_first_round" if off + 8 <= 80 else "udp_second_round")
    return t


REQUIRED = ({f"cls_{x}_{f}" for x in l4ref.NAMES for f in ("v4", "v6")} | {"cls_NONE_other", "len_0"} |
            {f"opt_{x}" for x in OPTION_RULES} |
            {"v4_hl20", "v4_hl24", "v4_hl60", "v6_ext0", "v6_ext1", "v6_ext8", "v6_bad_ninth", "v6_bad_cut", "v6_bad_past",
             "v6_ah", "v4_fo_4000", "v4_fo_8000", "v4_fo_2000",
             "tcp_m0", "tcp_m19", "tcp_m20", "off_0", "off_16", "off_20", "off_60", "off_eq_m", "off_m_plus4",
             "udp_m0", "udp_m7", "udp_m8", "ulen_0", "ulen_7", "ulen_8", "ulen_65535", "ulen_m", "ulen_m_plus1",
             "ulen_below_m", "tcp_first_round", "tcp_second_round", "udp_first_round", "udp_second_round", "opt_bad",
             "area_ends_frame_tail"})


def poison(n, phase=0):
    return np.resize(np.roll(POISON, -phase), n)


def lay(items, align):
    """(buf, desc): every frame starts at a byte with (offset & 15) == align, with
    its tail right behind it and poison around both; l3_off varies; the last frame
    ends on the buffer's last byte."""
    order = sorted(range(len(items)), key=lambda i: (items[i][1] is None, len(items[i][0]) > 0))
    assert items[order[-1]][1] is None and len(items[order[-1]][0]) > 0
    pos, at = 0, []
    for i in order:
        f, tail, _ = items[i]
        l3 = (5 * i) % 23
        pos = max(pos + 1, l3)
        pos += (align - pos) % 16
        at.append((i, pos, l3))
        pos += len(f) + (len(tail) if tail is not None else 0)
    last = at[-1][1] + len(items[order[-1]][0])
    assert last == max(p + len(items[i][0]) for i, p, _ in at)
    buf = poison(last, 3)
    desc = np.zeros(len(items), DESC_DTYPE)
    for i, p, l3 in at:
        f, tail, _ = items[i]
        buf[p:p + len(f)] = f
        if tail is not None:
            buf[p + len(f):p + len(f) + len(tail)] = tail
        desc[i] = (p - l3, l3, len(f))
    return buf, desc


def tiled(items, n, slot=128):
    """n frames in `slot`-byte slots, tiled from the items that fit one with their
    tail (l3_off 0): (buf, desc, m), m the period in frames."""
    fit = [(f, tail) for f, tail, _ in items if len(f) + (len(tail) if tail is not None else 0) <= slot]
    m = len(fit)
    block = poison(m * slot, 7)
    lens = np.zeros(m, np.int64)
    for j, (f, tail) in enumerate(fit):
        block[j * slot:j * slot + len(f)] = f
        if tail is not None:
            block[j * slot + len(f):j * slot + len(f) + len(tail)] = tail
        lens[j] = len(f)
    reps = -(-n // m)
    buf = np.tile(block, reps)[:n * slot]
    desc = np.zeros(n, DESC_DTYPE)
    desc["frame_off"] = np.arange(n, dtype=np.uint64) * slot
    desc["ip_len"] = np.tile(lens, reps)[:n]
    return buf, desc, m


def expect_tiled(buf, desc, m):
    """l4ref.expect over one period, repeated: the frames of a tiled burst differ
    only in frame_off.  (seg, cls, hash, count)."""
    n = len(desc)
    s1, c1, h1, _ = l4ref.expect(buf, desc[:min(m, n)])
    reps = -(-n // m)
    cls = np.tile(c1, reps)[:n]
    return np.tile(s1, reps)[:n], cls, np.tile(h1, reps)[:n], counts(cls)


counts = l4ref.counts


def soup(rng, n):
    """n option-area bytes drawn from the kinds and lengths the walk tells apart."""
    alphabet = np.array((0, 1, 1, 1, 2, 3, 4, 8, 10, 30, 5, 0xB4, 6, 12, 40), np.uint8)
    o = alphabet[rng.integers(0, len(alphabet), n)]
    k = rng.integers(0, 4)
    if k == 0 and n >= 4:
        o[:4] = (2, 4, 5, 0xB4)
    elif k == 1 and n >= 12:
        o[:12] = (1, 1, 8, 10) + TSB
    return o


def fuzz(rng, n):
    """n frames: a third rssbatches.fuzz's mix (random bytes behind IP headers of
    every shape), a third TCP segments with a random data offset and an option soup
    behind headers of both families, with and without IP options and chains, and a
    third UDP / short / cut frames."""
    out = list(RB.fuzz(rng, n // 3))
    while len(out) < n:
        c = int(rng.integers(0, 100))
        if c < 55:
            th = 4 * int(rng.integers(4, 16))
            pay = int(rng.choice((0, 0, 1, 7, 40, 500)))
            l4 = tcp(rng, th, int(rng.integers(0, 64)), soup(rng, max(th - 20, 0)), pay, paybytes=OPTLIKE)
            if rng.integers(0, 6) == 0:
                l4 = l4[:int(rng.integers(0, len(l4) + 1))]
            pr = 6
        else:
            m = int(rng.choice((0, 7, 8, 9, 40, 300)))
            l4 = udp(rng, int(rng.choice((0, 7, 8, m, m + 1, max(m - 1, 0), 0xFFFF))), m)
            pr = 17
        k = int(rng.integers(0, 6))
        if k < 2:
            p = ip4(rng, l4, pr, frag=int(rng.choice((0, 0, 0, 0x4000, 0x2000))))
        elif k == 2:
            p = ip4(rng, l4, pr, int(rng.integers(6, 16)))
        elif k < 5:
            p = ip6(rng, l4, pr)
        else:
            p = ip6(rng, l4, pr, tuple((int(rng.choice((H, R, D, A))), 8 * int(rng.integers(1, 4)))
                                       for _ in range(int(rng.integers(1, 4)))))
        out.append(p)
    return [out[i] for i in rng.permutation(len(out))]
