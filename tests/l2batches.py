"""Raw Ethernet frames for the cgck_l2_desc tests (test_l2_cpu.py,
test_gpu_l2.py, tools/l2_ab.py): a corpus with every class behind 0, 1 and 2 VLAN
tags of both TPIDs, a third tag, each flag and every length boundary of the
contract; layouts that put it at a chosen start alignment between poison bytes, or
tile it into 64-byte slots; and the Python restatement of cgck_synth_eth.  An
item is (frame bytes, l3_off or None): l3_off is the Ethernet header's offset in
its slot where the test needs a particular one (the 16-bit bound of rule 8).
Nothing here calls the library under test."""
import numpy as np

import l2ref

DESC_DTYPE = l2ref.DESC_DTYPE
T1, T2 = 0x8100, 0x88A8
TAGSETS = ((), (T1,), (T2,), (T1, T1), (T2, T1), (T2, T2))
BCAST_DST = (0xFF,) * 6
# What a lane that looked outside its frame would find: a tag, an IPv4 ethertype
# and header start, an IPv6 ethertype and header start, broadcast bytes.
POISON = np.array((0x81, 0x00, 0x08, 0x00, 0x45, 0x00, 0x00, 0x14, 0x86, 0xDD, 0x60, 0xFF, 0xFF, 0xFF, 0x88, 0xA8,
                   0x08, 0x06, 0x45), np.uint8)


def be16(v):
    return ((v >> 8) & 255, v & 255)


def eth(rng, et, body, tags=(), dst=None, cut=None):
    """dst (default: a random unicast address), a random source, the tags (TPID and
    a random TCI each), the ethertype and the body; cut: keep only the first bytes."""
    d = rng.integers(0, 256, 6, dtype=np.uint8) if dst is None else np.array(dst, np.uint8)
    if dst is None:
        d[0] &= 0xFE
    parts = [d, rng.integers(0, 256, 6, dtype=np.uint8)]
    for tp in tags:
        parts += [np.array(be16(tp), np.uint8), rng.integers(0, 256, 2, dtype=np.uint8)]
    parts += [np.array(be16(et), np.uint8), np.asarray(body, np.uint8)]
    f = np.concatenate(parts)
    return f if cut is None else f[:cut]


def ip4(rng, total, n=None, hl=5, ver=4):
    """n (default total) random bytes with the IPv4 version / header length byte and
    the total-length field set."""
    n = total if n is None else n
    p = rng.integers(0, 256, max(n, 4), dtype=np.uint8)
    p[0] = ver << 4 | hl
    p[2], p[3] = be16(total)
    return p[:n]


def ip6(rng, plen, n=None, ver=6):
    n = 40 + plen if n is None else n
    p = rng.integers(0, 256, max(n, 6), dtype=np.uint8)
    p[0] = ver << 4 | (int(p[0]) & 15)
    p[4], p[5] = be16(plen)
    return p[:n]


def classes(rng):
    """The class corpus: a list of items."""
    out = []
    for tg in TAGSETS:
        def e4(body, tg=tg):
            return eth(rng, 0x0800, body, tg), None

        def e6(body, tg=tg):
            return eth(rng, 0x86DD, body, tg), None

        out += [e4(ip4(rng, 40)), e4(ip4(rng, 40, 41)), e4(ip4(rng, 40, 46)), e4(ip4(rng, 20)),          # IP4
                e4(ip4(rng, 24, 24, hl=6)), e4(ip4(rng, 60, 64, hl=15)),
                e4(ip4(rng, 40, 19)), e4(ip4(rng, 40, 0)),                                               # TOOSMALL
                e4(ip4(rng, 40, ver=5)), e4(ip4(rng, 60, ver=6)), e4(ip4(rng, 40, ver=0)),               # BADVERS
                e4(ip4(rng, 40, hl=4)), e4(ip4(rng, 40, hl=0)), e4(ip4(rng, 24, 23, hl=6)),              # BADHLEN
                e4(ip4(rng, 60, 40, hl=15)),
                e4(ip4(rng, 19, 40)), e4(ip4(rng, 0, 40)), e4(ip4(rng, 23, 40, hl=6)),                   # BADLEN
                e4(ip4(rng, 41, 40)), e4(ip4(rng, 0xFFFF, 46)), e4(ip4(rng, 25, 24, hl=6)),              # TOOSHORT
                e6(ip6(rng, 20)), e6(ip6(rng, 20, 61)), e6(ip6(rng, 0)), e6(ip6(rng, 0, 46)),            # IP6
                e6(ip6(rng, 20, 39)), e6(ip6(rng, 0, 5)),                                                # TOOSMALL
                e6(ip6(rng, 20, ver=4)), e6(ip6(rng, 0, ver=7)),                                         # BADVERS
                e6(ip6(rng, 20, 59)), e6(ip6(rng, 1, 40)), e6(ip6(rng, 0xFFFF, 60)),                     # TOOSHORT
                (eth(rng, 0x0806, rng.integers(0, 256, 28, dtype=np.uint8), tg), None),                 # ARP
                (eth(rng, 0x0806, (), tg), None),
                (eth(rng, 0x88CC, rng.integers(0, 256, 46, dtype=np.uint8), tg), None),                 # OTHER
                (eth(rng, 0x002E, ip4(rng, 46), tg), None),                                             # 802.3 length
                (eth(rng, 0x0800, ip4(rng, 40), tg, dst=BCAST_DST), None),                              # flags
                (eth(rng, 0x86DD, ip6(rng, 8), tg, dst=(0x33, 0x33, 0, 0, 0, 1)), None),
                (eth(rng, 0x0800, ip4(rng, 40), tg, dst=(0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE)), None),
                (eth(rng, 0x0806, ip4(rng, 28), tg, dst=(0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF)), None),
                (eth(rng, 0x0806, ip4(rng, 28), tg, dst=BCAST_DST), None)]
        if len(tg) < 2:
            h = 14 + 4 * len(tg)
            for tp in (T1, T2):      # a TPID with no room for its tag: L = off, off + 3 (off = h)
                out += [(eth(rng, tp, ip4(rng, 40), tg, cut=h + c), None) for c in (0, 3)]
                out += [(eth(rng, tp, ip4(rng, 40), tg, cut=h + 3, dst=BCAST_DST), None)]
        else:                        # a third tag
            out += [(eth(rng, tp, ip4(rng, 40), tg), None) for tp in (T1, T2)]
    out += [(eth(rng, 0x0800, ip4(rng, 40), cut=c), None) for c in (0, 1, 12, 13, 14)]                   # L around 14
    out += [(eth(rng, 0x0800, ip4(rng, 40), cut=13, dst=BCAST_DST), None)]
    # rule 8: the last l3_off whose l3_off + off fits 16 bits, and the first that does not
    out += [(eth(rng, 0x0800, ip4(rng, 40)), 65535 - 14), (eth(rng, 0x0800, ip4(rng, 40)), 65535 - 13),
            (eth(rng, 0x86DD, ip6(rng, 4), (T1,)), 65535 - 18), (eth(rng, 0x86DD, ip6(rng, 4), (T1,)), 65535 - 17),
            (eth(rng, 0x0806, ip4(rng, 28), (T2, T1), dst=BCAST_DST), 65535 - 22),
            (eth(rng, 0x0806, ip4(rng, 28)), 65535)]
    return [out[i] for i in rng.permutation(len(out))]


def tags(item):
    """The classes and boundaries an item stands for, read from its bytes."""
    f, l3 = item
    L = len(f)
    c, flags, off, ip_len = l2ref.one(f, L, l3 or 0)
    nt = (off - 14) // 4
    t = {f"cls_{l2ref.NAMES[c]}", f"L{L}" if L <= 14 else "L>14"}
    if L < 14:
        return t
    t.add("bcast" if flags & l2ref.BCAST else "mcast" if flags & l2ref.MCAST else "ucast")
    if flags & l2ref.VLAN:
        t.add("vlan")
    ets = [int(f[12 + 4 * i]) << 8 | int(f[13 + 4 * i]) for i in range(3) if L >= 14 + 4 * i]
    if c == l2ref.RUNT and (l3 or 0) + off <= 65535:
        t.add(f"runt_tag{nt + 1}_L{L - off}")                     # L = off .. off + 3
    elif c == l2ref.RUNT:
        t.add(f"runt_l3_tags{nt}")
    else:
        t.add(f"{l2ref.NAMES[c]}_tags{nt}")
        if l3 is not None and l3 + off == 65535:
            t.add(f"l3_fits_tags{nt}")
        for e in ets[:nt]:
            t.add(f"tpid_{e:04x}")
        if nt == 2 and ets[2] in l2ref.TPIDS:
            t.add("third_tag")
        et, avail = ets[nt], L - off
        if et == 0x0800:
            t |= {f"v4_avail{avail}"} & {"v4_avail19", "v4_avail20"}
            if avail >= 20 and int(f[off]) >> 4 == 4:
                hl, total = (int(f[off]) & 15) * 4, int(f[off + 2]) << 8 | int(f[off + 3])
                if hl > 20:
                    t |= {f"v4_avail_hl{avail - hl:+d}"} & {"v4_avail_hl-1", "v4_avail_hl+0"}
                if 20 <= hl <= avail and total >= hl:
                    t |= {f"v4_avail_total{avail - total:+d}"} & {"v4_avail_total-1", "v4_avail_total+0",
                                                                  "v4_avail_total+1"}
        elif et == 0x86DD:
            t |= {f"v6_avail{avail}"} & {"v6_avail39", "v6_avail40"}
            if avail >= 40 and int(f[off]) >> 4 == 6:
                total = 40 + (int(f[off + 4]) << 8 | int(f[off + 5]))
                t |= {f"v6_avail_total{avail - total:+d}"} & {"v6_avail_total-1", "v6_avail_total+0",
                                                              "v6_avail_total+1"}
        elif et < 0x0600:
            t.add("len_8023")
    return t


REQUIRED = ({f"cls_{x}" for x in l2ref.NAMES} |
            {f"{x}_tags{t}" for x in l2ref.NAMES if x != "RUNT" for t in (0, 1, 2)} |
            {"tpid_8100", "tpid_88a8", "third_tag", "bcast", "mcast", "ucast", "vlan", "len_8023",
             "L0", "L13", "L14", "runt_tag1_L0", "runt_tag1_L3", "runt_tag2_L0", "runt_tag2_L3",
             "v4_avail19", "v4_avail20", "v4_avail_hl-1", "v4_avail_hl+0",
             "v4_avail_total-1", "v4_avail_total+0", "v4_avail_total+1",
             "v6_avail39", "v6_avail40", "v6_avail_total-1", "v6_avail_total+0", "v6_avail_total+1",
             "l3_fits_tags0", "l3_fits_tags1", "l3_fits_tags2", "runt_l3_tags0", "runt_l3_tags1"})


def poison(n, phase=0):
    return np.resize(np.roll(POISON, -phase), n)


def lay(items, align):
    """(buf, raw): every frame starts at a byte with (offset & 15) == align, with
    poison before and after it; an item without an l3_off of its own gets a small
    one; the last frame ends on the buffer's last byte."""
    pos, at = 0, []
    order = sorted(range(len(items)), key=lambda i: items[i][1] or 0)      # the large l3_offs last
    for i in order:
        f, l3 = items[i]
        l3 = (5 * i) % 23 if l3 is None else l3
        pos = max(pos + 1, l3)
        pos += (align - pos) % 16
        at.append((i, pos, l3))
        pos += len(f)
    last = max(p + len(items[i][0]) for i, p, _ in at)
    buf = poison(last, 3)
    raw = np.zeros(len(items), DESC_DTYPE)
    for i, p, l3 in at:
        f = items[i][0]
        buf[p:p + len(f)] = f
        raw[i] = (p - l3, l3, len(f))
    return buf, raw


def tiled(items, n, slot=64):
    """n frames in `slot`-byte slots, tiled from the items that fit one (l3_off 0):
    (buf, raw, m), m the period in frames."""
    fit = [f for f, l3 in items if l3 is None and len(f) <= slot]
    m = len(fit)
    block = poison(m * slot, 7)
    lens = np.zeros(m, np.int64)
    for j, f in enumerate(fit):
        block[j * slot:j * slot + len(f)] = f
        lens[j] = len(f)
    reps = -(-n // m)
    buf = np.tile(block, reps)[:n * slot]
    raw = np.zeros(n, DESC_DTYPE)
    raw["frame_off"] = np.arange(n, dtype=np.uint64) * slot
    raw["ip_len"] = np.tile(lens, reps)[:n]
    return buf, raw, m


def expect_tiled(buf, raw, m, slot=64):
    """l2ref.expect over one period, repeated: the frames of a tiled burst differ
    only in frame_off.  (desc_out, cls, count)."""
    n = len(raw)
    d1, c1, _ = l2ref.expect(buf, raw[:min(m, n)])
    reps = -(-n // m)
    out = np.tile(d1, reps)[:n].copy()
    out["frame_off"] = raw["frame_off"]
    cls = np.tile(c1, reps)[:n]
    return out, cls, counts(cls)


def counts(cls):
    """The counters a call adds, from its class bytes."""
    cls = np.asarray(cls)
    c = np.zeros(l2ref.NCOUNT, np.uint32)
    c[:l2ref.NCLASS] = np.bincount(cls & 15, minlength=l2ref.NCLASS)[:l2ref.NCLASS]
    c[10] = np.count_nonzero(cls & (l2ref.BCAST | l2ref.MCAST))
    c[11] = np.count_nonzero(cls & l2ref.VLAN)
    return c


def splitmix64(seed, j):
    M = (1 << 64) - 1
    z = (seed + (j + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def synth_eth_one(buf, k, fo, l3, ln, vlan_every, seed):
    """cgck_synth_eth's framing of frame k (include/cgck.h), whose IP header lies at
    buf[fo + l3]: writes the header into buf, returns the raw descriptor."""
    t = 1 if vlan_every and k % vlan_every == 0 else 0
    h = 14 + 4 * t
    e = fo + l3 - h
    m0, m1 = splitmix64(seed, 2 * k), splitmix64(seed, 2 * k + 1)
    buf[e:e + 8] = [(m0 >> (8 * i)) & 255 for i in range(8)]
    buf[e + 8:e + 12] = [(m1 >> (8 * i)) & 255 for i in range(4)]
    buf[e] &= 0xFE
    if t:
        buf[e + 12:e + 16] = (0x81, 0x00, (k >> 8) & 0x0F, k & 255)
    v = int(buf[fo + l3]) >> 4
    buf[e + h - 2:e + h] = be16(0x0800 if v == 4 else 0x86DD if v == 6 else 0x0806)
    return fo, l3 - h, max(ln + h, 60)


def synth_eth(buf, desc, vlan_every, seed):
    """cgck_synth_eth restated over a ring set's bytes and descriptors: writes the
    headers into buf, returns raw."""
    raw = np.zeros(len(desc), DESC_DTYPE)
    for k in range(len(desc)):
        raw[k] = synth_eth_one(buf, k, int(desc["frame_off"][k]), int(desc["l3_off"][k]), int(desc["ip_len"][k]),
                               vlan_every, seed)
    return raw
