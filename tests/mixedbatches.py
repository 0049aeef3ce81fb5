"""Batch builders for the CGCK_MIXED tests (test_mixed_cpu.py, test_gpu_mixed.py,
tools/make_mixed_golden.py), on top of ip6batches (layouts, IPv6 frames) and
ip6ref.packet: IPv4 frames of every header class, frames of neither family, the
family patterns inside a 64-packet step, valid checksum fields for the verify
tests, and the Python restatement of cgck_synth_imix_dual.  Nothing here calls
the library under test."""
import numpy as np

import ip6batches as B6
import ip6ref
import mixedref

V4_LENS = (20, 21, 28, 40, 60, 64, 576, 1500)
V4_PROTOS = (1, 6, 17, 47)
V4_FIELD = {1: 2, 6: 16, 17: 6}
OTHER_V = (0, 5, 15)
DESC_DTYPE = B6.DESC_DTYPE
packed, slotted, lay = B6.packed, B6.slotted, B6.lay


def v4(rng, ln, proto, hl=5, ip_sum0=False, l4_sum0=False):
    """A random IPv4 packet cut at ln bytes: ver/ihl 0x40 | hl, total length ln, ip_p proto."""
    p = rng.integers(0, 256, max(ln, 60), dtype=np.uint8)
    p[0] = 0x40 | hl
    p[2], p[3] = (ln >> 8) & 255, ln & 255
    p[9] = proto
    if ip_sum0:
        p[10:12] = 0
    if l4_sum0 and proto in V4_FIELD and 4 * hl + V4_FIELD[proto] + 2 <= len(p):
        p[4 * hl + V4_FIELD[proto]:4 * hl + V4_FIELD[proto] + 2] = 0
    return p[:ln]


def other(rng, ln, v):
    """A frame of neither family (an ARP frame, say): version nibble v."""
    p = rng.integers(0, 256, max(ln, 1), dtype=np.uint8)
    p[0] = (v << 4) | (int(p[0]) & 15)
    return p[:ln]


def v4_classes(rng):
    """Every IPv4 class of the issue once or more: lengths x protocols, ip_hl
    5..15, stored ip_sum 0, stored UDP sum 0, ip_len 0, 1, 19 and a length below
    ip_hl * 4."""
    out = [v4(rng, ln, pr) for ln in V4_LENS for pr in V4_PROTOS]
    out += [v4(rng, 4 * hl + 40 + hl % 3, V4_PROTOS[hl % 4], hl) for hl in range(5, 16)]
    out += [v4(rng, 4 * hl, 6, hl) for hl in (6, 15)]                      # a header and nothing after it
    out += [v4(rng, ln, pr, 5, ip_sum0=True) for ln, pr in ((40, 6), (576, 17), (61, 1))]
    out += [v4(rng, ln, 17, hl, l4_sum0=True) for ln, hl in ((28, 5), (64, 5), (577, 7))]
    out += [v4(rng, 0, 6), v4(rng, 1, 6), v4(rng, 19, 17), v4(rng, 24, 6, 7), v4(rng, 59, 1, 15)]
    return out


def v6_classes(rng):
    """ip6batches' lengths x next headers, the extension chains, SPECIALS (ip_len
    0 left out: it has no version nibble), and UDP with a stored field of 0."""
    out = [ip6ref.packet(rng, ln, B6.NHS[(i + j) % len(B6.NHS)], B6.chain_of(i + 5 * j) if ln >= 64 else ())
           for i, ln in enumerate(B6.LENS) for j in range(2)]
    out += [ip6ref.packet(rng, ln, nh, chain) for chain, nh, ln in B6.SPECIALS if ln > 0]
    for ln in (48, 64, 577):
        p = ip6ref.packet(rng, ln, 17)
        p[46:48] = 0
        out.append(p)
    return out


def other_classes(rng):
    return [other(rng, ln, v) for v in OTHER_V for ln in (1, 28, 64, 577)]


def all_classes(rng):
    fr = v4_classes(rng) + v6_classes(rng) + other_classes(rng)
    return [fr[i] for i in rng.permutation(len(fr))]


def tags(p):
    """The classes a packet belongs to, read from its bytes."""
    ln = len(p)
    if ln == 0:
        return {"len0"}
    v = int(p[0]) >> 4
    if v == 4:
        hl = int(p[0]) & 15
        t = {f"v4_len{ln}", f"v4_hl{hl}"}
        if ln >= 20 and ln < 4 * hl:
            t.add("v4_below_hl")
        if ln >= 20 and ln >= 4 * hl:
            pr = int(p[9])
            t.add(f"v4_p{pr}")
            if not p[10] and not p[11]:
                t.add("v4_ipsum0")
            if pr == 17 and 4 * hl + 8 <= ln and not p[4 * hl + 6] and not p[4 * hl + 7]:
                t.add("v4_udpsum0")
        return t
    if v == 6:
        l4, nh, st = ip6ref.walk(p, ln)
        t = {f"v6_len{ln}", f"v6_{st}"}
        if st == ip6ref.OK:
            t.add(f"v6_nh{nh}")
            if l4 > 40:
                t.add("v6_chain")
            if nh == 17 and not p[l4 + 6] and not p[l4 + 7]:
                t.add("v6_udpsum0")
        return t
    return {f"other_v{v}"}


REQUIRED = ({f"v4_len{ln}" for ln in V4_LENS + (1, 19)} | {f"v4_hl{h}" for h in range(5, 16)} |
            {f"v4_p{p}" for p in V4_PROTOS} | {"v4_ipsum0", "v4_udpsum0", "v4_below_hl", "len0"} |
            {f"v6_len{ln}" for ln in B6.LENS} | {f"v6_nh{nh}" for nh in B6.NHS} |
            {"v6_chain", "v6_no_l4", "v6_bad_len", "v6_udpsum0"} | {f"other_v{v}" for v in OTHER_V})


def pattern(rng, kind, n=64):
    """n frames of typical lengths whose families follow `kind` inside a step:
    "alt" alternating lanes; "runs" 64 IPv4 then 64 IPv6 and so on; "one6" an IPv6
    packet with an extension chain at lane 37 of each step of IPv4 packets; "one4"
    an IPv4 packet with options at lane 37 of each step of IPv6 packets."""
    lens = rng.choice(np.array((64, 65, 131, 576, 577, 1500)), n)
    out = []
    for i, ln in enumerate(lens):
        ln = int(ln)
        six = {"alt": i % 2 == 1, "runs": (i // 64) % 2 == 1, "one6": i % 64 == 37, "one4": i % 64 != 37}[kind]
        if six:
            chain = ((0, 8), (60, 16)) if kind == "one6" else B6.chain_of(i)
            out.append(ip6ref.packet(rng, max(ln, 131), (6, 17, 58)[i % 3], chain))
        else:
            out.append(v4(rng, ln, V4_PROTOS[i % 4], 11 if kind == "one4" else (5, 5, 6)[i % 3]))
    return out


def fill_fields(port, buf, offs, lens):
    """The batch with every checksum field it holds made valid (what a sender
    stores): the IPv4 header sum, and the L4 field of either family."""
    out, _ = mixedref.expect(port, buf, offs, lens, mixedref.IP | mixedref.L4 | mixedref.ZERO_FIELDS)
    fam = mixedref.family(buf, offs, lens)
    got = buf.copy()
    for i, (o, ln) in enumerate(zip(offs, lens)):
        o, ln, p = int(o), int(ln), buf[int(o):int(o) + int(ln)]
        at = []
        if fam[i] == 4 and ln >= 20 and ln >= 4 * (int(p[0]) & 15):
            hl = 4 * (int(p[0]) & 15)
            at.append((10, int(out[i]) & 0xFFFF))
            fo = V4_FIELD.get(int(p[9]))
            if fo is not None and hl + fo + 2 <= ln:
                at.append((hl + fo, int(out[i]) >> 16))
        elif fam[i] == 6:
            l4, nh, st = ip6ref.walk(p, ln)
            if st == ip6ref.OK and nh in ip6ref.FIELD:
                at.append((l4 + ip6ref.FIELD[nh], int(out[i]) >> 16))
        for a, v in at:
            got[o + a], got[o + a + 1] = v & 255, v >> 8
    return got


def l4_field_at(p):
    """Offset of the packet's L4 checksum field, or None."""
    ln = len(p)
    if ln and int(p[0]) >> 4 == 4:
        hl = 4 * (int(p[0]) & 15)
        fo = V4_FIELD.get(int(p[9])) if ln >= 20 and ln >= hl else None
        return hl + fo if fo is not None and hl + fo + 2 <= ln else None
    if ln and int(p[0]) >> 4 == 6:
        l4, nh, st = ip6ref.walk(p, ln)
        return l4 + ip6ref.FIELD[nh] if st == ip6ref.OK and nh in ip6ref.FIELD else None
    return None


def stamp_dual(p, ln, k):
    """cgck_synth_imix_dual's stamp on frame k (include/cgck.h)."""
    six, pk = k % 5 < 2, k % 7
    proto = 6 if pk < 4 else 17 if pk < 6 else 58 if six else 1
    if six:
        B6.stamp6(p, ln, proto)
        return
    p[0], p[1], p[2], p[3], p[9] = 0x45, 0, ln >> 8, ln & 255, proto
    p[10:12] = 0
    if 20 + V4_FIELD[proto] + 2 <= ln:
        p[20 + V4_FIELD[proto]:20 + V4_FIELD[proto] + 2] = 0


def imix_dual(port, n, seed, stride=0, l3_off=0):
    """cgck_synth_imix_dual restated: the oracle's stream bytes, its IMIX offsets
    and lengths, the per-frame stamp.  (buf, desc, offs, lens)."""
    d = [port.imix_desc(k) for k in range(n)]
    lens = np.array([x[1] for x in d], np.int64)
    fo = np.arange(n, dtype=np.int64) * stride if stride else np.array([x[0] for x in d], np.int64)
    offs = fo + l3_off
    buf = port.stream_bytes(0, n * stride if stride else int(offs[-1] + lens[-1]), seed)
    for k, (o, ln) in enumerate(zip(offs, lens)):
        stamp_dual(buf[o:o + ln], int(ln), k)
    desc = np.zeros(n, DESC_DTYPE)
    desc["frame_off"] = fo
    desc["l3_off"] = l3_off
    desc["ip_len"] = lens
    return buf, desc, offs, lens
