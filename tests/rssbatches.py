"""Frame builders for the per-frame RSS hash tests (test_rss_frames_cpu.py,
test_gpu_rss_frames.py, tools/make_rss_frames_golden.py, tools/rssf_ab.py), on
top of mixedbatches / ip6batches: every class of mixedbatches.all_classes plus
the classes only the hash tells apart (IPv4 fragments and DF, frames cut just
before and after their ports, IPv6 Fragment headers, chains cut mid-header), the
published verification tuples wrapped as minimal TCP frames, and a fuzz mix.
Nothing here calls the library under test."""
import ipaddress

import numpy as np

import ip6batches as B6
import ip6ref
import mixedbatches as MB
import rssref

DESC_DTYPE = B6.DESC_DTYPE
packed, slotted, lay = B6.packed, B6.slotted, B6.lay
H, D, R, A, F = B6.H, B6.D, B6.R, B6.A, B6.F
MF, DF = 0x2000, 0x4000
HF_ALL = rssref.RSS_TCP | rssref.RSS_UDP

# Microsoft's published IPv6 verification tuples ("Verifying the RSS Hash
# Calculation": source, destination, source port, destination port, the hash
# with TCP ports, the hash of the addresses alone) under the key the reference
# carries as freebsd_rss_key.
MS_IP6 = (
    ("3ffe:2501:200:1fff::7", "3ffe:2501:200:3::1", 2794, 1766, 0x40207D3D, 0x2CC18CD5),
    ("3ffe:501:8::260:97ff:fe40:efab", "ff02::1", 14230, 4739, 0xDDE51BBF, 0x0F0C461C),
    ("3ffe:1900:4545:3:200:f8ff:fe21:67cf", "fe80::200:f8ff:fe21:67cf", 44251, 38024, 0x02D1FEEF, 0x4B61E985),
)


def v4(rng, ln, proto, hl=5, frag=0):
    """mixedbatches.v4 with the flags / fragment-offset field set to `frag`."""
    p = MB.v4(rng, max(ln, 8), proto, hl)
    p[6], p[7] = frag >> 8, frag & 255
    return p[:ln]


def ms_frame4(tuple12):
    """A 40-byte IPv4 TCP frame carrying the 12 tuple bytes {src, dst, sport, dport}."""
    p = np.zeros(40, np.uint8)
    p[0], p[3], p[8], p[9] = 0x45, 40, 64, 6
    p[12:20] = tuple12[:8]
    p[20:24] = tuple12[8:12]
    return p


def ms_frame6(src, dst, sport, dport):
    """A 60-byte IPv6 TCP frame from src:sport to dst:dport."""
    p = np.zeros(60, np.uint8)
    p[0], p[5], p[6], p[7] = 0x60, 20, 6, 64
    p[8:24] = np.frombuffer(ipaddress.IPv6Address(src).packed, np.uint8)
    p[24:40] = np.frombuffer(ipaddress.IPv6Address(dst).packed, np.uint8)
    p[40:44] = (sport >> 8, sport & 255, dport >> 8, dport & 255)
    return p


def rss_classes(rng):
    """The classes the checksum tests have no reason to build."""
    out = [v4(rng, 60, 6, 5, MF), v4(rng, 64, 17, 6, MF | 185), v4(rng, 60, 6, 5, 1), v4(rng, 576, 17, 5, 0x1FFF),
           v4(rng, 60, 6, 5, DF), v4(rng, 61, 17, 7, DF), v4(rng, 60, 6, 5, DF | MF)]
    out += [v4(rng, hl + cut, pr, hl // 4, fr) for hl in (20, 24, 60) for cut in (3, 4) for pr in (6, 17)
            for fr in (0, DF)]
    out += [v4(rng, ln, pr, 4) for ln, pr in ((20, 6), (40, 17), (64, 6))]                 # ip_hl 4
    out += [v4(rng, ln, pr, hl) for pr in (1, 47) for ln, hl in ((28, 5), (64, 5), (84, 9))]
    out += [v4(rng, ln, pr, hl) for pr in (6, 17) for ln, hl in ((40, 5), (64, 5), (65, 6), (131, 11), (1500, 15))]
    out += [ip6ref.packet(rng, ln, nh, ((F, 8),)) for ln, nh in ((48, 6), (60, 17), (131, 6))]
    out += [ip6ref.packet(rng, ln, nh, ch + ((F, 8),)) for ln, nh, ch in
            ((100, 6, ((H, 8),)), (131, 17, ((H, 16), (D, 8))), (88, 6, ((A, 12),)))]
    for ch in ((), ((H, 8),), ((H, 8), (D, 16)), ((A, 12), (R, 24))):
        l4 = 40 + sum(b for _, b in ch)
        out += [ip6ref.packet(rng, l4 + cut, nh, ch) for cut in (3, 4, 10) for nh in (6, 17)]
    out += [ip6ref.packet(rng, ln, nh, ch) for nh in (58, 59) for ln, ch in ((40, ()), (64, ()), (131, ((H, 8),)))]
    out += [ip6ref.packet(rng, ln, 6, ((H, 8), (D, 16))) for ln in (49, 50, 60, 63, 64)]   # cut inside the chain
    out += [ip6ref.packet(rng, 41, 6, ((H, 8),)), ip6ref.packet(rng, 42, 17, ((A, 12),))]
    out += [ip6ref.packet(rng, 200, nh, ((H, 8),) + ((D, 8),) * k) for nh in (6, 17) for k in (7, 8)]
    return out


def all_classes(rng):
    fr = MB.all_classes(rng) + rss_classes(rng)
    return [fr[i] for i in rng.permutation(len(fr))]


def bad6(p):
    """Why an IPv6 frame is BAD_LEN: "short", "past" (l4_off past ip_len), "ninth"
    or "cut" (a header's first two bytes past ip_len); None when it is not."""
    ln = len(p)
    if ln < 40:
        return "short"
    off, nh, seen = 40, int(p[6]), 0
    while True:
        if off > ln:
            return "past"
        if nh == 44 or nh not in (0, 43, 60, 51):
            return None
        if seen == 8:
            return "ninth"
        if off + 2 > ln:
            return "cut"
        step = (int(p[off + 1]) + 2) * 4 if nh == 51 else (int(p[off + 1]) + 1) * 8
        nh, off, seen = int(p[off]), off + step, seen + 1


def tags(p):
    """mixedbatches.tags plus the hash's own classes, read from the bytes."""
    ln = len(p)
    t = set(MB.tags(p))
    kind, tup = rssref.tuple_of(p, ln, HF_ALL)
    if tup is not None:
        t.add(("v6" if kind & rssref.RSS_IP6 else "v4") + ("_4tuple" if kind & rssref.RSS_L4 else "_2tuple"))
    if ln == 0:
        return t
    v = int(p[0]) >> 4
    if v == 4 and ln >= 20:
        hl = 4 * (int(p[0]) & 15)
        if hl == 16:
            t.add("v4_ihl4")
        if hl >= 20 and ln >= hl:
            fo = int(p[6]) << 8 | int(p[7])
            if fo & MF:
                t.add("v4_mf")
            if fo & 0x1FFF:
                t.add("v4_off")
            if fo & 0x3FFF == 0:
                t.add("v4_df_only" if fo & DF else "v4_nofrag")
                t.add(f"v4_nofrag_p{int(p[9])}")
                if int(p[9]) in (6, 17) and ln - hl in (3, 4):
                    t.add(f"v4_p{int(p[9])}_hl{hl}_plus{ln - hl}")
    if v == 6:
        why = bad6(p)
        if why:
            t.add(f"v6_bad_{why}")
        else:
            off, nh, st = rssref.walk6(p, ln)
            if st == rssref.FRAG:
                t.add("v6_frag_direct" if off == 40 else "v6_frag_chain")
            else:
                t.add(f"v6_term{nh}")
                if nh in (6, 17) and ln - off in (3, 4, 10):
                    t.add(f"v6_nh{nh}_plus{ln - off}" + ("_chain" if off > 40 else ""))
    return t


RSS_REQUIRED = ({"v4_mf", "v4_off", "v4_df_only", "v4_nofrag", "v4_ihl4", "v4_nofrag_p1", "v4_nofrag_p47",
                 "v4_nofrag_p6", "v4_nofrag_p17", "v6_frag_direct", "v6_frag_chain", "v6_term58", "v6_term59",
                 "v6_bad_short", "v6_bad_past", "v6_bad_ninth", "v6_bad_cut",
                 "v4_2tuple", "v4_4tuple", "v6_2tuple", "v6_4tuple"} |
                {f"v4_p{pr}_hl{hl}_plus{c}" for pr in (6, 17) for hl in (20, 24, 60) for c in (3, 4)} |
                {f"v6_nh{nh}_plus{c}{s}" for nh in (6, 17) for c in (3, 4, 10) for s in ("", "_chain")})
REQUIRED = MB.REQUIRED | RSS_REQUIRED


def pattern(rng, kind, n=64):
    """mixedbatches.pattern's family patterns ("alt", "runs", "one6", "one4") with
    every frame an unfragmented TCP or UDP frame that holds its ports: "one6" puts
    an IPv6 extension chain at lane 37 of each step of IPv4 frames without options,
    "one4" an IPv4 frame with options at lane 37 of each step of IPv6 frames
    without a chain (one lane of the wave needs the second load round), "alt" and
    "runs" mix options and chains among plain frames."""
    lens = rng.choice(np.array((64, 65, 131, 576, 577, 1500)), n)
    out = []
    for i, ln in enumerate(lens):
        ln, pr = int(ln), (6, 17)[i % 2]
        six = {"alt": i % 2 == 1, "runs": (i // 64) % 2 == 1, "one6": i % 64 == 37, "one4": i % 64 != 37}[kind]
        if six:
            chain = ((H, 8), (D, 16)) if kind == "one6" else () if kind == "one4" else B6.chain_of(i)
            out.append(ip6ref.packet(rng, max(ln, 131), pr, chain))
        else:
            hl = 11 if kind == "one4" else 5 if kind == "one6" else (5, 5, 6)[i % 3]
            out.append(v4(rng, ln, pr, hl, DF if i % 3 == 0 else 0))
    return out


def fuzz(rng, n):
    """n random frames: about a quarter each IPv4 and IPv6 frames that hash their
    ports, a sixth each that hash addresses only, and random frames of any kind
    (most of them cut short, BAD_LEN or of neither family) for the rest."""
    lens = np.array((40, 44, 52, 60, 64, 65, 99, 131, 576, 1500))
    out = []
    for _ in range(n):
        c = int(rng.integers(0, 100))
        ln = int(rng.choice(lens)) + int(rng.integers(0, 4))
        pr = int(rng.choice((6, 17)))
        if c < 25:
            hl = int(rng.choice((5, 5, 5, 6, 10, 15)))
            out.append(v4(rng, max(ln, 4 * hl + 4), pr, hl, int(rng.choice((0, DF)))))
        elif c < 40:
            k = int(rng.integers(0, 3))
            out.append(v4(rng, ln, (pr, int(rng.choice((1, 47, 132))), pr)[k], int(rng.choice((5, 7))),
                          (MF, 0, int(rng.integers(1, 0x2000)))[k]))
        elif c < 62:
            ch = tuple((int(rng.choice((H, R, D, A))), 8 * int(rng.integers(1, 4))) for _ in range(int(rng.integers(0, 3)))) \
                if rng.integers(0, 3) == 0 else ()
            out.append(ip6ref.packet(rng, max(ln, 44 + sum(b for _, b in ch)), pr, ch))
        elif c < 78:
            k = int(rng.integers(0, 3))
            ch = (((F, 8),), ((H, 8), (F, 8)), ())[k]
            out.append(ip6ref.packet(rng, max(ln, 56), (pr, pr, int(rng.choice((58, 59, 132))))[k], ch))
        elif c < 90:
            ln = int(rng.integers(0, 140))
            ch = tuple((int(rng.choice((H, R, D, A))), 8 * int(rng.integers(1, 3))) for _ in range(int(rng.integers(0, 10))))
            out.append(ip6ref.packet(rng, ln, pr, ch) if rng.integers(0, 2) else
                       MB.v4(rng, ln, pr, int(rng.integers(4, 16))))
        else:
            out.append(MB.other(rng, int(rng.integers(1, 200)), int(rng.choice((0, 1, 5, 7, 15)))))
    return out


def refill(rng, buf, offs, lens):
    """A copy of buf with every byte outside the frames replaced."""
    keep = np.zeros(buf.nbytes, bool)
    for o, ln in zip(offs, lens):
        keep[int(o):int(o) + int(ln)] = True
    out = rng.integers(0, 256, buf.nbytes, dtype=np.uint8)
    out[keep] = buf[keep]
    return out
