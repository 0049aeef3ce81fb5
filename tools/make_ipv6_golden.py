#!/usr/bin/env python3
"""Generate tests/golden/ipv6.json: the IPv6 (CGCK_IP6) cases, with every
expected checksum produced by the REFERENCE's own compiled in_cksum
(oracle/_ref/libref_cksum.so, built by oracle/build_ref.sh) run over
pseudo-header || segment.  Runs in the build container only:

    make -C oracle && python tools/make_ipv6_golden.py

The reference has no IPv6 code, but its in_cksum is the Internet checksum of
a byte string, and an IPv6 upper-layer checksum is exactly that of the
40-byte pseudo-header (RFC 8200 section 8.1) followed by the segment.  The
known-answer cases are checked a second way here, with plain RFC 1071
big-endian arithmetic written out below, before they are recorded.

Each case: name, hex (the frame, l3_off bytes of link header included),
l3_off, ip_len, the expected walk (l4_off, nh, status ok | no_l4 | bad_len),
hi_zero (out.hi with the checksum field read as zero: what a fill stores),
hi_gen (out.hi over the bytes as stored) and the verify verdicts of
CGCK_VERIFY_TOY | CGCK_IP6 without and with CGCK_V_UDP_ZERO_SKIP.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle  # noqa: E402

BAD_L4, BAD_LEN = 2, 4
FIELD = {6: 16, 17: 6, 58: 2}
EXT8 = (0, 43, 60)      # length (b[1] + 1) * 8
AH = 51                 # length (b[1] + 2) * 4
FRAG = 44


def walk(p, ip_len):
    """include/cgck.h, CGCK_IP6: where the upper-layer header starts."""
    if ip_len < 40:
        return 40, 0, "bad_len"
    off, nh = 40, int(p[6])
    for walked in range(9):
        if off > ip_len:
            return off, nh, "bad_len"
        if nh == FRAG:
            return off, nh, "no_l4"
        if nh not in EXT8 and nh != AH:
            fo = FIELD.get(nh)
            if fo is not None and off + fo + 2 > ip_len:
                return off, nh, "bad_len"
            return off, nh, "ok"
        if walked == 8 or off + 2 > ip_len:
            return off, nh, "bad_len"
        ln = (int(p[off + 1]) + 2) * 4 if nh == AH else (int(p[off + 1]) + 1) * 8
        nh, off = int(p[off]), off + ln
    raise AssertionError("unreachable")


def pseudo_segment(p, ip_len, l4_off, nh, zero_field):
    n = ip_len - l4_off
    ph = bytes(p[8:40]) + n.to_bytes(4, "big") + bytes((0, 0, 0, nh))
    seg = bytearray(bytes(p[l4_off:ip_len]))
    if zero_field and nh in FIELD:
        seg[FIELD[nh]:FIELD[nh] + 2] = b"\0\0"
    return np.frombuffer(ph + bytes(seg), np.uint8).copy()


def rfc1071_be(data):
    """RFC 1071 by the book: big-endian 16-bit words, end-around carry,
    complement; the two bytes to transmit are this value high byte first."""
    b = bytes(data) + (b"\0" if len(data) & 1 else b"")
    s = sum(b[i] << 8 | b[i + 1] for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def make_case(R, name, frame, l3_off, ip_len):
    p = frame[l3_off:]
    l4_off, nh, status = walk(p, ip_len)
    c = {"name": name, "hex": bytes(frame).hex(), "l3_off": l3_off, "ip_len": ip_len,
         "l4_off": l4_off, "nh": nh, "status": status, "hi_zero": 0, "hi_gen": 0,
         "verdict_toy": 0, "verdict_toy_udp_skip": 0}
    if status == "bad_len":
        c["verdict_toy"] = c["verdict_toy_udp_skip"] = BAD_LEN
    if status != "ok":
        return c
    z = pseudo_segment(p, ip_len, l4_off, nh, True)
    g = pseudo_segment(p, ip_len, l4_off, nh, False)
    c["hi_zero"] = R.in_cksum(z, 0, len(z))
    c["hi_gen"] = R.in_cksum(g, 0, len(g))
    if nh in FIELD:
        fo = l4_off + FIELD[nh]
        stored = int(p[fo]) | int(p[fo + 1]) << 8
        bad = BAD_L4 if stored != c["hi_zero"] else 0
        c["verdict_toy"] = bad
        c["verdict_toy_udp_skip"] = 0 if nh == 17 and stored == 0 else bad
    return c


def header(ip_len, first_nh, src, dst):
    h = bytearray(40)
    h[0] = 0x60
    h[4:6] = max(ip_len - 40, 0).to_bytes(2, "big")
    h[6] = first_nh
    h[7] = 64
    h[8:24] = src
    h[24:40] = dst
    return h


def ext(kind, next_nh, nbytes, rng):
    h = bytearray(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())
    h[0] = next_nh
    h[1] = nbytes // 4 - 2 if kind == AH else nbytes // 8 - 1
    return h


def build(rng, ip_len, nh, chain=(), l3_off=0):
    """A frame: l3_off link bytes, the 40-byte header, the chain's extension
    headers, random upper-layer bytes; cut at ip_len."""
    kinds = [k for k, _ in chain] + [nh]
    body = bytearray(header(ip_len, kinds[0], rng.integers(0, 256, 16, dtype=np.uint8).tobytes(),
                            rng.integers(0, 256, 16, dtype=np.uint8).tobytes()))
    for i, (kind, nbytes) in enumerate(chain):
        body += ext(kind, kinds[i + 1], nbytes, rng)
    if len(body) < ip_len:
        body += rng.integers(0, 256, ip_len - len(body), dtype=np.uint8).tobytes()
    link = rng.integers(0, 256, l3_off, dtype=np.uint8).tobytes()
    return np.frombuffer(link + bytes(body[:ip_len]), np.uint8).copy()


def fill(R, frame, l3_off, ip_len):
    """Store the correct checksum into the frame's field (a valid packet)."""
    p = frame[l3_off:]
    l4_off, nh, status = walk(p, ip_len)
    assert status == "ok" and nh in FIELD
    z = pseudo_segment(p, ip_len, l4_off, nh, True)
    v = R.in_cksum(z, 0, len(z))
    fo = l3_off + l4_off + FIELD[nh]
    frame[fo] = v & 255
    frame[fo + 1] = v >> 8
    return v


def kat_cases(R):
    """Known answers, written out: fe80::1 -> ff02::1 ICMPv6 echo request,
    2001:db8::1 -> 2001:db8::2 UDP 53 -> 1024 "hi!\\n", and a TCP SYN."""
    out = []
    src1, dst1 = bytes.fromhex("fe800000000000000000000000000001"), bytes.fromhex("ff020000000000000000000000000001")
    src2, dst2 = bytes.fromhex("20010db8000000000000000000000001"), bytes.fromhex("20010db8000000000000000000000002")
    icmp = bytes.fromhex("8000" "0000" "1234" "0001") + b"abcdefgh"
    udp = bytes.fromhex("0035" "0400" "000c" "0000") + b"hi!\n"
    tcp = bytes.fromhex("c000" "0050" "00000001" "00000000" "5002" "ffff" "0000" "0000")
    for name, nh, src, dst, seg in (("kat_icmpv6_echo", 58, src1, dst1, icmp), ("kat_udp", 17, src2, dst2, udp),
                                    ("kat_tcp_syn", 6, src2, dst2, tcp)):
        ip_len = 40 + len(seg)
        frame = np.frombuffer(bytes(header(ip_len, nh, src, dst)) + seg, np.uint8).copy()
        c = make_case(R, name, frame, 0, ip_len)
        # the second way: RFC 1071 big-endian arithmetic over the same bytes;
        # the reference returns the value whose little-endian store puts those
        # two bytes on the wire high byte first
        be = rfc1071_be(src + dst + len(seg).to_bytes(4, "big") + bytes((0, 0, 0, nh)) + seg) or 0xFFFF
        assert c["hi_zero"] == ((be & 255) << 8 | be >> 8), (name, hex(be), hex(c["hi_zero"]))
        c["rfc1071_be"] = be
        out.append(c)
    # by hand, kat_icmpv6_echo: src + dst words fe80 + 1 + ff02 + 1 = 1fd84;
    # length 0010, next header 003a; message 8000 + 1234 + 0001 + 6162 + 6364 +
    # 6566 + 6768 = 226c9... summed and folded below in full
    words = [0xfe80, 1, 0xff02, 1, 0x0010, 0x003a, 0x8000, 0x1234, 0x0001, 0x6162, 0x6364, 0x6566, 0x6768]
    s = sum(words)
    s = (s & 0xFFFF) + (s >> 16)
    assert out[0]["rfc1071_be"] == (~s) & 0xFFFF
    return out


def main():
    R = oracle.reference()
    if R is None:
        sys.exit("make_ipv6_golden: oracle/_ref/libref_cksum.so missing (run make -C oracle)")
    rng = np.random.default_rng(0x1B6)
    cases = kat_cases(R)

    # lengths at the kernels' boundaries x upper-layer protocols x header offsets
    small, big = (40, 41, 48, 60, 61, 64), (575, 576, 1279, 1280, 1499, 1500, 1514)
    protos = (6, 17, 58, 59, 253)
    for i, ln in enumerate(small):
        for j, nh in enumerate(protos):
            l3 = (0, 14, 15, 18)[(i + j) % 4]
            cases.append(make_case(R, f"len{ln}_nh{nh}_l3{l3}", build(rng, ln, nh, (), l3), l3, ln))
    for i, ln in enumerate(big):
        for nh in (protos[i % 5], protos[(i + 2) % 5]):
            l3 = (0, 14, 15, 18)[i % 4]
            cases.append(make_case(R, f"len{ln}_nh{nh}_l3{l3}", build(rng, ln, nh, (), l3), l3, ln))

    # extension chains
    chains = {
        "hbh8": ((0, 8),), "hbh16_dst8": ((0, 16), (60, 8)), "rt24": ((43, 24),), "ah24": ((51, 24),),
        "ah12_dst8": ((51, 12), (60, 8)), "hbh8_rt8_dst8_ah8": ((0, 8), (43, 8), (60, 8), (51, 8)),
        "eight": ((0, 8),) + ((60, 8),) * 7, "hbh2048": ((0, 2048),),
    }
    for name, ch in chains.items():
        hdrs = sum(nb for _, nb in ch)
        for nh in (6, 17, 58, 59):
            for l3 in (0, 15):
                if hdrs > 1024 and (nh > 17 or l3):   # the long header: two cases are enough
                    continue
                ln = 40 + hdrs + 33
                cases.append(make_case(R, f"chain_{name}_nh{nh}_l3{l3}", build(rng, ln, nh, ch, l3), l3, ln))
    for nh in (6, 17):
        cases.append(make_case(R, f"frag_nh{nh}", build(rng, 100, nh, ((FRAG, 8),)), 0, 100))
        cases.append(make_case(R, f"hbh8_frag_nh{nh}", build(rng, 100, nh, ((0, 8), (FRAG, 8))), 0, 100))
        # a chain running past ip_len: the second header's bytes are not there
        cases.append(make_case(R, f"chain_past_len_nh{nh}", build(rng, 49, nh, ((0, 8), (60, 16))), 0, 49))
        cases.append(make_case(R, f"chain_l4_past_len_nh{nh}", build(rng, 52, nh, ((0, 8), (60, 16))), 0, 52))
        cases.append(make_case(R, f"chain_field_past_len_nh{nh}", build(rng, 40 + 8 + 5, nh, ((0, 8),)), 0, 53))
        cases.append(make_case(R, f"nine_headers_nh{nh}", build(rng, 200, nh, ((0, 8),) + ((60, 8),) * 8), 0, 200))
    cases.append(make_case(R, "short_39", build(rng, 40, 6)[:39], 0, 39))
    cases.append(make_case(R, "short_0", np.zeros(0, np.uint8), 0, 0))

    # the zero class: a payload word adjusted so the folded sum is 0xFFFF (S
    # a nonzero multiple of 65535), for which the output is 0xFFFF, not 0
    for nh in (6, 17, 58):
        for ln in (72, 577):
            f = build(rng, ln, nh)
            l4 = 40
            fo = l4 + FIELD[nh]
            f[fo:fo + 2] = 0
            z = pseudo_segment(f, ln, l4, nh, True)
            s = sum(int(z[i]) | (int(z[i + 1]) << 8 if i + 1 < len(z) else 0) for i in range(0, len(z), 2)) % 65535
            at = l4 + 20     # an even offset from the region's start, past every field
            w = int(f[at]) | int(f[at + 1]) << 8
            w = (w - s) % 65535 or 65535
            f[at], f[at + 1] = w & 255, w >> 8
            c = make_case(R, f"zero_class_nh{nh}_len{ln}", f, 0, ln)
            assert c["hi_zero"] == 0xFFFF, c
            cases.append(c)

    # verify vectors: valid packets, single-byte corruptions of them, and UDP
    # with a stored 0 (RFC 768's "no checksum", which IPv6 forbids: BAD_L4
    # unless the caller asks for CGCK_V_UDP_ZERO_SKIP)
    for nh in (6, 17, 58):
        for ln, ch, l3 in ((80, (), 0), (1280, (), 14), (121, ((0, 8), (60, 8)), 15)):
            f = build(rng, ln, nh, ch, l3)
            fill(R, f, l3, ln)
            c = make_case(R, f"valid_nh{nh}_len{ln}", f, l3, ln)
            assert c["verdict_toy"] == 0
            cases.append(c)
            l4 = c["l4_off"]
            for what, at in (("src", 8), ("dst_last", 39), ("l4_first", l4), ("field", l4 + FIELD[nh]),
                             ("last", ln - 1)):
                g = f.copy()
                g[l3 + at] ^= 0x40
                c = make_case(R, f"corrupt_{what}_nh{nh}_len{ln}", g, l3, ln)
                assert c["verdict_toy"] == BAD_L4, c["name"]
                cases.append(c)
    for ln in (48, 64, 1500):
        f = build(rng, ln, 17)
        f[46:48] = 0
        c = make_case(R, f"udp_stored_zero_len{ln}", f, 0, ln)
        assert c["verdict_toy"] == BAD_L4 and c["verdict_toy_udp_skip"] == 0
        cases.append(c)

    # random chains and lengths
    for k in range(60):
        ch = tuple((int(rng.choice((0, 43, 60, 51))), 8 * int(rng.integers(1, 4))) for _ in range(int(rng.integers(0, 4))))
        hdrs = sum(nb for _, nb in ch)
        ln = 40 + hdrs + int(rng.integers(0, 90))
        nh = int(rng.choice((6, 17, 58, 59, 132)))
        l3 = int(rng.choice((0, 14, 15, 18)))
        cases.append(make_case(R, f"random_{k}", build(rng, ln, nh, ch, l3), l3, ln))

    path = os.path.join(ROOT, "tests", "golden", "ipv6.json")
    with open(path, "w") as f:
        json.dump({"note": "made by tools/make_ipv6_golden.py with the reference's compiled in_cksum",
                   "cases": cases}, f, indent=0)
    st = {s: sum(1 for c in cases if c["status"] == s) for s in ("ok", "no_l4", "bad_len")}
    print(f"{path}: {len(cases)} cases {st}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
