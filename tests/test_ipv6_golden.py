"""The IPv6 fixture (tests/golden/ipv6.json, made by tools/make_ipv6_golden.py
with the reference's compiled in_cksum) against both oracles, the chain walk
re-derived here, and the library's IPv6 surface.  No GPU."""
import ctypes

import numpy as np
import pytest

import cgck
import ip6ref
import oracle
from conftest import load_golden


@pytest.fixture(scope="module")
def cases():
    return load_golden("ipv6.json")["cases"]


def rewalk(p, ip_len):
    """include/cgck.h, CGCK_IP6, restated: (l4_off, nh, status)."""
    if ip_len < 40:
        return 40, 0, "bad_len"
    off, nh, hops = 40, p[6], 0
    while off <= ip_len and nh in (0, 43, 60, 51) and hops < 8 and off + 2 <= ip_len:
        nh, off, hops = p[off], off + ((p[off + 1] + 2) * 4 if nh == 51 else (p[off + 1] + 1) * 8), hops + 1
    if off > ip_len:
        return off, nh, "bad_len"
    if nh == 44:
        return off, nh, "no_l4"
    if nh in (0, 43, 60, 51):   # a header that does not fit, or the ninth
        return off, nh, "bad_len"
    fo = {6: 16, 17: 6, 58: 2}.get(nh)
    return off, nh, "bad_len" if fo is not None and off + fo + 2 > ip_len else "ok"


def frame(c):
    return np.frombuffer(bytes.fromhex(c["hex"]), np.uint8).copy()


def test_fixture_shape(cases):
    assert 200 <= len(cases) <= 400
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for want in ("kat_icmpv6_echo", "kat_udp", "kat_tcp_syn", "zero_class_nh6_len72", "udp_stored_zero_len48",
                 "frag_nh6", "nine_headers_nh6", "chain_past_len_nh6", "chain_hbh16_dst8_nh17_l30"):
        assert want in names, want
    assert {c["status"] for c in cases} == {"ok", "no_l4", "bad_len"}


def test_chain_walk(cases):
    for c in cases:
        p = [int(x) for x in frame(c)[c["l3_off"]:]]
        assert rewalk(p, c["ip_len"]) == (c["l4_off"], c["nh"], c["status"]), c["name"]
        assert ip6ref.walk(p, c["ip_len"]) == (c["l4_off"], c["nh"], c["status"]), c["name"]


@pytest.mark.parametrize("which", ["port", "reference"])
def test_oracle_agreement(cases, which):
    """Every recorded checksum is in_cksum(pseudo-header || segment)."""
    O = oracle.port() if which == "port" else oracle.reference()
    if O is None:
        pytest.skip("oracle/_ref not built (no reference tree at build time)")
    for c in cases:
        p = frame(c)[c["l3_off"]:]
        for zero, key in ((True, "hi_zero"), (False, "hi_gen")):
            st, l4, nh, fo, hi = ip6ref.l4_cksum(O, p, c["ip_len"], zero)
            assert (st, hi) == (c["status"], c[key]), (c["name"], key)


def test_fixture_verdicts(cases):
    """The recorded verdicts follow from the recorded checksums and the
    stored field; the zero class outputs 0xFFFF; the known answers carry
    their RFC 1071 value."""
    for c in cases:
        p = frame(c)[c["l3_off"]:]
        if c["status"] == "bad_len":
            assert c["verdict_toy"] == c["verdict_toy_udp_skip"] == cgck.BAD_LEN
            continue
        fo = ip6ref.FIELD.get(c["nh"])
        if c["status"] != "ok" or fo is None:
            assert c["verdict_toy"] == c["verdict_toy_udp_skip"] == 0
            continue
        stored = int(p[c["l4_off"] + fo]) | int(p[c["l4_off"] + fo + 1]) << 8
        bad = cgck.BAD_L4 if stored != c["hi_zero"] else 0
        assert c["verdict_toy"] == bad, c["name"]
        assert c["verdict_toy_udp_skip"] == (0 if c["nh"] == 17 and stored == 0 else bad), c["name"]
        if c["name"].startswith("zero_class"):
            assert c["hi_zero"] == 0xFFFF
        if c["name"].startswith("corrupt_") or c["name"].startswith("udp_stored_zero"):
            assert c["verdict_toy"] == cgck.BAD_L4
        if "rfc1071_be" in c:
            be = c["rfc1071_be"]
            assert c["hi_zero"] == ((be & 255) << 8 | be >> 8)


def test_library_surface():
    """The flag, the exported synth entry point and the binding's method:
    absent before the IPv6 work."""
    assert cgck.IP6 == 1 << 9
    assert "cgck_synth_strided_ip6" in cgck.EXPORTS
    L = cgck.load()
    assert ctypes.cast(L.cgck_synth_strided_ip6, ctypes.c_void_p).value
    assert hasattr(cgck.Engine, "synth_strided_ip6")
    # without a context the call is refused cleanly (no device needed)
    assert L.cgck_synth_strided_ip6(None, None, 0, 64, 64, 6, 1, None) < 0
    assert b"cgck_synth_strided_ip6" in L.cgck_last_error()
