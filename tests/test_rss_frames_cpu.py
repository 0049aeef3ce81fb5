"""The per-frame RSS hash without a GPU: the referee (tests/rssref.py) against
the reference-made fixture and the reference's rss_hash4, the class batch's
coverage, the fuzz mix, the header's constants against the binding's, and the
three exported symbols."""
import os
import re

import numpy as np
import pytest

import cgck
import oracle
import rssbatches as RB
import rssref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return load_golden("rss_frames.json")


def frames_of(hexes):
    return [np.frombuffer(bytes.fromhex(h), np.uint8) for h in hexes]


def test_referee_reproduces_the_fixture(port, gold):
    key = np.frombuffer(bytes.fromhex(gold["key"]), np.uint8)
    for v in gold["ms"]:
        f = frames_of([v["frame"]])[0]
        for hf, want in ((rssref.RSS_TCP, v["tcp"]), (RB.HF_ALL, v["tcp"]), (0, v["ip"]), (rssref.RSS_UDP, v["ip"])):
            h, kind, _ = rssref.expect(port, f, [0], [len(f)], key, hf)
            assert int(h[0]) == want, (v, hf)
            assert int(kind[0]) & rssref.RSS_L4 == (rssref.RSS_L4 if hf & rssref.RSS_TCP else 0)
    # the published values themselves (Microsoft, "Verifying the RSS Hash Calculation")
    six = [v for v in gold["ms"] if v["frame"].startswith("6")]
    assert [(v["tcp"], v["ip"]) for v in six] == [(t, i) for *_, t, i in RB.MS_IP6]
    assert (six[0]["tcp"], six[0]["ip"]) == (0x40207D3D, 0x2CC18CD5)
    frames = frames_of(gold["frames"])
    rng = np.random.default_rng(1)
    buf, _, offs, lens = RB.packed(rng, frames, 0)
    for name, s in gold["sets"].items():
        h, kind, _ = rssref.expect(port, buf, offs, lens, key, s["hf"])
        assert h.tolist() == s["hash"], name
        assert kind.tolist() == s["kind"], name
    # and, where the reference's own build is present, side by side
    R = oracle.reference_rss()
    if R is not None:
        assert bytes(R.key).hex() == gold["key"]
        for name, s in gold["sets"].items():
            h, kind, _ = rssref.expect(R, buf, offs, lens, R.key, s["hf"])
            assert h.tolist() == s["hash"] and kind.tolist() == s["kind"], name


def test_ipv4_l4_hash_is_rss_hash4(port, gold):
    """hash & 0x7F of an IPv4 frame that hashed its ports = the reference's
    rss_hash4(laddr = ip_dst, faddr = ip_src, lport = dport, fport = sport)."""
    R = oracle.reference_rss() or port
    key = np.frombuffer(bytes.fromhex(gold["key"]), np.uint8).copy()
    rng = np.random.default_rng(3)
    frames = [f for f in RB.all_classes(rng) + RB.fuzz(rng, 300)
              if rssref.tuple_of(f, len(f), RB.HF_ALL)[0] == rssref.RSS_L4]
    assert len(frames) > 60
    for f in frames:
        hl = 4 * (int(f[0]) & 15)
        src, dst = (int.from_bytes(bytes(f[a:a + 4]), "little") for a in (12, 16))
        sport, dport = (int.from_bytes(bytes(f[a:a + 2]), "little") for a in (hl, hl + 2))
        h, _, _ = rssref.expect(port, f, [0], [len(f)], key, RB.HF_ALL, mask=0x7F)
        assert int(h[0]) == R.rss_hash4(dst, src, dport, sport, key)


def test_class_batch_covers_required():
    frames = RB.all_classes(np.random.default_rng(31))
    have = set().union(*(RB.tags(f) for f in frames))
    assert RB.REQUIRED <= have, sorted(RB.REQUIRED - have)
    # the case the checksum rule calls BAD_LEN and the hash does not
    import ip6ref
    cut = [f for f in frames if "v6_nh6_plus10" in RB.tags(f)]
    assert cut and all(ip6ref.walk(f, len(f))[2] == ip6ref.BADLEN for f in cut)
    assert all(rssref.tuple_of(f, len(f), RB.HF_ALL)[0] == rssref.RSS_IP6 | rssref.RSS_L4 for f in cut)


def test_fuzz_mix():
    """At least 60 % of the fuzz frames carry a hash and each hashed kind is at
    least 5 % of them all, so a comparison over them cannot pass on BAD_LEN alone."""
    frames = RB.fuzz(np.random.default_rng(77), 5000)
    kinds = np.array([rssref.tuple_of(f, len(f), RB.HF_ALL)[0] for f in frames])
    assert np.count_nonzero(rssref.hashed(kinds)) >= 0.60 * len(frames)
    for k in (0, rssref.RSS_L4, rssref.RSS_IP6, rssref.RSS_IP6 | rssref.RSS_L4):
        assert np.count_nonzero(kinds == k) >= 0.05 * len(frames), k
    assert np.count_nonzero(kinds == rssref.BAD_LEN) and np.count_nonzero(kinds == rssref.NOT_IP)


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "cgck.h")).read()
    for name, val in (("RSS_TCP", cgck.RSS_TCP), ("RSS_UDP", cgck.RSS_UDP), ("RSS_L4", cgck.RSS_L4),
                      ("RSS_IP6", cgck.RSS_IP6), ("BAD_LEN", cgck.BAD_LEN), ("NOT_IP", cgck.NOT_IP)):
        m = re.search(rf"\bCGCK_{name}\s*=\s*1u << (\d+)", src)
        assert m and 1 << int(m.group(1)) == val, name
    assert (cgck.RSS_TCP, cgck.RSS_UDP, cgck.RSS_L4, cgck.RSS_IP6, cgck.BAD_LEN, cgck.NOT_IP) == \
        (rssref.RSS_TCP, rssref.RSS_UDP, rssref.RSS_L4, rssref.RSS_IP6, rssref.BAD_LEN, rssref.NOT_IP)
    import ctypes
    assert ctypes.sizeof(cgck.RssSpec) == 24 and ctypes.sizeof(cgck.RssRes) == 32


def test_library_exports_the_frame_hash():
    L = cgck.load()
    for name in ("cgck_rss_strided", "cgck_rss_desc", "cgck_rss_desc_host"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert L.cgck_abi_version() == 2
