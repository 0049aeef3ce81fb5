"""CGCK_MIXED without a GPU: the public constants, the referee's consistency
with the oracle's IPv4 batch referee, the IPv6 referee and the reference's
compiled functions, the reference-made fixture tests/golden/mixed.json, and the
stamp referee of cgck_synth_imix_dual.  Nothing here runs a kernel."""
import os
import re

import numpy as np
import pytest

import ip6batches as B6
import ip6ref
import mixedbatches as MB
import mixedref as MR
from conftest import ROOT, load_golden

GEN = MR.IP | MR.L4
FLAG_SETS = (GEN, MR.L4, MR.IP, GEN | MR.ZERO_FIELDS, GEN | MR.VERIFY,
             GEN | MR.VERIFY | MR.V_IP_ZERO_IS_FFFF | MR.V_UDP_ZERO_SKIP)


def same(got, exp, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]}, " \
                          f"want {np.asarray(exp)[bad[:5]]}"


def test_public_constants():
    """include/cgck.h declares CGCK_MIXED = 1 << 10 and CGCK_NOT_IP = 1 << 3, the
    binding exports both, and the ABI version stays 2."""
    import cgck
    with open(os.path.join(ROOT, "include", "cgck.h")) as f:
        h = f.read()
    m = re.search(r"\bCGCK_MIXED\s*=\s*1u\s*<<\s*(\d+)", h)
    assert m and 1 << int(m.group(1)) == 1 << 10
    v = re.search(r"\bCGCK_NOT_IP\s*=\s*1u\s*<<\s*(\d+)", h)
    assert v and 1 << int(v.group(1)) == 8
    assert re.search(r"#define\s+CGCK_ABI_VERSION\s+2\b", h)
    assert cgck.MIXED == 1 << 10 and cgck.NOT_IP == 8
    assert "cgck_synth_imix_dual" in cgck.EXPORTS and re.search(r"\bint\s+cgck_synth_imix_dual\s*\(", h)
    assert hasattr(cgck.Engine, "synth_imix_dual")
    assert (MR.MIXED, MR.NOT_IP, MR.BAD_LEN) == (cgck.MIXED, cgck.NOT_IP, cgck.BAD_LEN)


def mixed_batch(seed, first_off=3):
    rng = np.random.default_rng(seed)
    return MB.packed(rng, MB.all_classes(rng), first_off)


def test_referee_all_ipv4_is_the_port(port):
    """On IPv4 packets without ICMP the referee is port.batch_desc."""
    rng = np.random.default_rng(11)
    frames = [f for f in MB.v4_classes(rng) if len(f) and not (len(f) > 9 and f[9] == 1)]
    buf, desc, offs, lens = MB.packed(rng, frames, 1)
    for flags in FLAG_SETS:
        exp, ever = port.batch_desc(buf.copy(), desc.view(np.uint8), len(desc), flags)
        out, ver = MR.expect(port, buf, offs, lens, flags | MR.MIXED)
        same(out, exp, f"out {flags:#x}")
        same(ver, ever, f"verdict {flags:#x}")


def test_referee_all_ipv6_is_ip6ref(port):
    """On IPv6 packets the referee is ip6ref.expect, the skip bit removed."""
    rng = np.random.default_rng(12)
    buf, desc, offs, lens = MB.packed(rng, MB.v6_classes(rng), 7)
    for flags in FLAG_SETS:
        exp, ever, _ = ip6ref.expect(port, buf, offs, lens, (flags & ~MR.V_UDP_ZERO_SKIP) | MR.IP6)
        out, ver = MR.expect(port, buf, offs, lens, flags)
        same(out, exp, f"out {flags:#x}")
        same(ver, ever, f"verdict {flags:#x}")
    toy, skip = (MR.expect(port, buf, offs, lens, f)[1] for f in FLAG_SETS[4:])
    udp0 = [i for i, (o, ln) in enumerate(zip(offs, lens)) if "v6_udpsum0" in MB.tags(buf[o:o + ln])]
    assert udp0 and all(skip[i] == MR.BAD_L4 for i in udp0)          # compared, and bad, whatever the skip flag says


def test_referee_pure_is_the_port(port):
    """The IPv4 semantics written out over in_cksum / udp_cksum give what
    port.batch_desc gives, ICMP by ip_p included, on every class."""
    buf, desc, offs, lens = mixed_batch(13)
    for flags in FLAG_SETS:
        exp, ever = MR.expect(port, buf, offs, lens, flags)
        out, ver = MR.expect_pure(port, buf, offs, lens, flags)
        same(out, exp, f"out {flags:#x}")
        same(ver, ever, f"verdict {flags:#x}")
    fam = MR.family(buf, offs, lens)
    _, ver = MR.expect(port, buf, offs, lens, GEN)
    assert np.all(ver[fam == 0] == MR.NOT_IP) and np.all(ver[fam == -1] == MR.BAD_LEN)
    assert (fam == 0).sum() >= 12 and (fam == -1).sum() >= 1


def test_referee_with_the_reference(port):
    """With the reference's compiled functions the referee gives the port's
    results (wherever oracle/_ref is built)."""
    import oracle
    R = oracle.reference()
    if R is None:
        pytest.skip("oracle/_ref is not built here")
    buf, desc, offs, lens = mixed_batch(14, 0)
    valid = MB.fill_fields(port, buf, offs, lens)
    for b in (buf, valid):
        for flags in FLAG_SETS:
            exp, ever = MR.expect(port, b, offs, lens, flags)
            out, ver = MR.expect_pure(R, b, offs, lens, flags)
            same(out, exp, f"out {flags:#x}")
            same(ver, ever, f"verdict {flags:#x}")


def golden_batch():
    g = load_golden("mixed.json")
    frames = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in g["packets"]]
    return g, frames


def test_golden(port):
    """The reference-made fixture: the port-based referee reproduces it, every
    class occurs in it, and its verify sets hold every verdict."""
    g, frames = golden_batch()
    assert 150 <= len(frames) <= 260
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mixed.json")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "ipv6.json"))
    have = set().union(*(MB.tags(f) for f in frames))
    assert MB.REQUIRED <= have, sorted(MB.REQUIRED - have)
    buf, desc, offs, lens = MB.packed(np.random.default_rng(1), frames, 5)
    assert set(g["sets"]) == {"gen_both", "gen_both_zero_fields", "verify_toy", "verify_bsd"}
    for name, s in g["sets"].items():
        assert s["flags"] & MR.MIXED
        out, ver = MR.expect(port, buf, offs, lens, s["flags"])
        same(out, np.array(s["out"], np.uint32), f"out {name}")
        same(ver, np.array(s["verdict"], np.uint8), f"verdict {name}")
    vt = np.array(g["sets"]["verify_toy"]["verdict"])
    for bit in (MR.BAD_IP, MR.BAD_L4, MR.BAD_LEN, MR.NOT_IP):
        assert np.count_nonzero(vt & bit)
    assert np.count_nonzero(vt == 0) >= 40


@pytest.mark.parametrize("stride,l3", [(0, 0), (2048, 14)])
def test_stamp_referee(port, stride, l3):
    """cgck_synth_imix_dual restated over port.stream_bytes: the frames of
    cgck_synth_imix / cgck_synth_imix_ring, family by k % 5, protocol by k % 7,
    that protocol's field zeroed where the frame holds it."""
    n, seed = 420, 0x5EED
    buf, desc, offs, lens = MB.imix_dual(port, n, seed, stride, l3)
    raw = port.stream_bytes(0, len(buf), seed)
    assert list(lens[:12]) == list(B6.IMIX_CYCLE)
    touched = np.zeros(len(buf), bool)
    seen = set()
    for k in range(n):
        o, ln = int(offs[k]), int(lens[k])
        p = buf[o:o + ln]
        six, pk = k % 5 < 2, k % 7
        proto = 6 if pk < 4 else 17 if pk < 6 else 58 if six else 1
        seen.add((k % 12, six))
        if six:
            assert bytes(p[:4]) == b"\x60\0\0\0" and (int(p[4]) << 8 | int(p[5])) == ln - 40 and p[6] == proto
            at = list(range(7)) + [40 + ip6ref.FIELD[proto], 41 + ip6ref.FIELD[proto]]
        else:
            assert p[0] == 0x45 and p[1] == 0 and (int(p[2]) << 8 | int(p[3])) == ln and p[9] == proto
            at = [0, 1, 2, 3, 9, 10, 11, 20 + MB.V4_FIELD[proto], 21 + MB.V4_FIELD[proto]]
            assert not p[10] and not p[11]
        fa = MB.l4_field_at(p)
        assert fa is not None and not p[fa] and not p[fa + 1]       # every IMIX frame holds its field
        touched[[o + a for a in at]] = True
    assert len(seen) == 24                                           # every cycle position sees both families
    same(buf[~touched], raw[~touched], "bytes outside the stamps")
    out, ver = MR.expect(port, buf, offs, lens, GEN | MR.VERIFY)
    assert not np.any(ver & (MR.BAD_LEN | MR.NOT_IP))
