"""CPU tests of the cgck_l2_desc test infrastructure (no GPU): the class corpus
covers what the contract names, the referee (tests/l2ref.py) answers hand-written
frames as each rule says, it agrees with the reference stack's replay
(oracle/stack_replay.c: bsd_eth_in + ip_input) on the receive corpus, and the
binding's constants are the header's."""
import os
import re

import numpy as np

import cgck
import l2batches as LB
import l2ref
import rxcorpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = (0x02, 0, 0, 0, 0, 1)                 # a unicast destination
S = (0x02, 0, 0, 0, 0, 2)


def fr(*parts):
    return np.array([b for p in parts for b in p], np.uint8)


def v4(total, n, b0=0x45):
    p = [b0, 0, total >> 8, total & 255] + [0xAA] * 60
    return tuple(p[:n])


def v6(plen, n, b0=0x60):
    p = [b0, 0, 0, 0, plen >> 8, plen & 255] + [0xBB] * 60
    return tuple(p[:n])


def test_corpus_covers_required():
    items = LB.classes(np.random.default_rng(11))
    seen = set()
    for it in items:
        seen |= LB.tags(it)
    assert not LB.REQUIRED - seen, sorted(LB.REQUIRED - seen)
    assert len(items) < 400
    # every class, flag combination and tag count also lies in the 64-byte slots of the tiled bursts
    buf, raw, m = LB.tiled(items, 1)
    assert m > 200
    cls = l2ref.expect(*LB.tiled(items, m)[:2])[1]
    assert set((cls & 15).tolist()) == set(range(l2ref.NCLASS))
    assert {int(c) & 0xD0 for c in cls} >= {0, l2ref.VLAN, l2ref.BCAST, l2ref.MCAST, l2ref.VLAN | l2ref.BCAST,
                                            l2ref.VLAN | l2ref.MCAST}


T1, T2, IP, IP6, ARP = (0x81, 0x00), (0x88, 0xA8), (0x08, 0x00), (0x86, 0xDD), (0x08, 0x06)
TCI = (0x20, 0x05)
R = l2ref
RULES = (
    # (rule, frame, l3_off, class, flags, off, ip_len_out)
    ("1: L 13", fr(U, S, (0x08,)), 0, R.RUNT, 0, 14, 0),
    ("1: L 0", fr(), 0, R.RUNT, 0, 14, 0),
    ("2: no room for the first tag", fr(U, S, T1, TCI, (0x08,)), 0, R.RUNT, 0, 14, 0),
    ("2: no room for the second tag", fr(U, S, T1, TCI, T2, TCI, (0x08,)), 0, R.RUNT, R.VLAN, 18, 0),
    ("2: one tag", fr(U, S, T1, TCI, IP, v4(20, 20)), 0, R.IP4, R.VLAN, 18, 20),
    ("2: two tags, 88A8 then 8100", fr(U, S, T2, TCI, T1, TCI, IP, v4(20, 20)), 0, R.IP4, R.VLAN, 22, 20),
    ("2: a third tag", fr(U, S, T1, TCI, T1, TCI, T2, TCI, IP, v4(20, 20)), 0, R.OTHER, R.VLAN, 22, 0),
    ("3: broadcast", fr((0xFF,) * 6, S, ARP, (0,) * 28), 0, R.ARP, R.BCAST, 14, 0),
    ("3: multicast", fr((0x01, 0, 0x5E, 0, 0, 1), S, IP, v4(20, 20)), 0, R.IP4, R.MCAST, 14, 20),
    ("3: five FF bytes are multicast", fr((0xFF,) * 5, (0xFE,), S, IP, v4(20, 20)), 0, R.IP4, R.MCAST, 14, 20),
    ("3: flags on a drop class", fr((0xFF,) * 6, S, IP, v4(20, 19)), 0, R.TOOSMALL, R.BCAST, 14, 0),
    ("3: flags on a runt with L >= 14", fr((0xFF,) * 6, S, T1), 0, R.RUNT, R.BCAST, 14, 0),
    ("5: avail 19", fr(U, S, IP, v4(19, 19)), 0, R.TOOSMALL, 0, 14, 0),
    ("5: version 5", fr(U, S, IP, v4(20, 20, 0x55)), 0, R.BADVERS, 0, 14, 0),
    ("5: hl 16", fr(U, S, IP, v4(20, 20, 0x44)), 0, R.BADHLEN, 0, 14, 0),
    ("5: hl 24 past avail 23", fr(U, S, IP, v4(24, 23, 0x46)), 0, R.BADHLEN, 0, 14, 0),
    ("5: total 19 below hl", fr(U, S, IP, v4(19, 40)), 0, R.BADLEN, 0, 14, 0),
    ("5: total one past avail", fr(U, S, IP, v4(41, 40)), 0, R.TOOSHORT, 0, 14, 0),
    ("5: a 40-byte segment in a 60-byte frame", fr(U, S, IP, v4(40, 46)), 0, R.IP4, 0, 14, 40),
    ("5: version before header length", fr(U, S, IP, v4(20, 20, 0x54)), 0, R.BADVERS, 0, 14, 0),
    ("5: header length before total", fr(U, S, IP, v4(0, 20, 0x44)), 0, R.BADHLEN, 0, 14, 0),
    ("6: avail 39", fr(U, S, IP6, v6(0, 39)), 0, R.TOOSMALL, 0, 14, 0),
    ("6: version 4", fr(U, S, IP6, v6(0, 40, 0x45)), 0, R.BADVERS, 0, 14, 0),
    ("6: payload one past the frame", fr(U, S, IP6, v6(9, 48)), 0, R.TOOSHORT, 0, 14, 0),
    ("6: padded", fr(U, S, IP6, v6(6, 48)), 0, R.IP6, 0, 14, 46),
    ("6: payload length 0 (a jumbogram's)", fr(U, S, IP6, v6(0, 60)), 0, R.IP6, 0, 14, 40),
    ("6: total above 65535", fr(U, S, IP6, v6(0xFFFF, 60)), 0, R.TOOSHORT, 0, 14, 0),
    ("7: ARP", fr(U, S, ARP), 0, R.ARP, 0, 14, 0),
    ("7: an 802.3 length", fr(U, S, (0x00, 0x2E), v4(20, 46)), 0, R.OTHER, 0, 14, 0),
    ("7: LLDP", fr(U, S, (0x88, 0xCC), (1, 2, 3)), 0, R.OTHER, 0, 14, 0),
    ("8: l3_off + 14 = 65535", fr(U, S, IP, v4(20, 20)), 65521, R.IP4, 0, 14, 20),
    ("8: l3_off + 14 = 65536", fr(U, S, IP, v4(20, 20)), 65522, R.RUNT, 0, 14, 0),
    ("8: l3_off + 18 = 65536, tagged", fr((0xFF,) * 6, S, T1, TCI, ARP), 65518, R.RUNT, R.VLAN | R.BCAST, 18, 0),
)


def test_referee_rules():
    """One hand-written frame per rule, and the descriptor each becomes."""
    for what, f, l3, c, flags, off, ip_len in RULES:
        assert l2ref.one(f, len(f), l3) == (c, flags, off, ip_len), what
        buf = np.concatenate((np.full(l3 + 7, 0x81, np.uint8), f, np.full(9, 0x45, np.uint8)))
        raw = np.array([(7, l3, len(f))], l2ref.DESC_DTYPE)
        out, cls, count = l2ref.expect(buf, raw)
        assert tuple(out[0]) == (7, l3 if c == R.RUNT else l3 + off, ip_len), what
        assert cls[0] == c | flags, what
        want = np.zeros(12, np.uint32)
        want[c] = 1
        want[10] = bool(flags & (R.BCAST | R.MCAST))
        want[11] = bool(flags & R.VLAN)
        assert np.array_equal(count, want) and np.array_equal(count, LB.counts(cls)), what


def test_against_reference_replay(port):
    """bsd_eth_in + ip_input as the oracle replays them (both checksum flags 0: no
    frame is dropped on a sum) against the referee, on the receive corpus."""
    rng = np.random.default_rng(12)
    frames = rxcorpus.corpus(rng, port, 600, clean=False)
    buf, desc = rxcorpus.ring(frames)
    fns = port.fn_pointers()
    res, _ = port.replay_rx(fns[0], fns[1], buf.copy(), desc.view(np.uint8), len(desc), 0, 0, 0)
    raw = desc.copy()
    raw["l3_off"] = 0                                   # rxcorpus.ring: the Ethernet header opens the slot
    raw["ip_len"] = desc["ip_len"] + 14
    out, cls, count = l2ref.expect(buf, raw)
    passed = padded = 0
    for k, p in enumerate(frames):
        c, avail = int(cls[k]) & 15, len(p)
        total = int(p[2]) << 8 | int(p[3]) if avail >= 4 else None
        if res[k] != port.R_DROP:
            passed += 1
            assert c not in l2ref.DROPS and c == l2ref.IP4, (k, c, int(res[k]))
            assert int(out["ip_len"][k]) == min(total, avail), k
            assert int(out["l3_off"][k]) == 14
        if c == l2ref.IP4 and total < avail:            # Ethernet padding (rxcorpus: kind 30..39)
            padded += 1
            assert int(out["ip_len"][k]) < int(raw["ip_len"][k]) - 14, k
    assert passed > 300 and padded > 20
    assert all(count[c] > 0 for c in (l2ref.IP4, l2ref.TOOSMALL, l2ref.BADVERS, l2ref.BADHLEN, l2ref.BADLEN,
                                      l2ref.TOOSHORT))
    # every frame ip_input drops by one of its five length checks is dropped by the replay too
    assert all(res[k] == port.R_DROP for k in range(len(frames)) if int(cls[k]) & 15 in l2ref.DROPS)


def test_synth_eth_restatement_round_trip(port):
    """The restated cgck_synth_eth over the restated dual-stack ring: the referee
    returns the set's own descriptors, padding included."""
    import mixedbatches as MB
    buf, desc, offs, lens = MB.imix_dual(port, 25, 0x5EED, stride=2048, l3_off=18)
    raw = LB.synth_eth(buf, desc, 8, 0xE7)
    assert list(raw["l3_off"][:10]) == [0, 4, 4, 4, 4, 4, 4, 4, 0, 4]
    assert int(raw["ip_len"][0]) == 64 + 18 and int(raw["ip_len"][1]) == 576 + 14
    out, cls, count = l2ref.expect(buf, raw)
    assert np.array_equal(out, desc.astype(l2ref.DESC_DTYPE))
    assert count[l2ref.IP4] == 15 and count[l2ref.IP6] == 10 and count[11] == 4 and count[10] == 0


def test_constants_and_exports():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    names = ("IP4", "IP6", "ARP", "OTHER", "RUNT", "TOOSMALL", "BADVERS", "BADHLEN", "BADLEN", "TOOSHORT", "NCLASS")
    for i, x in enumerate(names):
        m = re.search(rf"\bCGCK_L2_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == i == getattr(cgck, f"L2_{x}"), x
        if x != "NCLASS":
            assert getattr(l2ref, x) == i and l2ref.NAMES[i] == x
    for x, bit in (("VLAN", 4), ("BCAST", 6), ("MCAST", 7)):
        m = re.search(rf"\bCGCK_L2_{x} = 1u << (\d+)", hdr)
        assert m and int(m.group(1)) == bit and getattr(cgck, f"L2_{x}") == 1 << bit == getattr(l2ref, x), x
    m = re.search(r"#define CGCK_L2_NCOUNT (\d+)", hdr)
    assert m and int(m.group(1)) == cgck.L2_NCOUNT == l2ref.NCOUNT == 12
    import ctypes
    assert ctypes.sizeof(cgck.L2Res) == 3 * ctypes.sizeof(ctypes.c_void_p)
    L = cgck.load()
    for name in ("cgck_l2_desc", "cgck_synth_eth"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert "#define CGCK_ABI_VERSION 2" in hdr and L.cgck_abi_version() == 2
