"""The edge-class corpus of edgecases.py, validated without a GPU the way
test_lpf_batches_cpu.py validates its builders: for every batch the GPU cells
of test_gpu_edgecases.py use, the oracle's answer on the finished buffer shows
that each class is what its label says, the class counts are the ones fixed by
construction, and the layout meets its rotation conditions."""
from collections import Counter

import numpy as np
import pytest

import cgck
import edgecases as E
import oracle

# (server cells that differ only in their request plan share one batch: corpus_cell)
ALL = sorted({E.corpus_cell(cell) for fam in E.CELLS for cell in E.cells(fam)}, key=E.cell_id)


def unique(b, cls):
    return len({id(f) for f in b.frames if f.cls == cls})


@pytest.mark.parametrize("cell", ALL, ids=E.cell_id)
def test_batch_is_what_its_labels_say(port, cell):
    (layout, lens, _), flags = cell
    b = E.cell_batch(port, cell)
    before = b.buf.copy()
    out, ver, after = E.expect(port, b, flags)
    assert np.array_equal(b.buf, before), "the expectation changed the corpus"
    ip6, raw = bool(flags & cgck.IP6), bool(flags & cgck.RAW)
    lo, hi = out & 0xFFFF, out >> 16
    L = b.lens
    assert E.disjoint(b) and b.n <= E.MAX_FRAMES
    assert int(b.starts[-1] + L[-1]) <= len(b.buf)

    # the exact class counts
    if layout == "plain64":
        assert b.n == E.PLAIN64_N == 199 and set(L.tolist()) == {64}
        assert all(int(f.data[0]) == 0x45 for f in b.frames)
        want = {"fill": 1, "zero_ip": 3, "zero_l4": 3, "zero_both": 3}
        if E.reads_fields(flags) and not raw:
            want["stored"] = E.counts4(64, flags)["stored"]
    else:
        every = [lens] if np.isscalar(lens) else lens
        want = Counter()
        for ln in every:
            want.update(E.counts6(ln, flags) if ip6 else E.counts4(ln, flags))
    classes = {f.cls for f in b.frames} - {"pad"}
    assert classes == {c for c, k in want.items() if k}
    for c in classes:
        assert unique(b, c) == want[c], c

    # crafted zero sums: 0xFFFF in the half (or halves) the frame was crafted for
    for i, f in enumerate(b.frames):
        if f.lo_ffff and (raw or (flags & cgck.IP and not ip6)):
            assert lo[i] == 0xFFFF, b.labels([i])
        if f.hi_ffff and flags & cgck.L4 and not raw:
            assert hi[i] == 0xFFFF, b.labels([i])
        if f.cls.startswith("zero_"):
            assert f.lo_ffff or f.hi_ffff
    if not ip6 and (raw or flags & cgck.IP) and layout != "plain64":
        zeros = [i for i, f in enumerate(b.frames) if f.label == "fill:00"]
        assert zeros and all(lo[i] == 0xFFFF for i in zeros)

    # planted fields: the verdict the rules intend
    key = flags & ~(cgck.STORE | cgck.IP6)
    if flags & cgck.VERIFY and want.get("stored"):   # (none at 20 bytes: no room for a field)
        stored = [i for i, f in enumerate(b.frames) if f.cls == "stored"]
        for i in stored:
            w = b.frames[i].want
            assert ver[i] == (w if ip6 else w[key]), b.labels([i])
        assert {int(ver[i]) for i in stored} >= {0, cgck.BAD_L4}   # good verdicts and bad ones
    elif not flags & cgck.VERIFY and not raw:
        assert not (ver & 3).any()

    # BAD_LEN
    if not ip6 and not raw:
        sweep = [i for i, f in enumerate(b.frames) if f.cls == "hl_sweep"]
        short = [i for i in sweep if b.frames[i].hl * 4 > L[i]]
        assert [i for i in sweep if ver[i] & cgck.BAD_LEN] == short
        ff = [i for i, f in enumerate(b.frames) if f.label == "fill:ff" and L[i] < 60]
        assert sorted(np.nonzero(ver & cgck.BAD_LEN)[0].tolist()) == sorted(short + ff)
        if layout != "plain64" and int(L.min()) < 60:
            assert len(short) > 0
        assert not out[short + ff].any()
    if not flags & cgck.STORE:
        assert np.array_equal(after, before)

    # the rotation: every class at every index mod 4, in two lanes or more, and
    # once in the last, partial 64-frame chunk
    if layout == "plain64":
        assert b.n % 64 == 7
        for c in classes:
            lanes = {i % 64 for i, f in enumerate(b.frames) if f.cls == c}
            assert len(lanes) >= 2 and {i % 4 for i in lanes} == {0, 1, 2, 3}, c
        return
    assert b.n % 64 != 0
    tail = range(b.n - b.n % 64, b.n)
    assert Counter(b.frames[i].cls for i in tail) == Counter(classes)
    for c in classes:
        at = [i for i, f in enumerate(b.frames) if f.cls == c and i < tail[0]]
        assert {i % 4 for i in at} == {0, 1, 2, 3}, c
        assert len({i % 64 for i in at}) >= 2, c


TABLE = {   # (IP field, L4 field) where both sums are 0xFFFF -> the verdict under (VERIFY_BSD, VERIFY_TOY)
    6: {(0xFFFF, 0xFFFF): (0, 0), (0, 0): (2, 3), (0, 0xFFFF): (0, 1), (0xFFFF, 0): (2, 2)},
    17: {(0xFFFF, 0xFFFF): (0, 0), (0, 0): (0, 3), (0, 0xFFFF): (0, 1), (0xFFFF, 0): (0, 2)},
    1: {(0xFFFF, 0xFFFF): (0, 0), (0, 0): (0, 1), (0, 0xFFFF): (0, 1), (0xFFFF, 0): (0, 0)},   # no L4 field
}


@pytest.mark.parametrize("ip_len", [64, 99, 1500])
def test_each_rule_decides_a_verdict(port, ip_len):
    """The four field pairs on a frame whose two sums are 0xFFFF: the 0 = 0xFFFF
    rule of the IP field and the UDP zero-skip rule each decide a verdict."""
    for vi, flags in enumerate((cgck.VERIFY_BSD, cgck.VERIFY_TOY)):
        rng = np.random.default_rng(ip_len)
        seen = 0
        for f in E.stored_frames(port, rng, ip_len, flags):
            if "zero_both" not in f.label:
                continue
            _, pair, p = f.label.split("/")
            ipf, l4f = (int(x, 16) for x in pair.split("."))
            out, ver = port.batch_strided(f.data.copy(), 1, ip_len, 0, ip_len, flags)
            assert out[0] == 0xFFFFFFFF, f.label
            assert ver[0] == TABLE[int(p[1:])][(ipf, l4f)][vi] == f.want[flags], f.label
            seen += 1
        assert seen == 12
    # ICMP's field exists without the pseudo-header
    flags = E.NOPS_VERIFY
    got = {f.label.split("/")[1]: int(port.batch_strided(f.data.copy(), 1, ip_len, 0, ip_len, flags)[1][0])
           for f in E.stored_frames(port, np.random.default_rng(1), ip_len, flags) if f.label.endswith("/p1") and "zero_both" in f.label}
    assert got == {"ffff.ffff": 0, "0000.0000": 3, "0000.ffff": 1, "ffff.0000": 2}


@pytest.mark.parametrize("ip_len", [64, 99, 1500])
@pytest.mark.parametrize("flags", [E.GZ, E.GZ | cgck.L4_NOPSEUDO])
def test_zero_classes_all_27(port, ip_len, flags):
    rng = np.random.default_rng(ip_len + flags)
    fr = [f for f in E.frames4(port, rng, ip_len, flags) if f.cls == "zero_both"]
    assert len(fr) == 9
    for f in fr:
        assert port.batch_strided(f.data.copy(), 1, ip_len, 0, ip_len, flags)[0][0] == 0xFFFFFFFF, f.label


def test_against_the_reference_build(port):
    """GEN_BOTH frames whose header fits, ip_hl 0..4 included: the oracle's two
    halves are the reference's own in_cksum / udp_cksum of the same bytes."""
    R = oracle.reference()
    if R is None:
        pytest.skip("no reference build (oracle/_ref)")
    checked = low = 0
    for fam in ("lpa", "dstr", "slot2"):
        for cell in E.cells(fam):
            if cell[1] != cgck.GEN_BOTH:
                continue
            b = E.cell_batch(port, cell)
            out, ver, _ = E.expect(port, b, cgck.GEN_BOTH)
            for i in {id(f): i for i, f in enumerate(b.frames)}.values():
                f = b.frames[i].data
                hl, ln = (int(f[0]) & 15) * 4, len(f)
                if hl > ln:
                    assert ver[i] == cgck.BAD_LEN
                    continue
                assert out[i] & 0xFFFF == R.in_cksum(f, 0, hl), b.labels([i])
                assert out[i] >> 16 == R.udp_cksum(f, 0, ln - hl), b.labels([i])
                checked += 1
                low += hl < 20
    assert checked > 1000 and low > 100
