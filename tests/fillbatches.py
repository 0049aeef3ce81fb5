"""Batch builders of the fill / counter tests (test_gpu_lpf.py, validated on the
CPU by test_lpf_batches_cpu.py): packed batches (batches.packed_batch), the
same frames in 2048-byte ring slots at +14, planted corruption, and the
reference bytes of the device's IMIX generators.  Every builder yields frames
that are pairwise disjoint: a CGCK_STORE batch must not overlap."""
import numpy as np

import cgck
from batches import packed_batch

IMIX_CYCLE = [64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576]   # the generators' 7:4:1 cycle


def packed(rng, n, lens, first_off=0, plain=False):
    """(buf, desc): n frames back to back (batches.packed_batch).  plain: every
    frame of 20 bytes or more is TCP with ip_hl = 5, so each one verifies and a
    flipped payload byte is always seen (the counter tests)."""
    buf, desc = packed_batch(rng, n, lens, first_off=first_off)
    if plain:
        s = starts(desc)
        for k in np.nonzero(desc["ip_len"] >= 20)[0]:
            buf[s[k]] = 0x45
            buf[s[k] + 9] = 6
    return buf, desc


def ring(rng, n, lens, slot=2048, l3_off=14):
    """(buf, desc): frame k at slot * k + l3_off, lengths drawn from `lens`
    (at most slot - l3_off), IPv4 headers as packed_batch stamps them."""
    L = rng.choice(np.asarray(lens), n)
    assert int(L.max()) + l3_off <= slot
    buf = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
    for k in range(n):
        o, ln = k * slot + l3_off, int(L[k])
        if ln < 1:
            continue
        buf[o] = 0x40 | (5 if rng.random() < 0.7 else int(rng.integers(0, 16)))
        if ln > 9:
            buf[o + 9] = rng.choice([6, 6, 17, 1, int(rng.integers(0, 256))])
        if ln >= 4:
            buf[o + 2], buf[o + 3] = (ln >> 8) & 0xFF, ln & 0xFF
    desc = np.zeros(n, cgck.DESC_DTYPE)
    desc["frame_off"] = np.arange(n, dtype=np.int64) * slot
    desc["l3_off"] = l3_off
    desc["ip_len"] = L
    return buf, desc


def starts(desc):
    return desc["frame_off"].astype(np.int64) + desc["l3_off"]


def disjoint(desc):
    """True when no two non-empty frames of the batch share a byte."""
    s, ln = starts(desc), desc["ip_len"].astype(np.int64)
    keep = ln > 0
    s, ln = s[keep], ln[keep]
    order = np.argsort(s, kind="stable")
    s, ln = s[order], ln[order]
    return bool(np.all(s[1:] >= s[:-1] + ln[:-1]))


def fields_coincide(buf, desc):
    """Frames whose two checksum fields are the same two bytes (ip_hl * 4 + the
    L4 field's offset = 10: ip_hl 1 with UDP, ip_hl 2 with ICMP).  A fill stores
    the IP sum there and then the L4 sum over it, so such a frame cannot verify
    on both; the builders' random headers produce a few."""
    s, ln = starts(desc), desc["ip_len"].astype(np.int64)
    ok = ln >= 20
    hl = np.where(ok, (buf[np.where(ok, s, 0)] & 15).astype(np.int64) * 4, 0)
    proto = np.where(ok, buf[np.where(ok, s + 9, 0)], 0)
    fo = np.select([proto == 6, proto == 17, proto == 1], [16, 6, 2], -1)
    return ok & (ln >= hl) & (fo >= 0) & (hl + fo == 10) & (hl + fo + 2 <= ln)


def corrupt(buf, desc, every):
    """Flip one byte inside every `every`-th frame of at least 40 bytes (byte 30:
    past an ip_hl = 5 header, so the L4 sum changes and nothing else does).
    Returns the indices of the frames hit."""
    s, ln = starts(desc), desc["ip_len"]
    hit = [k for k in range(0, len(desc), every) if ln[k] >= 40]
    for k in hit:
        buf[s[k] + 30] ^= 0x5A
    return np.asarray(hit, np.int64)


def synth_imix_ref(port, n, seed, slot=0, l3_off=0):
    """The bytes cgck_synth_imix (slot 0) / cgck_synth_imix_ring write, from the
    oracle: the seeded stream with an IPv4 header stamped on every frame.
    (buf, desc)."""
    desc = np.zeros(n, cgck.DESC_DTYPE)
    if slot:
        nbytes = n * slot
        offs = np.arange(n, dtype=np.int64) * slot + l3_off
        lens = np.asarray([IMIX_CYCLE[k % 12] for k in range(n)])
        desc["frame_off"] = np.arange(n, dtype=np.int64) * slot
        desc["l3_off"] = l3_off
    else:
        nbytes = cgck.load().cgck_imix_bytes(n)
        pairs = [port.imix_desc(k) for k in range(n)]
        offs = np.asarray([p[0] for p in pairs], np.int64)
        lens = np.asarray([p[1] for p in pairs])
        desc["frame_off"] = offs
    desc["ip_len"] = lens
    buf = port.stream_bytes(0, nbytes, seed)
    for k in range(n):
        port.stamp_header(buf, int(offs[k]), int(lens[k]))
    return buf, desc
