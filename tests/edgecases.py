"""A deterministic corpus of header, zero-sum and stored-field edge classes,
built to go through every kernel family's own finishing code
(test_gpu_edgecases.py; validated without a GPU by test_edgecases_cpu.py).

Nothing here calls the library under test.  The oracle (oracle.port(), and
ip6ref over it for IPv6) is used twice: while a frame is crafted (compute the
sum, retune a word) and, by the tests, on the finished buffer for the
expectation.

Classes (Frame.label is "<class>:<detail>", Frame.cls the class):
  hl_sweep   ip_hl 0..15 x ip_p {6, 17, 1, 253}, random bytes (ip_hl * 4 >
             ip_len are the BAD_LEN cases; ip_hl 1 / UDP and ip_hl 2 / ICMP
             share the two checksum fields' bytes)
  fill       all 0x00, all 0xFF, a plain header over a 0xFF payload
  zero_ip / zero_l4 / zero_both
             the header sum, the L4 sum or both are multiples of 65535 under
             the batch's own flags (out = 0xFFFF); under CGCK_RAW the whole
             region's sum is
  stored     checksum fields planted to decide a verdict: correct, off by one,
             0 and 0xFFFF where the sum is 0xFFFF, a UDP field of 0
  pad        ordinary frames that fill a layout up (ip_hl 5, TCP)
"""
from dataclasses import dataclass, field

import numpy as np

import cgck
import ip6ref

PROTOS = (6, 17, 1, 253)
ZERO_PROTOS = (6, 17, 1)
ZERO_HLS = (5, 6, 10)
NH6 = (6, 17, 58, 59, 253)
MAX_FRAMES = 1100
SLOT, SLOT_L3 = 2048, 14


@dataclass
class Frame:
    label: str
    data: np.ndarray
    lo_ffff: bool = False    # crafted: the oracle's out.lo is 0xFFFF
    hi_ffff: bool = False    # crafted: the oracle's out.hi is 0xFFFF
    want: object = None      # stored: {flag set: intended verdict}
    hl: int = -1             # hl_sweep: the ip_hl planted

    @property
    def cls(self):
        return self.label.split(":")[0]


def reads_fields(flags):
    return bool(flags & (cgck.ZERO_FIELDS | cgck.VERIFY))


def craft_flags(flags):
    """The flags a frame is crafted under: both halves, the batch's pseudo-header
    choice, the fields read as zero exactly when the batch reads them so."""
    f = cgck.IP | cgck.L4 | (flags & cgck.L4_NOPSEUDO)
    return f | (cgck.ZERO_FIELDS if reads_fields(flags) else 0)


def field_off(proto, flags):
    """The L4 checksum field's offset after the header, or -1 (include/cgck.h)."""
    if flags & cgck.L4_NOPSEUDO:
        return 2 if proto == 1 else -1
    return {6: 16, 17: 6}.get(proto, -1)


def one(port, f, flags):
    """The oracle's (lo, hi) of one IPv4 frame; the frame is not changed."""
    out, _ = port.batch_strided(f.copy(), 1, len(f), 0, len(f), flags & ~cgck.STORE)
    return int(out[0]) & 0xFFFF, int(out[0]) >> 16


def retune(f, at, cks):
    """Subtract the sum a checksum `cks` stands for from the 16-bit word at `at`
    (an even offset of the summed region), so the region's sum becomes a multiple
    of 65535: tests/golden's make_golden.py does the same with ip_id."""
    s = (0xFFFF - cks) % 65535
    w = int(f[at]) | int(f[at + 1]) << 8
    w = (w - s) % 65535
    f[at], f[at + 1] = w & 255, w >> 8


def put16(f, at, v):
    f[at], f[at + 1] = v & 255, v >> 8


def off_by_one(v):
    return v + 1 if v < 0xFFFF else v - 1   # a checksum is never 0, so neither is this


def header4(rng, ip_len, hl, proto, sane=False):
    """Random bytes under ip_v 4, ip_hl, ip_len and ip_p.  sane: also what a
    receiving stack checks before it asks for a checksum (oracle/stack_replay.c):
    no fragment (DF alone), a TTL, and where they fit a TCP data offset of 5 and
    a UDP length of the whole L4 region, so a crafted frame reaches its verdict."""
    f = rng.integers(0, 256, ip_len, dtype=np.uint8)
    f[0] = 0x40 | hl
    f[2], f[3] = ip_len >> 8, ip_len & 255
    f[9] = proto
    if sane:
        f[6], f[7], f[8] = 0x40, 0, 64
        l4 = ip_len - hl * 4
        if proto == 6 and l4 >= 13:
            f[hl * 4 + 12] = 0x50 | (int(f[hl * 4 + 12]) & 15)
        if proto == 17 and l4 >= 6:
            f[hl * 4 + 4], f[hl * 4 + 5] = l4 >> 8, l4 & 255
    return f


def zero_frame(port, rng, ip_len, hl, proto, flags, which, sane=False):
    """A frame whose header sum (which & 1) and L4 sum (which & 2) are multiples
    of 65535 under `flags`; under CGCK_RAW the whole region's sum."""
    f = header4(rng, ip_len, hl, proto, sane)
    if flags & cgck.RAW:
        retune(f, 4, one(port, f, cgck.RAW)[0])
        return f
    cf = craft_flags(flags)
    if which & 1:
        retune(f, 4, one(port, f, cf)[0])
    if which & 2:
        retune(f, hl * 4 + 20, one(port, f, cf)[1])
    return f


def verdict4(flags, proto, ip_sum, l4_sum, ip_field, l4_field):
    """The verdict the rules of include/cgck.h give a frame with a fitting header
    whose sums (fields read as zero) are ip_sum / l4_sum and whose planted fields
    are ip_field / l4_field.  Restated here, not taken from the oracle's verdict."""
    want = 0xFFFF if flags & cgck.V_IP_ZERO_IS_FFFF and ip_field == 0 else ip_field
    v = cgck.BAD_IP if ip_sum != want else 0
    skipped = flags & cgck.V_UDP_ZERO_SKIP and proto == 17 and l4_field == 0
    if field_off(proto, flags) >= 0 and not skipped and l4_sum != l4_field:
        v |= cgck.BAD_L4
    return v


VERIFY_SETS = (cgck.VERIFY_BSD, cgck.VERIFY_TOY)


def stored_frames(port, rng, ip_len, flags, sane=False):
    """Frames whose checksum fields are planted.  Each carries `want`: the
    intended verdict under VERIFY_BSD and VERIFY_TOY (the pseudo-header choice
    of `flags` added), from the rules, for test_edgecases_cpu.py to hold against
    the oracle."""
    nops = flags & cgck.L4_NOPSEUDO
    cf = craft_flags(flags)
    frames = []

    def add(label, f, proto, lo, hi, ipf, l4f, **kw):
        want = {vs | nops: verdict4(vs | nops, proto, lo, hi, ipf, l4f) for vs in VERIFY_SETS}
        frames.append(Frame(f"stored:{label}", f, want=want, **kw))

    for proto in ZERO_PROTOS:
        if ip_len < 42:
            break
        fo = field_off(proto, flags)
        for label, dip, dl4 in (("ok", 0, 0), ("l4_off", 0, 1), ("ip_off", 1, 0)):
            f = header4(rng, ip_len, 5, proto, sane)
            lo, hi = one(port, f, cf)
            ipf = off_by_one(lo) if dip else lo
            l4f = off_by_one(hi) if dl4 else hi
            put16(f, 10, ipf)
            if fo >= 0:
                put16(f, 20 + fo, l4f)
            add(f"{label}/p{proto}", f, proto, lo, hi, ipf, l4f)
        if proto == 17 and fo >= 0:
            f = header4(rng, ip_len, 5, proto, sane)
            lo, hi = one(port, f, cf)
            put16(f, 10, lo)
            put16(f, 20 + fo, 0)
            add("udp0/p17", f, proto, lo, hi, lo, 0)
        # where both sums are 0xFFFF: a stored 0xFFFF is right, a stored 0 only by
        # CGCK_V_IP_ZERO_IS_FFFF (IP) or where CGCK_V_UDP_ZERO_SKIP skips it (UDP)
        for ipf, l4f in ((0xFFFF, 0xFFFF), (0, 0), (0, 0xFFFF), (0xFFFF, 0)):
            f = zero_frame(port, rng, ip_len, 5, proto, flags, 3, sane)
            put16(f, 10, ipf)
            if fo >= 0:
                put16(f, 20 + fo, l4f)
            add(f"zero_both/{ipf:04x}.{l4f:04x}/p{proto}", f, proto, 0xFFFF, 0xFFFF, ipf, l4f,
                lo_ffff=True, hi_ffff=True)
    return frames


def frames4(port, rng, ip_len, flags, sane=False):
    """The IPv4 class list of one length and flag set."""
    assert ip_len >= 20
    raw = bool(flags & cgck.RAW)
    frames = [Frame(f"hl_sweep:hl{hl}/p{p}", header4(rng, ip_len, hl, p, sane), hl=hl) for hl in range(16) for p in PROTOS]
    frames.append(Frame("fill:00", np.zeros(ip_len, np.uint8), lo_ffff=True))
    frames.append(Frame("fill:ff", np.full(ip_len, 0xFF, np.uint8)))
    f = np.full(ip_len, 0xFF, np.uint8)
    f[0], f[9] = 0x45, 6
    frames.append(Frame("fill:hdr_ff", f))
    for which, cls in ((1, "zero_ip"), (2, "zero_l4"), (3, "zero_both")):
        for p in ZERO_PROTOS:
            for hl in ZERO_HLS:
                if ip_len < (hl * 4 + 22 if which & 2 else max(hl * 4, 20)):
                    continue
                frames.append(Frame(f"{cls}:hl{hl}/p{p}", zero_frame(port, rng, ip_len, hl, p, flags, which, sane),
                                    lo_ffff=raw or bool(which & 1), hi_ffff=not raw and bool(which & 2)))
    if reads_fields(flags) and not raw:
        frames += stored_frames(port, rng, ip_len, flags, sane)
    return frames


def counts4(ip_len, flags):
    """The class counts frames4 yields, by construction."""
    c = {"hl_sweep": 64, "fill": 3}
    c["zero_ip"] = 3 * sum(ip_len >= max(hl * 4, 20) for hl in ZERO_HLS)
    c["zero_l4"] = c["zero_both"] = 3 * sum(ip_len >= hl * 4 + 22 for hl in ZERO_HLS)
    if reads_fields(flags) and not flags & cgck.RAW and ip_len >= 42:
        c["stored"] = 3 * (3 + 4) + (1 if field_off(17, flags) >= 0 else 0)
    return c


# --------------------------------------------------------------------------- IPv6

def header6(rng, ip_len, nh, hbh=False):
    return ip6ref.packet(rng, ip_len, nh, ((0, 8),) if hbh else ())


def hi6(port, f, flags):
    return ip6ref.l4_cksum(port, f, len(f), reads_fields(flags))[4]


def frames6(port, rng, ip_len, flags):
    """The IPv6 class list of one length (>= 62) and flag set."""
    assert ip_len >= 62
    frames = [Frame("fill:00", np.zeros(ip_len, np.uint8)), Frame("fill:ff", np.full(ip_len, 0xFF, np.uint8))]
    f = header6(rng, ip_len, 6)
    f[40:] = 0xFF
    frames.append(Frame("fill:hdr_ff", f))
    if flags & cgck.RAW:
        f = header6(rng, ip_len, 6)
        retune(f, 4, port.in_cksum(f, 0, ip_len))
        return frames + [Frame("zero_l4:raw", f, lo_ffff=True)]
    zeros = []
    for nh in NH6:
        f = header6(rng, ip_len, nh)
        retune(f, 60, hi6(port, f, flags))
        zeros.append((nh, 40, f))
    if ip_len >= 70:
        f = header6(rng, ip_len, 6, hbh=True)
        retune(f, 68, hi6(port, f, flags))
        zeros.append((6, 48, f))
    frames += [Frame(f"zero_l4:nh{nh}@{l4}", f, hi_ffff=True) for nh, l4, f in zeros]
    if reads_fields(flags):
        skip = bool(flags & cgck.V_UDP_ZERO_SKIP)
        for nh in (6, 17, 58):
            fo = 40 + ip6ref.FIELD[nh]
            f = header6(rng, ip_len, nh)
            hi = hi6(port, f, flags)
            g = f.copy()
            put16(f, fo, hi)
            put16(g, fo, off_by_one(hi))
            frames.append(Frame(f"stored:ok/nh{nh}", f, want=0))
            frames.append(Frame(f"stored:off/nh{nh}", g, want=cgck.BAD_L4))
            for v in (0, 0xFFFF):
                f = header6(rng, ip_len, nh)
                retune(f, 60, hi6(port, f, flags))
                put16(f, fo, v)
                bad = v == 0 and not (skip and nh == 17)
                frames.append(Frame(f"stored:zero_l4/{v:04x}/nh{nh}", f, hi_ffff=True, want=cgck.BAD_L4 if bad else 0))
    return frames


def counts6(ip_len, flags):
    if flags & cgck.RAW:
        return {"fill": 3, "zero_l4": 1}
    c = {"fill": 3, "zero_l4": 5 + (ip_len >= 70)}
    if reads_fields(flags):
        c["stored"] = 12
    return c


# --------------------------------------------------------------------------- layouts

def pad_frame(rng, ip_len, ip6):
    return Frame("pad:", header6(rng, ip_len, 6) if ip6 else header4(rng, ip_len, 5, 6))


def order(rng, lists, ip6=False):
    """The frames of a batch, in order, from one class list per length.

    The lists are interleaved frame by frame (a mixed batch mixes its lengths
    inside every 64-frame step).  The result is repeated with a rotation: four
    copies rotated by 0..3 where that stays within MAX_FRAMES, else the hl_sweep
    frames once (64 per length: every lane) and the other classes twice, rotated
    by 0 and 1.  Each rotated part is padded to a multiple of 4 frames, so copy c
    moves a frame to the next lower index mod 4 and to another lane.  Pad frames
    then fill the batch up to a multiple of 64, and one frame of every class
    follows: the last, partial 64-frame chunk."""
    mixed = []
    for i in range(max(len(x) for x in lists)):
        mixed += [x[i] for x in lists if i < len(x)]
    lens = [len(x[0].data) for x in lists]

    def padded(fr):
        return fr + [pad_frame(rng, lens[k % len(lens)], ip6) for k in range(-len(fr) % 4)]

    def rotations(fr, copies):
        fr = padded(fr)
        return [fr[(j + c) % len(fr)] for c in range(copies) for j in range(len(fr))]

    if 4 * (len(mixed) + 3) + 64 + 16 <= MAX_FRAMES:
        seq = rotations(mixed, 4)
    else:
        seq = padded([f for f in mixed if f.cls == "hl_sweep"]) + rotations([f for f in mixed if f.cls != "hl_sweep"], 2)
    seq += [pad_frame(rng, lens[k % len(lens)], ip6) for k in range(-len(seq) % 64)]
    seen = {}
    for f in mixed:
        seen.setdefault(f.cls, f)
    seq += list(seen.values())
    assert len(seq) <= MAX_FRAMES, len(seq)
    return seq


@dataclass
class Batch:
    buf: np.ndarray
    frames: list
    desc: object = None      # DESC_DTYPE array, or None for a strided batch
    stride: int = 0
    l3_off: int = 0
    ip_len: int = 0
    starts: np.ndarray = field(default=None, repr=False)

    @property
    def n(self):
        return len(self.frames)

    @property
    def lens(self):
        return np.asarray([len(f.data) for f in self.frames], np.int64)

    def labels(self, idx):
        return [f"{int(i)}:{self.frames[int(i)].label}({len(self.frames[int(i)].data)})" for i in idx]

    def at_byte(self, pos):
        """Indices of the frames that hold the buffer positions `pos`."""
        k = np.searchsorted(self.starts, np.asarray(pos), side="right") - 1
        return np.unique(np.clip(k, 0, self.n - 1))


def _place(rng, seq, starts, nbytes):
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    for s, f in zip(starts, seq):
        buf[s:s + len(f.data)] = f.data
    return buf


def strided(rng, seq, stride, l3_off):
    ip_len = len(seq[0].data)
    assert all(len(f.data) == ip_len for f in seq) and ip_len <= stride
    starts = np.arange(len(seq), dtype=np.int64) * stride + l3_off
    buf = _place(rng, seq, starts, len(seq) * stride + l3_off + ip_len + 64)
    return Batch(buf, seq, None, stride, l3_off, ip_len, starts)


def _desc(starts, l3, lens):
    d = np.zeros(len(starts), cgck.DESC_DTYPE)
    d["frame_off"] = starts - l3
    d["l3_off"] = l3
    d["ip_len"] = lens
    return d


def packed(rng, seq, first_off=0):
    """Back to back in descriptor order, as batches.packed_batch lays frames out."""
    lens = np.asarray([len(f.data) for f in seq], np.int64)
    starts = first_off + np.concatenate(([0], np.cumsum(lens)[:-1]))
    l3 = np.minimum(rng.integers(0, 20, len(seq)), starts)
    return Batch(_place(rng, seq, starts, int(starts[-1] + lens[-1]) + 256), seq, _desc(starts, l3, lens), starts=starts)


def ring(rng, seq, slot=SLOT, l3_off=SLOT_L3):
    """Frame k at slot * k + l3_off (fillbatches.ring's layout)."""
    lens = np.asarray([len(f.data) for f in seq], np.int64)
    assert int(lens.max()) + l3_off <= slot
    starts = np.arange(len(seq), dtype=np.int64) * slot + l3_off
    return Batch(_place(rng, seq, starts, len(seq) * slot + 64), seq, _desc(starts, np.full(len(seq), l3_off), lens),
                 starts=starts)


def scattered(rng, seq):
    """Odd offsets: every frame starts at an odd address, gaps of 1..39 bytes."""
    lens = np.asarray([len(f.data) for f in seq], np.int64)
    starts = np.zeros(len(seq), np.int64)
    at = 33
    for i, ln in enumerate(lens):
        starts[i] = at
        at += int(ln) + int(rng.integers(1, 40))
        at |= 1
    return Batch(_place(rng, seq, starts, at + 128), seq, _desc(starts, rng.integers(0, 20, len(seq)), lens), starts=starts)


def corpus(port, seed, lens, flags, layout, **kw):
    """The batch of one cell: lens is one length (strided) or the lengths mixed."""
    rng = np.random.default_rng(seed)
    ip6 = bool(flags & cgck.IP6)
    build = frames6 if ip6 else frames4
    lens = [lens] if np.isscalar(lens) else list(lens)
    seq = order(rng, [build(port, rng, ln, flags & ~cgck.IP6) for ln in lens], ip6)
    return {"strided": strided, "packed": packed, "ring": ring, "scattered": scattered}[layout](rng, seq, **kw)


PLAIN64_N = 192 + 7


def plain64(port, seed, flags):
    """199 frames of 64 bytes at stride 64, every one with ip_hl 5, so every wave
    takes the 64 B fast path of lpa and lpd.  The zero_* frames of ip_hl 5, the
    0xFF-payload frame and (where the flags read fields) the stored frames, with
    pad frames up to an odd count m of at least 21, repeat with period m: a frame
    moves by m lanes, and to the next index mod 4 or the one before, each time."""
    rng = np.random.default_rng(seed)
    special = [f for f in frames4(port, rng, 64, flags)
               if f.label == "fill:hdr_ff" or (f.cls.startswith("zero_") and ":hl5/" in f.label) or f.cls == "stored"]
    special += [pad_frame(rng, 64, False) for _ in range(max(21 - len(special), 1 - len(special) % 2))]
    assert len(special) % 2 == 1 and 6 * len(special) <= PLAIN64_N
    return strided(rng, [special[i % len(special)] for i in range(PLAIN64_N)], 64, 0)


def expect(port, b, flags):
    """(out, verdict, the buffer after the call) from the oracle on the finished
    buffer; under CGCK_STORE the oracle's buffer is the expectation."""
    after = b.buf.copy()
    if flags & cgck.IP6 and not flags & cgck.RAW:
        return ip6ref.expect(port, b.buf, b.starts, b.lens, flags)
    fl = flags & ~cgck.IP6
    if b.desc is None:
        out, ver = port.batch_strided(after, b.n, b.stride, b.l3_off, b.ip_len, fl)
    else:
        out, ver = port.batch_desc(after, b.desc.view(np.uint8), b.n, fl)
    return out, ver, after


def disjoint(b):
    """No two frames of the batch share a byte (a CGCK_STORE batch must not)."""
    s, ln = b.starts, b.lens
    o = np.argsort(s, kind="stable")
    return bool(np.all(s[o][1:] >= s[o][:-1] + ln[o][:-1]))


# --------------------------------------------------------------------------- the cells

G, GZ = cgck.GEN_BOTH, cgck.GEN_BOTH | cgck.ZERO_FIELDS
NOPS = cgck.L4 | cgck.L4_NOPSEUDO
NOPS_VERIFY = cgck.IP | cgck.L4 | cgck.L4_NOPSEUDO | cgck.VERIFY
BASE = [G, cgck.RAW, cgck.IP, cgck.L4, NOPS, GZ]
FLAG_SETS = [cgck.RAW, cgck.IP, cgck.L4, G, NOPS, GZ, cgck.FILL_BOTH, cgck.IP | cgck.ZERO_FIELDS | cgck.STORE,
             cgck.VERIFY_BSD, cgck.VERIFY_TOY, NOPS_VERIFY, cgck.VERIFY_BSD | cgck.STORE]   # test_gpu_parity's
MIX4 = (41, 64, 99, 576, 1500)
MIX4_20 = MIX4 + (20,)
MIX6 = (62, 64, 99, 576, 1500)
GEN6 = [G | cgck.IP6, cgck.L4 | cgck.IP6, cgck.RAW | cgck.IP6]
VER6 = [G | cgck.IP6, cgck.VERIFY_TOY | cgck.IP6, cgck.VERIFY_TOY | cgck.V_UDP_ZERO_SKIP | cgck.IP6]


def S(stride, l3, ln):
    return ("strided", ln, (("stride", stride), ("l3_off", l3)))


PLAIN = ("plain64", 64, ())
BOTH = [("packed", MIX4, ()), ("ring", MIX4, ())]
BOTH6 = [("packed", MIX6, ()), ("ring", MIX6, ())]
# family -> (the shapes (layout, lengths, layout arguments), the flag sets): the
# table of test_gpu_edgecases.py; test_edgecases_cpu.py validates every batch
CELLS = {
    "lpd": ([S(64, 0, 64), S(64, 0, 48), PLAIN], BASE),
    "lpa": ([S(64, 0, 64), S(64, 0, 48), S(64, 0, 20), S(128, 16, 64), PLAIN],
            BASE + [cgck.FILL_BOTH, cgck.VERIFY_BSD, cgck.VERIFY_TOY, NOPS_VERIFY]),
    "dstr": ([S(1500, 0, 1500), S(1504, 4, 1501), S(64, 0, 64), S(60, 8, 60), S(24, 0, 20)],
             [G, cgck.RAW, cgck.IP, cgck.L4, NOPS]),
    "lpw": (BOTH, [G, GZ, cgck.VERIFY_BSD, cgck.VERIFY_TOY, NOPS]),
    "lpf": (BOTH, [cgck.FILL_BOTH, cgck.IP | cgck.ZERO_FIELDS | cgck.STORE, cgck.VERIFY_BSD | cgck.STORE]),
    "lpf_bad": (BOTH, [cgck.VERIFY_BSD, cgck.VERIFY_TOY]),
    "slot2": ([("scattered", MIX4_20, ())], FLAG_SETS),
    "lpp": ([("scattered", MIX4_20, ())], FLAG_SETS),
    "group": ([("scattered", MIX4_20, ())], FLAG_SETS),
    "lpd6": ([S(64, 0, 64)], GEN6),
    "lpa6": ([S(64, 0, 64), S(64, 0, 62)], GEN6),
    "dstr6": ([S(1500, 0, 1500), S(64, 0, 64)], GEN6),
    "lpw6": (BOTH6, VER6),
    "group6": ([("scattered", MIX6, ())], VER6 + [cgck.FILL_BOTH | cgck.IP6]),
}


# ------------------------------------------------------------------ the burst server's cells
# A server family (test_gpu_server_edgecases.py, test_server_routes_cpu.py) is
# a way into the resident burst server and the body that serves it there.  Its
# shapes carry, beside the layout's own arguments, the request plan: the batch
# goes in consecutive requests of at most `k` frames (requests()) to a server
# opened for `max_pkts` frames, and every request must take the route `route`
# (cgck_test_burst_route; "wide*": any number of workgroups).  "{sys}" /
# "{ldsp}" in a route stand for fl or rt: the body compiled for the flag set,
# or the run-time one (COMPILED; the LDS-resident body is compiled for CGCK_RAW
# too).
SMALL = (20, 41, 64, 80)       # G = 4 bodies: ip_hl 15 with a TCP field at +76 fits 80 bytes
MID = (41, 64, 99, 576)
OVER80 = (99, 256, 576)        # every request's max_len above 80, twelve frames within 8 KiB
BIG = (577, 1500)               # sixteen frames above 8 KiB of block whichever they are
LONG = (1600, 4000)            # past the S * G = 1536 unrolled bytes: the long-packet loop
PLAN_KEYS = ("plan_k", "plan_max_pkts", "plan_route")   # (no layout argument is named so)
SERVER_BYTES = 4 << 20         # cgck_burst_open's max_bytes in every cell
COMPILED = (cgck.VERIFY_BSD, cgck.FILL_BOTH, GZ)
RUNTIME = (G, cgck.VERIFY_TOY, NOPS, NOPS_VERIFY, cgck.RAW, cgck.VERIFY_BSD | cgck.STORE)
NO_STORE = [f for f in COMPILED + RUNTIME if not f & cgck.STORE]   # a pageable CGCK_STORE batch is launched
IN_PLACE = list(COMPILED + RUNTIME)
PAGEABLE, REGISTERED, REQUEST = cgck.ROUTE_PAGEABLE, cgck.ROUTE_REGISTERED, cgck.ROUTE_REQUEST


def P(layout, lens, k, route, max_pkts=4096):
    return (layout, lens, (("plan_k", k), ("plan_max_pkts", max_pkts), ("plan_route", route)))


# family -> how it is reached (cgck_desc_host on pageable or registered memory,
# cgck_burst_request over a registered mapping's device view)
SERVER = {
    "srv_ldsp4": PAGEABLE, "srv_ldsp16": PAGEABLE, "srv_scratch": PAGEABLE, "srv_sys4": REQUEST,
    "srv_sys16": REQUEST, "srv_inplace": REQUEST, "srv_wide_staged": PAGEABLE, "srv_wide_inplace": REQUEST,
    "srv_store_host": REGISTERED,
}
CELLS.update({
    "srv_ldsp4": ([P("packed", SMALL, 64, "one/lds/ldsp/g4u1/{ldsp}")], NO_STORE),
    "srv_ldsp16": ([P("packed", OVER80, 12, "one/lds/ldsp/g16u1/{ldsp}")], NO_STORE),
    "srv_scratch": ([P("packed", BIG, 16, "one/scratch/staged/g16u1/rt"),
                     P("scattered", MIX4, 48, "one/scratch/staged/g16u4/rt")], NO_STORE),
    "srv_sys4": ([P("packed", SMALL, 64, "one/lds/sys/g4u1/{sys}"),
                  P("scattered", SMALL, 64, "one/lds/sys/g4u1/{sys}")], IN_PLACE),
    "srv_sys16": ([P("packed", MIX4_20, 16, "one/lds/sys/g16u1/{sys}"),
                   P("scattered", MIX4_20, 16, "one/lds/sys/g16u1/{sys}")], IN_PLACE),
    "srv_inplace": ([P("packed", MIX4_20, 48, "one/lds/inplace/g16u4/rt"),
                     P("scattered", MIX4_20, 48, "one/lds/inplace/g16u4/rt"),
                     P("packed", LONG, 16, "one/lds/inplace/g16u1/rt"),
                     P("scattered", LONG, 16, "one/lds/inplace/g16u1/rt")], IN_PLACE),
    "srv_wide_staged": ([P("packed", SMALL, 128, "wide*/slice/staged/g4u1/rt", 128),
                         P("packed", MID, 128, "wide*/slice/staged/g16u4/rt", 128),
                         P("scattered", SMALL, MAX_FRAMES, "wide*/slice/staged/g4u1/rt"),
                         P("scattered", MID, MAX_FRAMES, "wide*/slice/staged/g16u4/rt")], NO_STORE),
    "srv_wide_inplace": ([P("scattered", SMALL, 128, "wide*/slice/inplace/g4u1/rt", 128),
                          P("scattered", MID, 128, "wide*/slice/inplace/g16u4/rt", 128),
                          P("packed", SMALL, MAX_FRAMES, "wide*/slice/inplace/g4u1/rt"),
                          P("packed", MID, MAX_FRAMES, "wide*/slice/inplace/g16u4/rt")], IN_PLACE),
    "srv_store_host": ([P("scattered", SMALL, 64, "one/lds/sys/g4u1/{sys}"),
                        P("packed", MIX4_20, 16, "one/lds/sys/g16u1/{sys}"),
                        P("scattered", MIX4_20, 48, "one/lds/inplace/g16u4/rt")],
                       [f for f in FLAG_SETS if f & cgck.STORE]),
})


def requests(batch, k):
    """The request plan: consecutive windows (lo, hi) of the batch, as few as hold
    at most k frames each and of sizes that differ by at most one, so the last
    request is no smaller than the others and takes their route."""
    m = -(-batch.n // k)
    return [(batch.n * i // m, batch.n * (i + 1) // m) for i in range(m)]


def plan(cell):
    """(k, max_pkts, route) of a server cell, the route with fl / rt filled in."""
    (_, _, kw), flags = cell
    kw = dict(kw)
    fl = {"sys": "fl" if flags in COMPILED else "rt", "ldsp": "fl" if flags in COMPILED + (cgck.RAW,) else "rt"}
    return kw["plan_k"], kw["plan_max_pkts"], kw["plan_route"].format(**fl)


def route_of(b, lo, hi, flags, mem, max_pkts, max_bytes=SERVER_BYTES):
    """The route the library names for frames [lo, hi) of the batch as one request."""
    return cgck.burst_route(max_pkts, max_bytes, mem, b.lens[lo:hi], flags)


def route_kinds(name):
    """The kinds of body a route name stands for (cgck.burst_route_kinds lists them
    all): W and the pass count left out, one U a kind."""
    p = name.split("/")
    if len(p) < 5:
        return set()
    p[0] = "wide" if p[0].startswith("wide") else p[0]
    g, us = p[3].split("u", 1)
    kinds = {"/".join(p[:3] + [f"{g}u{u.lstrip('u')}", p[4]]) for u in us.split("+")}
    if len(p) > 5:
        kinds.add("/".join(p[:3] + ["passes"]))
    return kinds


# The second slice pass (test_server_slice_passes): one request of PASS_N frames
# to a server opened for as many.  32 workgroups take 1026 or 1027 frames each:
# a full pass of 1024 descriptors, then a pass of 2 or 3.
PASS_N = 32 * 1024 + 71
PASS_BYTES = 8 << 20           # max_bytes: the mid mix staged is 32839 frames of ~200 padded bytes, 6.4 MB
PASS_CLASSES = ("zero_ip", "zero_l4", "zero_both", "stored", "hl_sweep", "fill")
PASS_CELLS = {   # mix -> the corpus cell per flag set
    "small": (("scattered", SMALL, ()), [G, cgck.VERIFY_BSD, cgck.VERIFY_TOY, cgck.FILL_BOTH]),
    "mid": (("scattered", MID, ()), [G, cgck.VERIFY_BSD, cgck.VERIFY_TOY]),
}


def second_pass(route, n=PASS_N, per_pass=1024):
    """The request indices that fall in a second pass of their slice, W taken from
    the route's name ("wide32/...")."""
    W = int(route.split("/")[0][4:])
    return [k for j in range(W) for k in range(n * j // W + per_pass, n * (j + 1) // W)]


def pass_batch(b, route, tiled):
    """PASS_N frames from the batch b: request k is frame (k + rot) % b.n, with
    the smallest rotation that puts every class b holds of PASS_CLASSES into a
    second pass.  tiled: copy k // b.n of the buffer holds it, so no two share a
    byte (CGCK_STORE); else the descriptors overlap in the one buffer."""
    want = {f.cls for f in b.frames} & set(PASS_CLASSES)
    late = second_pass(route)
    rot = next(r for r in range(b.n) if {b.frames[(k + r) % b.n].cls for k in late} >= want)
    idx = (np.arange(PASS_N) + rot) % b.n
    tile = (np.arange(PASS_N) // b.n) * len(b.buf) if tiled else 0
    starts = b.starts[idx] + tile
    buf = np.tile(b.buf, -(-PASS_N // b.n)) if tiled else b.buf.copy()
    return Batch(buf, [b.frames[i] for i in idx], _desc(starts, b.desc["l3_off"][idx].astype(np.int64), b.lens[idx]),
                 starts=starts)


# The RX window's frames (test_rx_window_edge_classes): those of frames4, under
# headers a stack reads on (header4's sane), whose header a stack takes: the
# zero-sum, planted-field and 0xFF-payload frames and the ip_hl sweep from 5 up
# to the frame's length, in bursts for the system-coherent G = 16 and G = 4
# bodies and for slices.
RX_LENS = (64, 99, 1500)
RX_L2 = (14, 16, 21)           # q even, zero and odd: the header bytes in chunk 0, chunk 1, across both


def rx_frames(port, ln):
    rng = np.random.default_rng(0x5A00 + ln)
    return [f for f in frames4(port, rng, ln, cgck.VERIFY_BSD, sane=True)
            if f.cls.startswith("zero_") or f.cls == "stored" or f.label == "fill:hdr_ff"
            or (f.cls == "hl_sweep" and 20 <= f.hl * 4 <= ln)]


def rx_bursts(port):
    """[(name, frames)]: bursts of 16 of every length mixed, of 64 frames of 64
    bytes, and one of 300."""
    per = [rx_frames(port, ln) for ln in RX_LENS]
    mixed = [f for i in range(max(map(len, per))) for x in per for f in x[i:i + 1]]
    small = per[0]
    return ([(f"16@{i}", mixed[i:i + 16]) for i in range(0, len(mixed) - 15, 16)]
            + [(f"64@{i}", small[i:i + 64]) for i in range(0, len(small) - 63, 64)] + [("300", mixed[:300])])


def cells(family):
    return [(shape, flags) for shape in CELLS[family][0] for flags in CELLS[family][1]]


def launched_mixes():
    """(layout, mix) of the launched families' cells."""
    return {(layout, lens) for fam, (shapes, _) in CELLS.items() if fam not in SERVER
            for layout, lens, _ in shapes if not np.isscalar(lens)}


def cell_id(cell):
    (layout, lens, kw), flags = cell
    # (the launched families' mixes keep the plain "mix"; a server family's mix
    # is named by its count and longest frame, so no two batches share an id)
    ln = lens if np.isscalar(lens) else "mix" if (layout, lens) in launched_mixes() else f"mix{len(lens)}x{max(lens)}"
    if dict(kw).get("plan_route"):   # a server cell: its plan, as k<frames a request>-m<max_pkts>
        kw = [(k, f"{k[5]}{v}") for k, v in kw if k != "plan_route"]
    return f"{layout}-{ln}-{'-'.join(str(v) for _, v in kw)}-{flags:#x}".replace("--", "-")


def corpus_cell(cell):
    """The cell without its request plan: server cells that differ only in the
    plan share one batch."""
    (layout, lens, kw), flags = cell
    return (layout, lens, tuple(x for x in kw if x[0] not in PLAN_KEYS)), flags


_cache = {}


def cell_batch(port, cell):
    """The batch of a cell (built once a session; callers copy what they change)."""
    (layout, lens, kw), flags = corpus_cell(cell)
    key = (layout, lens, kw, flags)
    if key not in _cache:
        seed = 0xED6E + sum(ord(c) for c in layout) * 7 + int(np.sum(lens)) * 131 + flags
        _cache[key] = plain64(port, seed, flags) if layout == "plain64" else corpus(port, seed, lens, flags, layout, **dict(kw))
    return _cache[key]
