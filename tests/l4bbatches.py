"""Inputs for the cgck_l4_build tests: a corpus of (class byte, flow index, segment
record, cap) items that reaches every class and flag of the contract under both
families, tagged and untagged, and the layouts that put its slots into a buffer.
Expectations come from tests/l4bref.py; nothing here calls the library."""
import numpy as np

import l4bref as R

POISON = 0xA5
SYN, ACK, FIN, RST, PSH = 0x02, 0x10, 0x01, 0x04, 0x08
# flow[]: two refused records in front, then the four shapes; nflow - 1 is a good one
NFLOW = 6
BAD_A, BAD_B, V4, V6, V4T, V6T = range(NFLOW)
GOOD = (V4, V6, V4T, V6T)


def flows(rng):
    f = np.zeros(NFLOW, R.FLOW_DTYPE)
    f.view(np.uint8)[:] = rng.integers(0, 256, f.nbytes, dtype=np.uint8)       # every byte random, the ignored ones too
    f["flags"] = [0x04, 0x83, 0, R.FLOW_IP6, R.FLOW_VLAN, R.FLOW_IP6 | R.FLOW_VLAN]
    return f


def seg(rng, **kw):
    """A record whose every byte is random (l4_off and hdr_len are ignored by the
    call) with a legal opt, then the fields given."""
    s = np.zeros(1, R.SEG_DTYPE)
    s.view(np.uint8)[:] = rng.integers(0, 256, s.nbytes, dtype=np.uint8)
    s["opt"] = 0
    s["pay_len"] = 0
    s["wscale"] = int(s["wscale"][0]) % 15
    for k, v in kw.items():
        s[k] = v
    return s[0]


class Corpus:
    """cls u8[m], fidx u32[m], seg SEG_DTYPE[m], flow FLOW_DTYPE[NFLOW], and per item
    capd: None for a roomy slot, an int d for cap = L + d, ("abs", v) for cap = v."""

    def __init__(self, rng):
        self.flow = flows(rng)
        it = []                                         # (cls byte, fidx, seg, capd)
        for f in GOOD:
            for opt in range(8):                        # each option subset, without payload
                it.append((R.SEG_TCP, f, seg(rng, opt=opt, th_flags=SYN if opt & 3 else ACK), None))
            it.append((R.SEG_TCP, f, seg(rng, opt=R.TS, pay_len=1, th_flags=ACK | PSH), None))
            it.append((R.SEG_TCP, f, seg(rng, opt=0, pay_len=1400, th_flags=ACK), None))
            for pay in (0, 1, 1400):
                it.append((R.SEG_UDP, f, seg(rng, pay_len=pay, opt=0xFF), None))       # opt is TCP's: ignored
            for capd in (-1, 0, 1):                     # cap at L - 1, L, L + 1
                it.append((R.SEG_TCP, f, seg(rng, opt=7, th_flags=SYN), capd))
                it.append((R.SEG_UDP, f, seg(rng), capd))
                it.append((R.SEG_TCP, f, seg(rng, opt=R.WS, pay_len=33, th_flags=SYN | ACK), capd))
            it.append((R.SEG_TCP, f, seg(rng, opt=R.OPT_BAD), None))                   # BADSEG
            it.append((R.SEG_TCP, f, seg(rng, opt=R.OPT_BAD | 7), 0))
            it.append((R.SEG_TCP, f, seg(rng, opt=0x08), None))
            it.append((R.SEG_TCP, f, seg(rng, opt=R.WS, wscale=15, th_flags=SYN), None))
            it.append((R.SEG_TCP, f, seg(rng, opt=R.WS, wscale=14, th_flags=SYN), None))   # built
            it.append((R.SEG_TCP, f, seg(rng, opt=R.MSS, wscale=15, th_flags=SYN), None))  # built: no WS, wscale ignored
            it.append((R.SEG_UDP, f, seg(rng, pay_len=65528), None))                   # BADSEG
            it.append((R.SEG_UDP, f, seg(rng, pay_len=65527), ("abs", 65535)))                  # NOROOM: no cap holds it
            it.append((R.SEG_TCP, f, seg(rng, pay_len=65535), ("abs", 65535)))                  # NOROOM
            it.append((R.SEG_TCP, f, seg(rng), ("abs", 0)))                            # NOROOM: cap 0
            it.append((R.SEG_TCP | 0x30, f, seg(rng, opt=R.TS), None))                 # the low nibble counts
            it.append((R.SEG_UDP | 0xC0, f, seg(rng), None))
            for c in (2, 5, 10, 15, 0x12):              # SKIP, whatever else is wrong
                it.append((c, f if c != 5 else NFLOW, seg(rng, opt=R.OPT_BAD if c == 10 else 0), None))
        for f, s in ((BAD_A, seg(rng)), (BAD_B, seg(rng, opt=R.OPT_BAD)), (NFLOW, seg(rng)), (0xFFFFFFFF, seg(rng)),
                     (NFLOW, seg(rng, opt=R.OPT_BAD))):
            it.append((R.SEG_TCP, f, s, None))          # BADFLOW, before BADSEG
            it.append((R.SEG_UDP, f, s, 0))
        it.append((R.SEG_TCP, NFLOW - 1, seg(rng, opt=7, th_flags=SYN, mss=1460, wscale=7), 0))      # 18 + 40 + 40 bytes
        self.cls = np.array([x[0] for x in it], np.uint8)
        self.fidx = np.array([x[1] for x in it], np.uint32)
        self.seg = np.array([x[2] for x in it], R.SEG_DTYPE)
        self.capd = [x[3] for x in it]
        self.m = len(it)

    def L(self, i):
        """(header bytes, L) of item i were it built; (0, 0) where rules 1 to 3 refuse it."""
        f = int(self.fidx[i])
        if f >= NFLOW:
            return 0, 0
        hb = R.hdr_bytes(int(self.flow["flags"][f]), int(self.cls[i]), int(self.seg["opt"][i]))
        return hb, hb + int(self.seg["pay_len"][i]) if hb else 0

    def cap(self, i):
        hb, L = self.L(i)
        d = self.capd[i]
        if d is None:
            return min(L + 5, 65535) if L else 40
        return d[1] if isinstance(d, tuple) else max(L + d, 0)


def lay(C, align, l3s=(0, 14, 3, 64)):
    """Every item once, each frame start at `align` mod 16, POISON between the slots
    and random bytes (payload that must survive) inside them: (buf, slot).  A slot
    whose frame is built has cap bytes behind its frame start (the last one ends the
    buffer), any other 128 whatever cap it claims."""
    rng = np.random.default_rng(1000 + align)
    slot = np.zeros(C.m, R.DESC_DTYPE)
    parts, at = [], 0
    for i in range(C.m):
        l3 = l3s[i % len(l3s)]
        cap = C.cap(i)
        L = C.L(i)[1]
        room = cap if i == C.m - 1 else max(cap, 128) if 0 < L <= cap else 128
        pad = (align - (at + l3 + 1)) % 16 + 1          # at least one poison byte in front
        parts.append(np.full(pad + l3, POISON, np.uint8))
        slot[i] = (at + pad, l3, cap)
        parts.append(rng.integers(0, 256, room, dtype=np.uint8))
        at += pad + l3 + room
    buf = np.concatenate(parts)
    assert np.all(((slot["frame_off"].astype(np.int64) + slot["l3_off"]) & 15) == align)
    return buf, slot


def tiled(C, n, slot_bytes=128):
    """n frames in slot_bytes-byte slots, frame k from item k % m, the Ethernet
    header at offset k % 3 of its slot: (buf of random bytes, slot, cls, fidx, seg)."""
    rng = np.random.default_rng(77)
    k = np.arange(n)
    i = k % C.m
    slot = np.zeros(n, R.DESC_DTYPE)
    slot["frame_off"] = k * slot_bytes
    slot["l3_off"] = k % 3
    cap = np.array([C.cap(j) for j in range(C.m)], np.int64)[i]
    slot["ip_len"] = np.minimum(cap, slot_bytes - (k % 3))
    period = rng.integers(0, 256, 3 * C.m * slot_bytes, dtype=np.uint8)
    buf = np.tile(period, -(-n // (3 * C.m)))[:n * slot_bytes].copy()
    return buf, slot, C.cls[i].copy(), C.fidx[i].copy(), C.seg[i].copy()


def packed(C, start, reps=3):
    """The items that are built without payload, `reps` times over in a shuffled
    order, back to back with cap == L from byte `start` on: neighbours share dwords
    and 16-byte granules.  (buf, slot, cls, fidx, seg); POISON in front and behind."""
    rng = np.random.default_rng(78)
    flags = C.flow["flags"]
    idx = [i for i in range(C.m) if C.L(i)[0] and int(C.seg["pay_len"][i]) == 0 and int(C.fidx[i]) in GOOD
           and R.one(C.seg[i], C.flow[int(C.fidx[i])], int(C.cls[i]), 0, 0, 65535, 0)[1] is not None]
    idx = rng.permutation(np.array(idx * reps))
    L = np.array([C.L(i)[1] for i in idx], np.int64)
    off = start + np.concatenate(([0], np.cumsum(L)[:-1]))
    slot = np.zeros(len(idx), R.DESC_DTYPE)
    slot["frame_off"] = off
    slot["ip_len"] = L
    buf = np.full(start + int(L.sum()) + 13, POISON, np.uint8)
    assert len({int(flags[int(f)]) for f in C.fidx[idx]}) == 4
    return buf, slot, C.cls[idx].copy(), C.fidx[idx].copy(), C.seg[idx].copy()


def with_ids(buf, desc, cls, first):
    """buf (frames built with ip ids 0, 1, ...) as a call with ip_id0 = first builds
    it: the id field and the header sum of every built IPv4 frame, restated over
    whole arrays (the three-pass test compares a burst piece by piece)."""
    k = np.nonzero(((cls & 15) <= R.UDP) & ((cls & R.IP6) == 0))[0]
    o = (desc["frame_off"].astype(np.int64) + desc["l3_off"])[k]
    out = buf.copy()
    ids = (first + k) & 0xFFFF
    out[o + 4], out[o + 5] = ids >> 8, ids & 255
    out[o + 10] = out[o + 11] = 0
    h = out[o[:, None] + np.arange(20)].astype(np.int64)
    s = (h[:, 0::2] | h[:, 1::2] << 8).sum(axis=1) % 65535
    c = np.where(s == 0, 0xFFFF, 0xFFFF - s)
    out[o + 10], out[o + 11] = c & 255, c >> 8
    return out
