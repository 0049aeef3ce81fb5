"""IPv6 batch builders for the lpw6 tests (test_gpu_ipv6_lpw.py,
test_ipv6_imix_cpu.py): frames from ip6ref.packet laid back to back, in ring
slots or at a stride, and the Python restatement of cgck_synth_imix_ip6 /
cgck_synth_imix_ring_ip6 (the oracle's stream bytes and IMIX descriptors plus
the IPv6 stamp).  Nothing here calls the library under test."""
import numpy as np

import ip6ref

LENS = (40, 41, 48, 60, 61, 64, 575, 576, 1279, 1280, 1499, 1500, 1514)
NHS = (6, 17, 58, 59, 253)
IMIX = (64,) * 7 + (576,) * 4 + (1500,)
IMIX_CYCLE = (64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576)      # cgck_synth_imix's 12-frame cycle
DESC_DTYPE =np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")])
H, D, R, A, F = 0, 60, 43, 51, 44

# test_gpu_ipv6.py::test_chains' cases that fit a 2048 B slot, and the two short lengths
SPECIALS = (
    (((A, 24),), 6, 130), (((R, 24),), 58, 99), (((A, 12), (D, 8)), 17, 88),
    (((F, 8),), 6, 100), (((H, 8), (F, 8)), 17, 100),
    (((H, 8),) + ((D, 8),) * 7, 17, 200),       # eight headers
    (((H, 8),) + ((D, 8),) * 8, 17, 200),       # a ninth
    (((H, 8), (D, 16)), 6, 49),                 # the second header's bytes are past ip_len
    (((H, 8), (D, 16)), 6, 60),                 # the L4 region would start past ip_len
    (((H, 8),), 6, 48 + 17),                    # the TCP checksum field does not fit
    ((), 6, 39), ((), 17, 0),
)


def chain_of(i):
    """Every 5th frame carries HBH(8), every 11th HBH(16) + DestOpt(8)."""
    return ((H, 16), (D, 8)) if i % 11 == 10 else ((H, 8),) if i % 5 == 4 else ()


def frames_of(rng, lens, nhs, chains=False, specials=()):
    """One frame per length (nh in turn); with `specials`, SPECIALS[j] replaces
    frame specials[j]."""
    out = []
    for i, ln in enumerate(lens):
        out.append(ip6ref.packet(rng, int(ln), nhs[i % len(nhs)], chain_of(i) if chains else ()))
    for j, at in enumerate(specials):
        chain, nh, ln = SPECIALS[j]
        out[at] = ip6ref.packet(rng, ln, nh, chain)
    return out


def lay(rng, frames, offs, tail=256):
    """The frames at byte offsets offs of a random buffer: (buf, desc with l3_off 0, offs, lens)."""
    offs = np.asarray(offs, np.int64)
    lens = np.array([len(f) for f in frames], np.int64)
    buf = rng.integers(0, 256, int((offs + lens).max()) + tail, dtype=np.uint8)
    for f, o in zip(frames, offs):
        buf[o:o + len(f)] = f
    desc = np.zeros(len(frames), DESC_DTYPE)
    desc["frame_off"] = offs
    desc["ip_len"] = lens
    return buf, desc, offs, lens


def packed(rng, frames, first_off=0):
    """Back to back: frame k + 1 starts where frame k ends."""
    lens = np.array([len(f) for f in frames], np.int64)
    offs = first_off + np.concatenate(([0], np.cumsum(lens)[:-1]))
    return lay(rng, frames, offs)


def slotted(rng, frames, slot=2048, l3=14):
    """Frame k at k * slot + l3, the descriptor's l3_off carrying l3."""
    buf, desc, offs, lens = lay(rng, frames, np.arange(len(frames), dtype=np.int64) * slot + l3)
    desc["frame_off"] = offs - l3
    desc["l3_off"] = l3
    return buf, desc, offs, lens


def stamp6(p, ln, nh):
    """cgck_synth_strided_ip6's stamp on one frame."""
    p[0:4] = (0x60, 0, 0, 0)
    p[4], p[5], p[6] = (ln - 40) >> 8, (ln - 40) & 255, nh
    if nh in ip6ref.FIELD and 40 + ip6ref.FIELD[nh] + 2 <= ln:
        p[40 + ip6ref.FIELD[nh]:40 + ip6ref.FIELD[nh] + 2] = 0


def imix6(port, n, nh, seed, stride=0, l3_off=0):
    """cgck_synth_imix_ip6 (stride 0) / cgck_synth_imix_ring_ip6 restated: the
    oracle's stream bytes, its IMIX offsets and lengths, the IPv6 stamp.
    (buf, desc, offs, lens); buf ends with the last frame (packed) or slot."""
    d = [port.imix_desc(k) for k in range(n)]
    lens = np.array([x[1] for x in d], np.int64)
    fo = np.arange(n, dtype=np.int64) * stride if stride else np.array([x[0] for x in d], np.int64)
    offs = fo + l3_off
    buf = port.stream_bytes(0, n * stride if stride else int(offs[-1] + lens[-1]), seed)
    for o, ln in zip(offs, lens):
        stamp6(buf[o:o + ln], int(ln), nh)
    desc = np.zeros(n, DESC_DTYPE)
    desc["frame_off"] = fo
    desc["l3_off"] = l3_off
    desc["ip_len"] = lens
    return buf, desc, offs, lens
