"""IPv6 referee for the CGCK_IP6 tests: the semantics of include/cgck.h
restated in Python, with every checksum delegated to an oracle's in_cksum
(oracle.port() or oracle.reference()) run over pseudo-header || segment.
Nothing here calls the library under test."""
import numpy as np

IP, L4, ZERO_FIELDS, STORE, VERIFY, V_UDP_ZERO_SKIP, IP6 = 1 << 1, 1 << 2, 1 << 4, 1 << 5, 1 << 6, 1 << 8, 1 << 9
BAD_L4, BAD_LEN = 2, 4
OK, NO_L4, BADLEN = "ok", "no_l4", "bad_len"
FIELD = {6: 16, 17: 6, 58: 2}


def walk(p, ip_len):
    """(l4_off, terminal nh, status) of the IPv6 packet p[:ip_len]."""
    if ip_len < 40:
        return 40, 0, BADLEN
    off, nh, seen = 40, int(p[6]), 0
    while True:
        if off > ip_len:
            return off, nh, BADLEN
        if nh == 44:
            return off, nh, NO_L4
        if nh not in (0, 43, 60, 51):
            break
        if seen == 8 or off + 2 > ip_len:
            return off, nh, BADLEN
        step = (int(p[off + 1]) + 2) * 4 if nh == 51 else (int(p[off + 1]) + 1) * 8
        nh, off, seen = int(p[off]), off + step, seen + 1
    if nh in FIELD and off + FIELD[nh] + 2 > ip_len:
        return off, nh, BADLEN
    return off, nh, OK


def pseudo(p, l4_off, nh, ip_len):
    """The 40-byte pseudo-header: src, dst, length as 32 bits big-endian, 0 0 0 nh."""
    n = ip_len - l4_off
    return np.concatenate((np.asarray(p[8:40], np.uint8),
                           np.array([n >> 24, (n >> 16) & 255, (n >> 8) & 255, n & 255, 0, 0, 0, nh], np.uint8)))


def l4_cksum(oracle_obj, p, ip_len, zero_field):
    """(status, l4_off, nh, field offset or None, out.hi) of one packet."""
    l4, nh, st = walk(p, ip_len)
    if st != OK:
        return st, l4, nh, None, 0
    fo = l4 + FIELD[nh] if nh in FIELD else None
    seg = np.array(p[l4:ip_len], np.uint8)
    if zero_field and fo is not None:
        seg[fo - l4:fo - l4 + 2] = 0
    buf = np.ascontiguousarray(np.concatenate((pseudo(p, l4, nh, ip_len), seg)))
    return st, l4, nh, fo, oracle_obj.in_cksum(buf, 0, len(buf))


def expect(oracle_obj, buf, offs, lens, flags):
    """out (u32), verdict (u8) and, with STORE, the bytes after the fill, of a
    header-mode batch: packet i is buf[offs[i] : offs[i] + lens[i]]."""
    n = len(offs)
    out = np.zeros(n, np.uint32)
    ver = np.zeros(n, np.uint8)
    after = buf.copy()
    zero = bool(flags & (ZERO_FIELDS | VERIFY))
    for i in range(n):
        o, ln = int(offs[i]), int(lens[i])
        p = buf[o:o + ln]
        if ln < 40:
            ver[i] = BAD_LEN
            continue
        if not flags & L4:
            continue
        st, l4, nh, fo, hi = l4_cksum(oracle_obj, p, ln, zero)
        if st == BADLEN:
            ver[i] = BAD_LEN
        if st != OK:
            continue
        out[i] = hi << 16
        if fo is None:
            continue
        stored = int(p[fo]) | int(p[fo + 1]) << 8
        if flags & VERIFY and not (flags & V_UDP_ZERO_SKIP and nh == 17 and stored == 0) and stored != hi:
            ver[i] |= BAD_L4
        if flags & STORE:
            after[o + fo] = hi & 255
            after[o + fo + 1] = hi >> 8
    return out, ver, after


def ext(kind, next_nh, nbytes, rng):
    """One extension header of `kind` (0, 43, 60: nbytes a multiple of 8; 51: of
    4, at least 8) leading to next_nh, random body."""
    h = rng.integers(0, 256, nbytes, dtype=np.uint8)
    h[0] = next_nh
    h[1] = nbytes // 4 - 2 if kind == 51 else nbytes // 8 - 1
    return h


def packet(rng, ip_len, nh, chain=()):
    """A random IPv6 packet of ip_len bytes: chain = ((kind, nbytes), ...)
    extension headers before the upper-layer protocol nh.  Bytes the chain
    would put past ip_len are cut off (the BAD_LEN cases)."""
    p = rng.integers(0, 256, max(ip_len, 40), dtype=np.uint8)
    p[0:4] = (0x60, 0, 0, 0)
    p[4] = ((ip_len - 40) >> 8) & 255
    p[5] = (ip_len - 40) & 255
    kinds = [k for k, _ in chain] + [nh]
    p[6] = kinds[0]
    off = 40
    for i, (kind, nbytes) in enumerate(chain):
        h = ext(kind, kinds[i + 1], nbytes, rng)
        room = max(0, min(nbytes, len(p) - off))
        p[off:off + room] = h[:room]
        off += nbytes
    return p[:ip_len]


def stamp_strided(buf, n, stride, ip_len, nh):
    """cgck_synth_strided_ip6's stamps on a stream_bytes buffer, vectorised."""
    v = buf[:n * stride].reshape(n, stride)
    v[:, 0] = 0x60
    v[:, 1:4] = 0
    v[:, 4] = (ip_len - 40) >> 8
    v[:, 5] = (ip_len - 40) & 255
    v[:, 6] = nh
    if nh in FIELD and 40 + FIELD[nh] + 2 <= ip_len:
        v[:, 40 + FIELD[nh]:40 + FIELD[nh] + 2] = 0
