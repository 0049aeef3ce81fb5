"""Referee for the per-frame RSS hash (cgck_rss_strided / cgck_rss_desc /
cgck_rss_desc_host): the frame semantics of include/cgck.h, section 3, restated
in Python.  It finds each frame's tuple; the hash itself is delegated to an
oracle's toeplitz_hash (oracle.port() or oracle.reference_rss()).  Nothing here
calls the library under test."""
import numpy as np

RSS_TCP, RSS_UDP = 1 << 0, 1 << 1
BAD_LEN, NOT_IP, RSS_L4, RSS_IP6 = 1 << 2, 1 << 3, 1 << 4, 1 << 5
NO_QUEUE = 0xFF
OK, FRAG, BADLEN = "ok", "frag", "bad_len"


def walk6(p, ip_len):
    """(l4_off, nh, status) of the IPv6 frame p[:ip_len]: ip6ref.walk's loop
    without its last clause (no checksum field has to fit)."""
    if ip_len < 40:
        return 40, 0, BADLEN
    off, nh, seen = 40, int(p[6]), 0
    while True:
        if off > ip_len:
            return off, nh, BADLEN
        if nh == 44:
            return off, nh, FRAG
        if nh not in (0, 43, 60, 51):
            return off, nh, OK
        if seen == 8 or off + 2 > ip_len:
            return off, nh, BADLEN
        step = (int(p[off + 1]) + 2) * 4 if nh == 51 else (int(p[off + 1]) + 1) * 8
        nh, off, seen = int(p[off]), off + step, seen + 1


def ports_hashed(proto, hf):
    return (proto == 6 and bool(hf & RSS_TCP)) or (proto == 17 and bool(hf & RSS_UDP))


def tuple_of(p, ip_len, hf):
    """(kind, the hashed bytes or None) of the frame p[:ip_len]."""
    if ip_len == 0:
        return BAD_LEN, None
    v = int(p[0]) >> 4
    if v == 4:
        hl = (int(p[0]) & 15) * 4
        if ip_len < 20 or hl < 20 or ip_len < hl:
            return BAD_LEN, None
        frag = ((int(p[6]) << 8 | int(p[7])) & 0x3FFF) != 0
        if not frag and ip_len >= hl + 4 and ports_hashed(int(p[9]), hf):
            return RSS_L4, np.concatenate((p[12:20], p[hl:hl + 4]))
        return 0, np.array(p[12:20])
    if v == 6:
        off, nh, st = walk6(p, ip_len)
        if st == BADLEN:
            return BAD_LEN, None
        if st == OK and ports_hashed(nh, hf) and ip_len >= off + 4:
            return RSS_IP6 | RSS_L4, np.concatenate((p[8:40], p[off:off + 4]))
        return RSS_IP6, np.array(p[8:40])
    return NOT_IP, None


def expect(oracle_obj, buf, offs, lens, key, hf, mask=0xFFFFFFFF, queue_num=0, key_size=None):
    """hash (u32), kind (u8) and queue (u8, 0xFF where there is no hash; all
    0xFF with queue_num 0) of a batch: frame i is buf[offs[i] : offs[i] + lens[i]]."""
    n = len(offs)
    h = np.zeros(n, np.uint32)
    kind = np.zeros(n, np.uint8)
    queue = np.full(n, NO_QUEUE, np.uint8)
    for i in range(n):
        o, ln = int(offs[i]), int(lens[i])
        kind[i], t = tuple_of(buf[o:o + ln], ln, hf)
        if t is None:
            continue
        h[i] = oracle_obj.toeplitz_hash(np.ascontiguousarray(t, np.uint8), key, key_size=key_size) & mask
        if queue_num:
            queue[i] = int(h[i]) % queue_num
    return h, kind, queue


def hashed(kind):
    """Which frames of a kind array carry a hash."""
    return (np.asarray(kind) & (BAD_LEN | NOT_IP)) == 0
