"""The seeded differential cases of the CPU suite, as functions of the
implementation under them: the tests run them over the restatement (oracle
port) and compare with tests/golden/differential.json, which
tests/golden/make_golden.py recorded by running the same functions over the
reference's own build (oracle/_ref); where that build is present the tests
also run both side by side."""
import hashlib
import json
import os

import numpy as np

import rxcorpus


def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "differential.json")) as f:
        return json.load(f)


def cksum_random(C):
    """in_cksum / udp_cksum of C over 20000 random (offset, length) pairs of
    one 4 KiB buffer whose header-length nibbles change as the walk goes."""
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8)
    a, b = [], []
    for _ in range(20000):
        off = int(rng.integers(0, 16))
        n = int(rng.integers(0, 1700))
        a.append(C.in_cksum(buf, off, n))
        o2 = int(rng.integers(0, 16))
        buf[o2] = (int(buf[o2]) & 0xF0) | int(rng.integers(0, 16))
        hl = (int(buf[o2]) & 15) * 4
        n2 = int(rng.integers(0, 4096 - o2 - hl))
        b.append(C.udp_cksum(buf, o2, n2))
    return a, b


def rss_random(C, key):
    """toeplitz_hash of C over 3000 random (data, key, cnt, key_size) and
    rss_hash4 over 2000 random tuples with `key`."""
    rng = np.random.default_rng(99)
    t, r = [], []
    for _ in range(3000):
        cnt = int(rng.integers(0, 64))
        ks = int(rng.integers(0, 80))
        d = rng.integers(0, 256, max(cnt, 1), dtype=np.uint8)
        k = rng.integers(0, 256, max(ks, 4), dtype=np.uint8)
        t.append(C.toeplitz_hash(d, k, cnt, ks))
    for _ in range(2000):
        la, fa = (int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64))
        lp, fp = (int(x) for x in rng.integers(0, 1 << 16, 2))
        r.append(C.rss_hash4(la, fa, lp, fp, key))
    return t, r


RX_CONFIGS = [(stack, ip_in, tcp_in) for stack in (0, 1)
              for ip_in, tcp_in in ((0, 0), (1, 1), (2, 2), (1, 2), (2, 1))]


def digest(arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def rx_replays(port, C):
    """The RX replay (oracle/stack_replay.c) with C's in_cksum / udp_cksum
    over a 600-frame corpus stamped by C, per RX_CONFIGS: the
    (outcomes, counters, ring bytes) of each."""
    rng = np.random.default_rng(11)
    frames = rxcorpus.corpus(rng, C, 600)
    fns = C.fn_pointers()
    out = []
    for stack, ip_in, tcp_in in RX_CONFIGS:
        buf, desc = rxcorpus.ring(frames)
        res, ctr = port.replay_rx(fns[0], fns[1], buf, desc.view(np.uint8), len(desc), stack, ip_in, tcp_in)
        out.append((res, ctr, buf))
    return out


def keepalives(rng, n):
    import oracle
    ka = np.zeros(n, oracle.Port.KA_DTYPE)
    ka["laddr"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ka["faddr"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ka["lport"] = rng.integers(0, 2 ** 16, n)
    ka["fport"] = rng.integers(0, 2 ** 16, n)
    ka["rcv_nxt"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ka["snd_una"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    ka["hiwat"] = rng.integers(0, 2 ** 20, n)
    ka["scale"] = rng.integers(0, 9, n)
    return ka


def rsp_replay(port, C):
    """The response replay (oracle_replay_rx_rsp) with C's functions over a
    600-frame corpus stamped by C and 20 keepalives: (outcomes, counters,
    replies sent, ip ids, the pool after the run, tx_base, tx_stride)."""
    rng = np.random.default_rng(81)
    frames = rxcorpus.rsp_corpus(rng, C, 600)
    buf, desc, tx_base, tx_stride = rxcorpus.pool(frames, 700)
    ka = keepalives(rng, 20)
    fns = C.fn_pointers()
    local = np.zeros(2048 * 64, np.uint8)
    res, ctr, txs, idn = port.replay_rx_rsp(fns[0], fns[1], buf, desc.view(np.uint8), len(desc), 1, 1,
                                            buf[tx_base:], tx_stride, 700, local, rxcorpus.LADDR, ka, 77)
    return res, ctr, txs, idn, buf, tx_base, tx_stride
