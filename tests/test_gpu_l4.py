"""cgck_l4_desc (l4d_kernel, cgck_l4d.hip).  Every output of every call is compared
with the referee (tests/l4ref.py), never with the library itself, by exact
equality.  Every output array lies between canary bytes that must survive, and
`desc` and the frame bytes are read back unchanged.  The frame buffer is a plain
allocation of exactly the burst's bytes, so a frame that ends the burst ends the
allocation."""
import ctypes
import itertools
import socket

import numpy as np
import pytest

import cgck
import l4batches as LB
import l4ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("seg", "cls", "hash", "count")
CAN, CANARY = 64, 0xC3
NC = 16                                                 # counters allocated: 12 and four that stay untouched
SEED = (np.arange(NC, dtype=np.uint32) * 5 + 2)         # count[] before a call: running counters
DTYPES = {"seg": l4ref.SEG_DTYPE, "cls": np.uint8, "hash": np.uint32, "count": np.uint32}


def kernel_of(names):
    return "l4d_kernel<%s, %s>" % (("false", "true")["seg" in names], ("false", "true")[len(set(names) - {"seg"}) > 0])


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {got[bad[:5]]}, want {exp[bad[:5]]}"


class Guarded:
    """`nbytes` of device memory at `shift` bytes past a canary, a canary after it."""

    def __init__(self, eng, nbytes, fill=CANARY, shift=0):
        self.eng, self.nbytes, self.at = eng, nbytes, CAN + shift
        self.host = np.full(self.at + nbytes + CAN, CANARY, np.uint8)
        self.host[self.at:self.at + nbytes] = fill
        self.buf = cgck.DeviceBuffer(len(self.host))
        self.buf.upload(self.host, stream=eng.stream)
        self.ptr = self.buf.ptr + self.at

    def put(self, arr):
        arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert arr.nbytes == self.nbytes
        self.host[self.at:self.at + self.nbytes] = arr
        self.buf.upload(self.host, stream=self.eng.stream)
        return self

    def get(self, dtype, what):
        """The array after the calls so far; the canaries must be whole."""
        after = np.zeros_like(self.host)
        self.buf.download(after, stream=self.eng.stream)
        self.eng.sync()
        lo, hi = after[:self.at], after[self.at + self.nbytes:]
        assert np.all(lo == CANARY) and np.all(hi == CANARY), f"{what}: bytes outside the array were written"
        return after[self.at:self.at + self.nbytes].copy().view(dtype)

    def free(self):
        self.buf.free()


class Frames:
    """The burst's bytes in an allocation of exactly their size."""

    def __init__(self, eng, buf):
        self.eng, self.host = eng, buf
        self.buf = cgck.DeviceBuffer(max(buf.nbytes, 1))
        assert self.buf.ptr % 16 == 0
        self.buf.upload(buf, stream=eng.stream)
        self.ptr = self.buf.ptr

    def unchanged(self):
        after = np.zeros_like(self.host)
        self.buf.download(after, stream=self.eng.stream)
        self.eng.sync()
        assert np.array_equal(after, self.host), "the frame bytes changed"

    def free(self):
        self.buf.free()


def l4(eng, buf, desc, names=ALL, shift=0, calls=1):
    """cgck_l4_desc over host arrays, `calls` times: ({name: array}, kernel name).
    seg, cls and hash start as 0xEE bytes, count as SEED; desc lies `shift` bytes
    past a 16-byte boundary."""
    n = len(desc)
    fr = Frames(eng, buf)
    dr = Guarded(eng, 12 * n, shift=shift).put(desc)
    sizes = {"seg": 32 * n, "cls": n, "hash": 4 * n, "count": 4 * NC}
    mem = {x: Guarded(eng, sizes[x], 0xEE) for x in names}
    if "count" in mem:
        mem["count"].put(SEED)
    try:
        for _ in range(calls):
            eng.l4_desc(fr.ptr, dr.ptr, n, **{x: mem[x].ptr for x in names})
        kern = eng.last_kernel
        got = {x: mem[x].get(DTYPES[x], x) for x in names}
        same(dr.get(np.uint8, "desc"), desc.view(np.uint8), "desc[] after the call")
        fr.unchanged()
    finally:
        for x in (fr, dr, *mem.values()):
            x.free()
    return got, kern


def judge(got, exp, what, calls=1):
    eseg, ecls, ehash, ecount = exp
    for x in got:
        if x == "seg":
            for f in l4ref.FIELDS:
                same(got[x][f], eseg[f], f"seg.{f}, {what}")
        elif x == "cls":
            same(got[x], ecls, f"cls, {what}")
        elif x == "hash":
            same(got[x], ehash, f"hash, {what}")
        else:
            want = SEED.copy()
            want[:l4ref.NCOUNT] += np.uint32(calls) * ecount
            same(got[x], want, f"count after {calls} call(s), {what}")


@pytest.fixture(scope="module")
def corpus():
    return LB.classes(np.random.default_rng(21))


@pytest.fixture(scope="module")
def tiled700(corpus):
    buf, desc, m = LB.tiled(corpus, 700)
    return buf, desc, LB.expect_tiled(buf, desc, m)


# -- 1. the class corpus at every start alignment ---------------------------------------

@pytest.mark.parametrize("align", range(16))
def test_classes_every_alignment(engine, corpus, align):
    buf, desc = LB.lay(corpus, align)
    start = desc["frame_off"].astype(np.int64) + desc["l3_off"]
    assert np.all((start & 15) == align) and int((start + desc["ip_len"]).max()) == len(buf)
    exp = l4ref.expect(buf, desc)
    assert {int(c) for c in exp[1]} >= {c | f for c in range(l4ref.NCLASS) for f in (0, l4ref.IP6)}
    got, kern = l4(engine, buf, desc, shift=4 * (align % 4))
    assert kern == "l4d_kernel<true, true>", kern
    judge(got, exp, f"alignment {align}")


# -- 2. outputs --------------------------------------------------------------------------

@pytest.mark.parametrize("names", [c for r in (1, 2, 3, 4) for c in itertools.combinations(ALL, r)], ids="+".join)
def test_outputs(engine, tiled700, names):
    """Every subset of the outputs; the counters after two calls (+=), with the four
    words past them untouched."""
    buf, desc, exp = tiled700
    got, kern = l4(engine, buf, desc, names, calls=2)
    assert tuple(got) == names and kern == kernel_of(names), kern
    judge(got, exp, f"outputs {names}", calls=2)
    if "count" in got:
        assert np.all(exp[3][:l4ref.NCLASS] > 0) and exp[3][11] > 0
        same(got["count"][l4ref.NCOUNT:], SEED[l4ref.NCOUNT:], "count[12..]")


# -- 3. burst sizes ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_tails(engine, corpus, n):
    buf, desc, m = LB.tiled(corpus, n)
    got, kern = l4(engine, buf, desc)
    assert kern == "l4d_kernel<true, true>", kern
    judge(got, LB.expect_tiled(buf, desc, m), f"n {n}")


def test_three_passes(engine, corpus):
    """Above twice what one pass of the grid covers, plus a step and a frame: every
    wave runs three steps, so both prefetch depths carry real frames and run dry
    (the zero chunk past the end)."""
    per_pass = engine.l4_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024
    n = 2 * per_pass + 65
    assert n * 128 < 128_000_000
    buf, d1, m = LB.tiled(corpus, 1)
    piece = 64 * m                                      # frames per piece: whole periods, under 1 MiB of records
    buf, dp, _ = LB.tiled(corpus, piece)
    eseg, ecls, ehash, ecount = LB.expect_tiled(buf, dp, m)
    reps = -(-n // piece)
    # The descriptors go up and the results come down a piece at a time, and the
    # burst's bytes are the piece's, repeated: the host never holds an array of
    # the whole burst other than the frame bytes.
    fr = Frames(engine, np.tile(buf, reps)[:n * 128])
    L, st = cgck.load(), engine.stream
    sizes = {"desc": 12 * n, "seg": 32 * n, "cls": n, "hash": 4 * n, "count": 4 * NC}
    dev = {x: cgck.DeviceBuffer(2 * CAN + sz) for x, sz in sizes.items()}
    try:
        for x, d in dev.items():
            assert L.cgck_memset(d.ptr, CANARY, 2 * CAN + sizes[x], st) == 0
            assert L.cgck_memset(d.ptr + CAN, 0xEE, sizes[x], st) == 0
        dev["count"].upload(SEED, off=CAN, stream=st)
        for a in range(0, n, piece):
            d = dp[:min(piece, n - a)].copy()
            d["frame_off"] += np.uint64(128 * a)
            dev["desc"].upload(d, off=CAN + 12 * a, stream=st)
        engine.sync()
        engine.l4_desc(fr.ptr, dev["desc"].ptr + CAN, n, **{x: dev[x].ptr + CAN for x in ALL})
        assert engine.last_kernel == "l4d_kernel<true, true>", engine.last_kernel

        def fetch(x, off, count, dtype):
            got = np.zeros(count, dtype)
            dev[x].download(got, off=off, stream=st)
            engine.sync()
            return got

        total = np.zeros(l4ref.NCOUNT, np.uint64)
        for a in range(0, n, piece):
            k = min(piece, n - a)
            gs = fetch("seg", CAN + 32 * a, k, l4ref.SEG_DTYPE)
            same(gs.view(np.uint8), eseg[:k].view(np.uint8), f"seg, frames {a} ..")
            same(fetch("cls", CAN + a, k, np.uint8), ecls[:k], f"cls, frames {a} ..")
            same(fetch("hash", CAN + 4 * a, k, np.uint32), ehash[:k], f"hash, frames {a} ..")
            gd = fetch("desc", CAN + 12 * a, k, l4ref.DESC_DTYPE)
            assert np.array_equal(gd["ip_len"], dp["ip_len"][:k]) and int(gd["frame_off"][k - 1]) == 128 * (a + k - 1)
            total += LB.counts(ecls[:k])
        want = SEED.copy()
        want[:l4ref.NCOUNT] += total.astype(np.uint32)
        same(fetch("count", CAN, NC, np.uint32), want, "count")
        for x, d in dev.items():
            for off in (0, CAN + sizes[x]):
                assert np.all(fetch(x, off, CAN, np.uint8) == CANARY), f"{x}: bytes outside the array were written"
        fr.unchanged()
    finally:
        for d in (fr, *dev.values()):
            d.free()


# -- 4. fuzz -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed, align", [(51, 3), (52, 12)])
def test_fuzz(engine, seed, align):
    """2000 frames in all: random bytes behind IP headers of every shape, random
    data offsets, option areas drawn from the kinds the walk tells apart."""
    rng = np.random.default_rng(seed)
    items = [(f, None, None) for f in LB.fuzz(rng, 1000)]
    if len(items[-1][0]) == 0:
        items.append((LB.ip4(rng, LB.tcp(rng), 6), None, None))
    buf, desc = LB.lay(items, align)
    exp = l4ref.expect(buf, desc)
    assert np.count_nonzero(exp[3][:l4ref.NCLASS]) == l4ref.NCLASS
    opts = {int(o) for o in exp[0]["opt"]}            # the walk is exercised: each bit alone, and with OPT_BAD
    assert opts >= {0, l4ref.MSS, l4ref.TS, l4ref.OPT_BAD, l4ref.OPT_BAD | l4ref.MSS, l4ref.OPT_BAD | l4ref.TS}
    got, _ = l4(engine, buf, desc)
    judge(got, exp, f"fuzz seed {seed}")


# -- 5. composition ----------------------------------------------------------------------

def test_after_l2_rss_steer(engine):
    """cgck_synth_imix_dual ring -> cgck_synth_eth -> cgck_l2_desc ->
    cgck_rss_steer_desc -> cgck_l4_desc over desc_out, in queue order: the referee's
    records on the same descriptors, and the arrival-order records permuted by perm."""
    n, stride, l3, qn = 300, 2048, 18, 5
    key = np.frombuffer(bytes.fromhex(load_golden("rss_frames.json")["key"]), np.uint8).copy()
    db = cgck.DeviceBuffer(n * stride)
    dd, dr, d1, d2 = (Guarded(engine, 12 * n, 0xEE) for _ in range(4))
    q, qo, pm = Guarded(engine, n, 0xEE), Guarded(engine, 4 * (qn + 2), 0xEE), Guarded(engine, 4 * n, 0xEE)
    sa, sq, cq, hq = Guarded(engine, 32 * n, 0xEE), Guarded(engine, 32 * n, 0xEE), Guarded(engine, n, 0xEE), Guarded(engine, 4 * n, 0xEE)
    try:
        engine.synth_imix_dual(db.ptr, dd.ptr, n, 0x5EED, stride, l3)
        engine.synth_eth(db.ptr, dd.ptr, dr.ptr, n, 8, 0xE7)
        engine.l2_desc(db.ptr, dr.ptr, n, desc_out=d1.ptr)
        engine.rss_steer_desc(db.ptr, d1.ptr, n, cgck.Engine.rss_spec(key, 0xFFFFFFFF, cgck.RSS_TCP | cgck.RSS_UDP, qn),
                              q.ptr, qoff=qo.ptr, perm=pm.ptr, desc_out=d2.ptr)
        engine.l4_desc(db.ptr, d1.ptr, n, seg=sa.ptr)
        engine.l4_desc(db.ptr, d2.ptr, n, seg=sq.ptr, cls=cq.ptr, hash=hq.ptr)
        buf = np.zeros(n * stride, np.uint8)
        db.download(buf, stream=engine.stream)
        arrival, steered = d1.get(l4ref.DESC_DTYPE, "l2_desc's descriptors"), d2.get(l4ref.DESC_DTYPE, "steered descriptors")
        perm, qoff = pm.get(np.uint32, "perm"), qo.get(np.uint32, "qoff")
        # every queue has frames; every frame of the set is IP, so the unsteered bin is empty
        assert sorted(perm.tolist()) == list(range(n)) and qoff[qn] == qoff[qn + 1] == n
        assert np.all(np.diff(qoff[:qn + 1].astype(np.int64)) > 0)
        same(steered.view(np.uint8), arrival[perm].view(np.uint8), "desc_out against desc[perm]")
        eseg, ecls, ehash, ecount = l4ref.expect(buf, steered)
        # the set's header bytes are random: IPv4 frames are nearly all FRAG (random ip_off), the
        # IPv6 ones spread over the TCP and UDP classes; two frames in five are IPv6
        assert ecount[l4ref.NONE] == 0 and ecount[11] == 120 and ecount[l4ref.FRAG] > 100
        assert all(ecount[c] > 10 for c in (l4ref.TCP, l4ref.ICMP, l4ref.TCP_BADOFF, l4ref.TCP_OFFLONG, l4ref.UDP_BADLEN))
        assert np.count_nonzero(eseg["opt"]) > 5
        got_q, got_a = sq.get(l4ref.SEG_DTYPE, "seg"), sa.get(l4ref.SEG_DTYPE, "seg in arrival order")
        for f in l4ref.FIELDS:
            same(got_q[f], eseg[f], f"seg.{f} in queue order")
        same(cq.get(np.uint8, "cls"), ecls, "cls in queue order")
        same(hq.get(np.uint32, "hash"), ehash, "hash in queue order")
        same(got_q.view(np.uint8), got_a[perm].view(np.uint8), "queue-order records against arrival-order records[perm]")
    finally:
        for x in (db, dd, dr, d1, d2, q, qo, pm, sa, sq, cq, hq):
            x.free()


# -- 6. the hash is the dst-cache entry's ------------------------------------------------

def test_hash_of_replies_to_dst_cache(engine):
    """Replies to the entries of a cgck_dst_cache_host build: hash[k] == entry.hash."""
    key = np.frombuffer(bytes.fromhex(load_golden("rss.json")["keys"]["freebsd"]), np.uint8).copy()
    ent = engine.dst_cache_host(cgck.Engine.dst_params((0x0A000001, 0x0A000003), (0x0A010001, 0x0A010002),
                                                       socket.htons(80), 4, 1, key), 300)
    n = len(ent)
    assert n > 100
    raw = ent.view(np.uint8).reshape(n, 16)
    rng = np.random.default_rng(61)
    items = []
    for k in range(n):
        ports = np.concatenate((raw[k, 10:12], raw[k, 8:10]))        # from fport to lport
        if k % 2:
            l4b = LB.udp(rng, 8 + k % 9, 8 + k % 9)
        else:
            l4b = LB.tcp(rng, 20 + 4 * (k % 3), LB.SYN | LB.ACK, (1,) * (4 * (k % 3)), k % 5)
        l4b[0:4] = ports
        p = LB.ip4(rng, l4b, (6, 17)[k % 2], (5, 5, 7)[k % 3])
        p[12:16], p[16:20] = raw[k, 4:8], raw[k, 0:4]                # from faddr to laddr
        items.append((p, None, None))
    buf, desc = LB.lay(items, 6)
    exp = l4ref.expect(buf, desc)
    got, _ = l4(engine, buf, desc, ("hash", "cls"))
    judge(got, exp, "replies")
    same(got["hash"], ent["hash"], "hash against the entries' SO_HASH")
    assert set(got["cls"].tolist()) == {l4ref.TCP, l4ref.UDP}


# -- 7. arguments ------------------------------------------------------------------------

def test_arguments(engine, tiled700):
    L = cgck.load()
    n = 64
    buf, desc, exp = tiled700
    buf, desc = buf[:n * 128], desc[:n]
    fr = Frames(engine, buf)
    dr = Guarded(engine, 12 * n).put(desc)
    o = Guarded(engine, 8192, 0xEE)
    ctx, by, R = engine.ctx, ctypes.byref, cgck.L4Res
    assert o.ptr % 16 == 0
    full = R(o.ptr, o.ptr + 2048, o.ptr + 3072, o.ptr + 4096)

    def rc(c=ctx, base=fr.ptr, ds=dr.ptr, cnt=n, rs=full):
        return L.cgck_l4_desc(c, base, ds, cnt, None if rs is None else by(rs), None)

    try:
        for what, r in (("NULL ctx", rc(c=None)), ("NULL res", rc(rs=None)), ("NULL base", rc(base=None)),
                        ("NULL desc", rc(ds=None)), ("every output NULL", rc(rs=R(None, None, None, None))),
                        ("desc misaligned", rc(ds=dr.ptr + 2)), ("seg at +8", rc(rs=R(o.ptr + 8, None, None, None))),
                        ("seg at +4", rc(rs=R(o.ptr + 4, o.ptr + 2048, None, None))),
                        ("n == 0, every output NULL", rc(cnt=0, rs=R(None, None, None, None))),
                        ("n == 0, seg misaligned", rc(cnt=0, rs=R(o.ptr + 8, None, None, None))),
                        ("n == 0, NULL base", rc(cnt=0, base=None))):
            assert r == EINVAL, (what, r)
        same(o.get(np.uint8, "outputs"), np.full(8192, 0xEE, np.uint8), "outputs after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        engine.strided(fr.ptr, n, 128, 0, 64, cgck.GEN_BOTH, o.ptr + 6144)
        engine.sync()
        before = engine.last_kernel
        assert not before.startswith("l4d_")
        assert rc(cnt=0) == 0 and rc(cnt=0, ds=None) == 0
        engine.sync()
        assert engine.last_kernel == before
        same(o.get(np.uint8, "outputs")[:6144], np.full(6144, 0xEE, np.uint8), "outputs after n == 0")
        # the same arguments with n > 0 are accepted
        assert rc() == 0 and engine.last_kernel == "l4d_kernel<true, true>"
        got = o.get(np.uint8, "outputs")
        same(got[:32 * n], exp[0][:n].view(np.uint8), "seg")
        same(got[2048:2048 + n], exp[1][:n], "cls")
        same(got[3072:3072 + 4 * n].view(np.uint32), exp[2][:n], "hash")
        same(got[4096:4096 + 4 * l4ref.NCOUNT].view(np.uint32), np.uint32(0xEEEEEEEE) + LB.counts(exp[1][:n]),
             "count (running from 0xEEEEEEEE)")
        same(dr.get(np.uint8, "desc"), desc.view(np.uint8), "desc[]")
        fr.unchanged()
    finally:
        for x in (fr, dr, o):
            x.free()
