"""cgck_l2_desc (l2d_kernel, cgck_l2d.hip) and cgck_synth_eth.  Every output of
every call is compared with the referee (tests/l2ref.py; further down the path
tests/rssref.py, tests/steerref.py and tests/mixedref.py over the oracle's port),
never with the library itself, by exact equality.  Every output array lies
between canary bytes that must survive, and `raw` and the frame bytes are read
back unchanged.  The frame buffer is a plain allocation of exactly the burst's
bytes, so a frame that ends the burst ends the allocation."""
import ctypes

import numpy as np
import pytest

import cgck
import l2batches as LB
import l2ref
import mixedbatches as MB
import mixedref
import rssbatches as RB
import rssref
import rxcorpus
import steerref
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("desc_out", "cls", "count")
CAN, CANARY = 64, 0xC3
NC = 16                                                 # counters allocated: 12 and four that stay untouched
SEED = (np.arange(NC, dtype=np.uint32) * 7 + 3)         # count[] before a call: running counters
KERNEL = {("desc_out",): "l2d_kernel<true, false>", ("cls",): "l2d_kernel<false, true>",
          ("count",): "l2d_kernel<false, true>", ("cls", "count"): "l2d_kernel<false, true>"}


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


def l2(eng, buf, raw, names=ALL, shift=0, calls=1):
    """cgck_l2_desc over host arrays, `calls` times: ({name: array}, kernel name).
    desc_out and cls start as 0xEE bytes, count as SEED."""
    n = len(raw)
    fr = Frames(eng, buf)
    dr = Guarded(eng, 12 * n, shift=shift).put(raw)
    sizes = {"desc_out": 12 * n, "cls": n, "count": 4 * NC}
    mem = {x: Guarded(eng, sizes[x], 0xEE, shift if x == "desc_out" else 0) for x in names}
    if "count" in mem:
        mem["count"].put(SEED)
    try:
        for _ in range(calls):
            eng.l2_desc(fr.ptr, dr.ptr, n, **{x: mem[x].ptr for x in names})
        kern = eng.last_kernel
        got = {x: mem[x].get({"desc_out": l2ref.DESC_DTYPE, "cls": np.uint8, "count": np.uint32}[x], x) for x in names}
        same(dr.get(np.uint8, "raw"), raw.view(np.uint8), "raw[] after the call")
        fr.unchanged()
    finally:
        for x in (fr, dr, *mem.values()):
            x.free()
    return got, kern


def judge(got, exp, what, calls=1):
    eout, ecls, ecount = exp
    for x in got:
        if x == "desc_out":
            for f in ("frame_off", "l3_off", "ip_len"):
                same(got[x][f], eout[f], f"desc_out.{f}, {what}")
        elif x == "cls":
            same(got[x], ecls, f"cls, {what}")
        else:
            want = SEED.copy()
            want[:l2ref.NCOUNT] += np.uint32(calls) * ecount
            same(got[x], want, f"count after {calls} call(s), {what}")


@pytest.fixture(scope="module")
def corpus():
    return LB.classes(np.random.default_rng(21))


# -- 1. the class corpus at every start alignment ---------------------------------------

@pytest.mark.parametrize("align", range(16))
def test_classes_every_alignment(engine, corpus, align):
    buf, raw = LB.lay(corpus, align)
    L = raw["ip_len"].astype(np.int64)
    start = raw["frame_off"].astype(np.int64) + raw["l3_off"]
    assert np.all((start & 15) == align) and int((start + L).max()) == len(buf)
    exp = l2ref.expect(buf, raw)
    assert set((exp[1] & 15).tolist()) == set(range(l2ref.NCLASS))
    got, kern = l2(engine, buf, raw)
    assert kern == "l2d_kernel<true, true>", kern
    judge(got, exp, f"alignment {align}")


# -- 2. burst sizes ----------------------------------------------------------------------

@pytest.mark.parametrize("size", ["1", "63", "64", "65", "255", "256", "257", "3 passes"])
def test_burst_sizes(engine, corpus, size):
    """64-byte slots tiled from the corpus.  The last size is above twice what one
    pass of the grid covers, a partial step short of three passes: every wave runs
    three steps, so both prefetch depths carry real frames and run dry."""
    per_pass = engine.l2_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024
    n = 3 * per_pass - 63 if size == "3 passes" else int(size)
    assert n > 2 * per_pass or n < 1024
    assert n * 64 < 64_000_000
    buf, raw, m = LB.tiled(corpus, n)
    exp = LB.expect_tiled(buf, raw, m)
    got, kern = l2(engine, buf, raw)
    assert kern.startswith("l2d_kernel<"), kern
    judge(got, exp, f"n {size} = {n}")


# -- 3. outputs --------------------------------------------------------------------------

@pytest.mark.parametrize("names", [("desc_out",), ("cls",), ("count",), ("cls", "count"), ALL])
def test_outputs(engine, corpus, names):
    buf, raw, m = LB.tiled(corpus, 700)
    exp = LB.expect_tiled(buf, raw, m)
    got, kern = l2(engine, buf, raw, names)
    assert tuple(got) == names and kern == KERNEL.get(names, "l2d_kernel<true, true>"), kern
    judge(got, exp, f"outputs {names}")


def test_count_accumulates(engine, corpus):
    """Two calls read exactly double; the words past the twelve counters stay."""
    buf, raw = LB.lay(corpus, 5)
    exp = l2ref.expect(buf, raw)
    assert np.all(exp[2][[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]] > 0)
    got, _ = l2(engine, buf, raw, ("count",), calls=2)
    judge(got, exp, "two calls", calls=2)
    same(got["count"][l2ref.NCOUNT:], SEED[l2ref.NCOUNT:], "count[12..]")


# -- 4. alignment of raw and desc_out ----------------------------------------------------

@pytest.mark.parametrize("shift", [4, 8, 12])
def test_descriptor_alignment(engine, corpus, shift):
    buf, raw, m = LB.tiled(corpus, 321)
    got, _ = l2(engine, buf, raw, shift=shift)
    judge(got, LB.expect_tiled(buf, raw, m), f"raw and desc_out at +{shift}")


# -- 5. arguments ------------------------------------------------------------------------

def test_arguments(engine, corpus):
    L = cgck.load()
    n = 64
    buf, raw, m = LB.tiled(corpus, n)
    fr = Frames(engine, buf)
    dr = Guarded(engine, 12 * n).put(raw)
    o = Guarded(engine, 4096, 0xEE)
    ctx, by, R = engine.ctx, ctypes.byref, cgck.L2Res
    full = R(o.ptr, o.ptr + 1024, o.ptr + 2048)

    def rc(c=ctx, base=fr.ptr, rw=dr.ptr, cnt=n, rs=full):
        return L.cgck_l2_desc(c, base, rw, cnt, None if rs is None else by(rs), None)

    try:
        for what, r in (("NULL ctx", rc(c=None)), ("NULL res", rc(rs=None)), ("NULL base", rc(base=None)),
                        ("NULL raw", rc(rw=None)), ("every output NULL", rc(rs=R(None, None, None))),
                        ("raw misaligned", rc(rw=dr.ptr + 2)), ("desc_out misaligned", rc(rs=R(o.ptr + 2, None, None))),
                        ("desc_out == raw", rc(rs=R(dr.ptr, None, None))),
                        ("n == 0, every output NULL", rc(cnt=0, rs=R(None, None, None))),
                        ("n == 0, NULL base", rc(cnt=0, base=None))):
            assert r == EINVAL, (what, r)
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        engine.strided(fr.ptr, n, 64, 0, 64, cgck.GEN_BOTH, o.ptr + 3072)
        engine.sync()
        before = engine.last_kernel
        assert not before.startswith("l2d_")
        assert rc(cnt=0) == 0 and rc(cnt=0, rw=None) == 0
        engine.sync()
        assert engine.last_kernel == before
        same(o.get(np.uint8, "outputs")[:3072], np.full(3072, 0xEE, np.uint8), "outputs after n == 0")
        # the same arguments with n > 0 are accepted
        assert rc() == 0 and engine.last_kernel == "l2d_kernel<true, true>"
        got = o.get(np.uint8, "outputs")
        eout, ecls, _ = LB.expect_tiled(buf, raw, m)
        same(got[:12 * n], eout.view(np.uint8), "desc_out")
        same(got[1024:1024 + n], ecls, "cls")
        same(dr.get(np.uint8, "raw"), raw.view(np.uint8), "raw[]")
        fr.unchanged()
    finally:
        for x in (fr, dr, o):
            x.free()


# -- 6. cgck_synth_eth -------------------------------------------------------------------

def test_synth_eth(engine, port):
    """25 frames: past two IMIX cycles and three vlan_every = 8 periods."""
    n, stride, l3, seed, eseed = 25, 2048, 18, 0x5EED, 0xE7
    buf, desc, offs, lens = MB.imix_dual(port, n, seed, stride=stride, l3_off=l3)
    raw = LB.synth_eth(buf, desc, 8, eseed)
    assert len(set(raw["l3_off"].tolist())) == 2 and np.count_nonzero(raw["ip_len"] == 60) == 0
    db = cgck.DeviceBuffer(n * stride)
    dd, dr, do = Guarded(engine, 12 * n, 0xEE), Guarded(engine, 12 * n, 0xEE), Guarded(engine, 12 * n, 0xEE)
    try:
        engine.synth_imix_dual(db.ptr, dd.ptr, n, seed, stride, l3)
        engine.synth_eth(db.ptr, dd.ptr, dr.ptr, n, 8, eseed)
        got = np.zeros(n * stride, np.uint8)
        db.download(got, stream=engine.stream)
        same(dd.get(np.uint8, "desc"), desc.view(np.uint8), "the set's descriptors")
        same(dr.get(np.uint8, "raw"), raw.view(np.uint8), "raw[]")
        same(got, buf, "the ring's bytes")
        engine.l2_desc(db.ptr, dr.ptr, n, desc_out=do.ptr)
        same(do.get(np.uint8, "desc_out"), desc.view(np.uint8), "l2_desc over the synthetic set")
        # 64-byte frames are padded to 60 + h > 60: none; a set at l3_off 14 has no room for a tag
        engine.synth_imix_dual(db.ptr, dd.ptr, n, seed, stride, 14)
        engine.sync()
        r = cgck.load().cgck_synth_eth(engine.ctx, db.ptr, dd.ptr, dr.ptr, n, 8, eseed, None)
        assert r == EINVAL, r
        same(dr.get(np.uint8, "raw"), raw.view(np.uint8), "raw[] after the refused call")
    finally:
        for x in (db, dd, dr, do):
            x.free()


# -- 7. the reason for the feature -------------------------------------------------------

def verify(eng, base, desc_ptr, n, flags):
    o, v = Guarded(eng, 4 * n, 0xEE), Guarded(eng, n, 0xEE)
    try:
        eng.desc(base, desc_ptr, n, flags, o.ptr, v.ptr)
        o.get(np.uint32, "out")
        return v.get(np.uint8, "verdict")
    finally:
        o.free()
        v.free()


def test_padded_frames_verify(engine, port):
    """A padded good frame verifies as CGCK_BAD_L4 under the descriptors a transport
    can write without reading the frame, and as good under cgck_l2_desc's."""
    rng = np.random.default_rng(31)
    flags = cgck.VERIFY_BSD | cgck.MIXED
    frames = rxcorpus.corpus(rng, port, 256, clean=True)
    buf, naive = rxcorpus.ring(frames)                   # {o, 14, L - 14}
    n = len(naive)
    raw = naive.copy()
    raw["l3_off"] = 0
    raw["ip_len"] = naive["ip_len"] + 14
    eout, ecls, _ = l2ref.expect(buf, raw)
    assert np.all(ecls & 15 == l2ref.IP4)
    offs, lens = eout["frame_off"].astype(np.int64) + eout["l3_off"], eout["ip_len"].astype(np.int64)
    ever = mixedref.expect(port, buf, offs, lens, flags)[1]
    good = ever == 0
    padded = lens < naive["ip_len"]
    assert np.count_nonzero(good & padded) > 5 and np.count_nonzero(~good) > 20
    fr = Frames(engine, buf)
    dn, dr, do = Guarded(engine, 12 * n).put(naive), Guarded(engine, 12 * n).put(raw), Guarded(engine, 12 * n, 0xEE)
    try:
        vn = verify(engine, fr.ptr, dn.ptr, n, flags)
        print(f"naive descriptors: {np.count_nonzero(vn[good & padded] & cgck.BAD_L4)} of "
              f"{np.count_nonzero(good & padded)} padded good frames marked BAD_L4")
        assert np.any(vn[good & padded] & cgck.BAD_L4), "no padded good frame was marked under the naive descriptors"
        engine.l2_desc(fr.ptr, dr.ptr, n, desc_out=do.ptr)
        same(do.get(np.uint8, "desc_out"), eout.view(np.uint8), "desc_out")
        vt = verify(engine, fr.ptr, do.ptr, n, flags)
        same(vt, ever, "verdicts under cgck_l2_desc's descriptors")
        assert not np.any(vt[good]), "an uncorrupted frame was marked"
        fr.unchanged()
    finally:
        for x in (fr, dn, dr, do):
            x.free()


# -- 8. end to end on one stream ---------------------------------------------------------

def wrap(rng, p):
    """An IP-or-not packet as a transport delivers it: the ethertype by its version
    nibble, 0 to 2 tags, padded to 60 bytes and sometimes beyond."""
    v = int(p[0]) >> 4 if len(p) else 0
    tg = LB.TAGSETS[int(rng.integers(0, len(LB.TAGSETS)))] if rng.integers(0, 3) == 0 else ()
    dst = (LB.BCAST_DST, (0x33, 0x33, 0, 0, 0, 9), None, None, None)[int(rng.integers(0, 5))]
    f = LB.eth(rng, 0x0800 if v == 4 else 0x86DD if v == 6 else 0x0806, p, tg, dst)
    pad = max(60 - len(f), 0) + int(rng.integers(0, 3)) * int(rng.integers(0, 12))
    return np.concatenate((f, rng.integers(1, 256, pad, dtype=np.uint8)))


def test_end_to_end(engine, port, corpus):
    """l2_desc, then rss_steer_desc with 7 queues, then each bin's slice through
    CGCK_VERIFY_TOY | CGCK_MIXED, all on the context's stream."""
    rng = np.random.default_rng(41)
    qn, flags, hf, slot = 7, cgck.VERIFY_TOY | cgck.MIXED, cgck.RSS_TCP | cgck.RSS_UDP, 2048
    key = np.frombuffer(bytes.fromhex(load_golden("rss_frames.json")["key"]), np.uint8).copy()
    plain = [f for f, l3 in corpus if l3 is None]
    fr_ = [wrap(rng, p) for p in RB.fuzz(rng, 220)] + [plain[i] for i in rng.permutation(len(plain))[:80]]
    fr_ = [fr_[i] for i in rng.permutation(len(fr_))]
    n = len(fr_)
    assert n == 300
    buf = LB.poison(n * slot, 1)
    raw = np.zeros(n, l2ref.DESC_DTYPE)
    for k, f in enumerate(fr_):
        l3 = (0, 2, 16)[k % 3]
        buf[k * slot + l3:k * slot + l3 + len(f)] = f
        raw[k] = (k * slot, l3, len(f))
    eout, ecls, _ = l2ref.expect(buf, raw)
    kinds = ecls & 15
    assert set(kinds.tolist()) == set(range(l2ref.NCLASS)) and np.count_nonzero(ecls & l2ref.VLAN) > 20
    assert np.count_nonzero((kinds <= l2ref.IP6) & (eout["ip_len"] + 14 < raw["ip_len"])) > 50       # padding cut off
    offs, lens = eout["frame_off"].astype(np.int64) + eout["l3_off"], eout["ip_len"].astype(np.int64)
    queue = rssref.expect(port, buf, offs, lens, key, hf, queue_num=qn)[2]
    qoff, perm, slot_of, dsteer = steerref.expect(queue, qn, eout.view(np.uint32).reshape(-1, 3))
    want_out, want_ver = mixedref.expect(port, buf, offs, lens, flags)
    noip = kinds > l2ref.IP6
    assert np.all(queue[noip] == rssref.NO_QUEUE) and np.all(want_ver[noip] == cgck.BAD_LEN)
    assert len(set(queue.tolist())) == qn + 1 and len(set(want_ver.tolist())) > 2

    fr = Frames(engine, buf)
    dr, d1, d2 = Guarded(engine, 12 * n).put(raw), Guarded(engine, 12 * n, 0xEE), Guarded(engine, 12 * n, 0xEE)
    q, qo, pm, sl = (Guarded(engine, n, 0xEE), Guarded(engine, 4 * (qn + 2), 0xEE), Guarded(engine, 4 * n, 0xEE),
                     Guarded(engine, 4 * n, 0xEE))
    o, v = Guarded(engine, 4 * n, 0xEE), Guarded(engine, n, 0xEE)
    try:
        engine.l2_desc(fr.ptr, dr.ptr, n, desc_out=d1.ptr)
        assert engine.last_kernel == "l2d_kernel<true, false>"
        engine.rss_steer_desc(fr.ptr, d1.ptr, n, cgck.Engine.rss_spec(key, 0xFFFFFFFF, hf, qn), q.ptr,
                              qoff=qo.ptr, perm=pm.ptr, slot=sl.ptr, desc_out=d2.ptr)
        for b in range(qn + 1):                          # no host read in between: the bins are the referee's
            lo, cnt = int(qoff[b]), int(qoff[b + 1] - qoff[b])
            assert cnt > 0
            engine.desc(fr.ptr, d2.ptr + 12 * lo, cnt, flags, o.ptr + 4 * lo, v.ptr + lo)
        same(d1.get(np.uint8, "desc_out"), eout.view(np.uint8), "l2_desc's descriptors")
        same(q.get(np.uint8, "queue"), queue, "queue")
        same(qo.get(np.uint32, "qoff"), qoff, "qoff")
        same(pm.get(np.uint32, "perm"), perm, "perm")
        same(sl.get(np.uint32, "slot"), slot_of, "slot")
        same(d2.get(np.uint32, "steered descriptors").reshape(n, 3), dsteer, "steered descriptors")
        out, ver = o.get(np.uint32, "out"), v.get(np.uint8, "verdict")
        same(ver, want_ver[perm], "verdict in slot order")
        same(out, want_out[perm], "out in slot order")
        lo = int(qoff[qn])
        assert set(perm[lo:].tolist()) >= set(np.nonzero(noip)[0].tolist())
        assert np.all(ver[slot_of[noip]] == cgck.BAD_LEN), "a non-IP or drop-class frame was not CGCK_BAD_LEN"
        same(dr.get(np.uint8, "raw"), raw.view(np.uint8), "raw[]")
        fr.unchanged()
    finally:
        for x in (fr, dr, d1, d2, q, qo, pm, sl, o, v):
            x.free()
