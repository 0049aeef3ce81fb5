"""cgck_steer and cgck_rss_steer_desc (cgck_steer.hip): the stable partition of a
burst by queue id.  Every output of every call is compared with the referee
(tests/steerref.py: numpy's stable argsort; for the fused call over
tests/rssref.py's queue ids, for the end-to-end run tests/mixedref.py's
verdicts), never with the library itself, by exact equality.  Every output array
and the workspace lie between canary bytes that must survive, and the inputs are
read back unchanged.  The tile size comes from cgck_test_steer_plan."""
import ctypes

import numpy as np
import pytest

import cgck
import mixedref
import rssbatches as RB
import rssref
import steerref
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("qoff", "perm", "slot", "desc_out")
CAN = 64                     # canary bytes on each side of an array (a multiple of 16)
CANARY = 0xC3
SCAN_PASS = 4096             # words per pass of steer_scan_kernel
ONE = "steer_one_kernel<"
SCATTER = "steer_scatter_kernel<"
SIZES = {"1": lambda T: 1, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65, "255": lambda T: 255,
         "256": lambda T: 256, "257": lambda T: 257, "T-1": lambda T: T - 1, "T": lambda T: T,
         "T+1": lambda T: T + 1, "2T+65": lambda T: 2 * T + 65}


def tile(queue_num=7):
    return cgck.steer_plan(1, queue_num)[0]


def tf(b):
    return "true" if b else "false"


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


def descs(rng, n):
    """n descriptors as u32[n][3]: cgck_steer moves them and never reads their fields."""
    return rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint32)


def steer(eng, queue, qn, desc=None, names=ALL, work_fill=0xA5, shift=0, null_work=False, twice=None):
    """One cgck_steer call over host arrays: ({name: array}, kernel name).  Every
    output starts as 0xEE bytes; inputs and canaries are checked afterwards.
    twice: a second workspace fill to call again with (both results must agree)."""
    queue = np.ascontiguousarray(queue, np.uint8)
    n = len(queue)
    sizes = {"qoff": 4 * (qn + 2), "perm": 4 * n, "slot": 4 * n, "desc_out": 12 * n}
    mem = {x: Guarded(eng, sizes[x], 0xEE, shift if x == "desc_out" else 0) for x in names}
    dq = Guarded(eng, n).put(queue)
    di = Guarded(eng, 12 * n, shift=shift).put(desc) if desc is not None else None
    wb = cgck.steer_work_bytes(n, qn)
    assert (wb == 0) == (cgck.steer_plan(n, qn)[1] <= 1)
    dw = Guarded(eng, wb, work_fill) if wb and not null_work else None
    try:
        eng.steer(dq.ptr, n, qn, di.ptr if di else None, work=dw.ptr if dw else None,
                  **{x: mem[x].ptr for x in names})
        kern = eng.last_kernel
        got = {x: mem[x].get(np.uint32, x) for x in names}
        if twice is not None and dw:
            dw.put(np.full(wb, twice, np.uint8))
            for x in names:
                mem[x].put(np.full(sizes[x], 0xEE, np.uint8))
            eng.steer(dq.ptr, n, qn, di.ptr if di else None, work=dw.ptr, **{x: mem[x].ptr for x in names})
            for x in names:
                same(mem[x].get(np.uint32, x), got[x], f"{x}, workspace refilled with {twice:#x}")
        if "desc_out" in got:
            got["desc_out"] = got["desc_out"].reshape(n, 3)
        same(dq.get(np.uint8, "queue"), queue, "queue[] after the call")
        if di:
            same(di.get(np.uint32, "desc_in"), np.asarray(desc).reshape(-1), "desc_in after the call")
        if dw:
            dw.get(np.uint8, "work")
    finally:
        for x in (*mem.values(), dq, di, dw):
            if x:
                x.free()
    return got, kern


def judge(got, queue, qn, desc, what):
    qoff, perm, slot, dout = steerref.expect(queue, qn, desc)
    exp = {"qoff": qoff, "perm": perm, "slot": slot, "desc_out": dout}
    for x in got:
        same(got[x], exp[x], f"{x}, {what}")


def kernel_of(n, qn, names):
    """The kernel a call reports last."""
    outs = ", ".join(tf(x in names) for x in ("perm", "slot", "desc_out"))
    if cgck.steer_plan(n, qn)[1] <= 1:
        return f"steer_one_kernel<{outs}>"
    return f"steer_scatter_kernel<{outs}>" if set(names) - {"qoff"} else "steer_scan_kernel"


def check(eng, queue, qn, rng, what, names=ALL, **kw):
    desc = descs(rng, len(queue)) if "desc_out" in names else None
    got, kern = steer(eng, queue, qn, desc, names, **kw)
    assert tuple(got) == tuple(names)
    assert kern == kernel_of(len(queue), qn, names), (what, kern)
    judge(got, queue, qn, desc, what)
    return got


def mixed_bytes(rng, n, qn):
    """Queue ids 0..qn-1, 0xFF and bytes at and above qn (qn itself, 200, 254)."""
    pool = np.concatenate((np.arange(qn), np.arange(qn), [0xFF, 0xFF, qn, 200, 254])).astype(np.uint8)
    return rng.choice(pool, n)


# -- 1. step and tile edges -----------------------------------------------------------

@pytest.mark.parametrize("size", list(SIZES))
def test_step_and_tile_edges(engine, size):
    T = tile(7)
    n = SIZES[size](T)
    rng = np.random.default_rng(1000 + n)
    check(engine, mixed_bytes(rng, n, 7), 7, rng, f"n {size} = {n}")


@pytest.mark.parametrize("qn", [1, 2, 8, 127, 128])
def test_queue_counts(engine, qn):
    n = 2 * tile(qn) + 65
    rng = np.random.default_rng(1100 + qn)
    check(engine, mixed_bytes(rng, n, qn), qn, rng, f"queue_num {qn}")
    check(engine, rng.integers(0, 256, n, dtype=np.uint8), qn, rng, f"queue_num {qn}, every byte value")


# -- 2. patterns ----------------------------------------------------------------------

def patterns(n, qn):
    k = np.arange(n)
    runs = (k // 64) % qn
    return {"one queue": np.full(n, 3), "all unsteered": np.full(n, 0xFF), "alternating": 1 + 4 * (k % 2),
            "ascending": k * (qn + 1) // n, "descending": (n - 1 - k) * (qn + 1) // n,
            "runs of 64": runs, "runs of 64 shifted by one": np.roll(runs, 1)}


@pytest.mark.parametrize("name", list(patterns(64, 8)))
def test_patterns(engine, name):
    rng = np.random.default_rng(1200)
    for n in (1000, 2 * tile(8) + 65):
        queue = patterns(n, 8)[name].astype(np.uint8)
        if name in ("ascending", "descending"):
            assert set(queue.tolist()) == set(range(9))          # the last ids are the unsteered bin's
        check(engine, queue, 8, rng, f"{name}, n {n}")


# -- 3. the scan's passes -------------------------------------------------------------

def test_scan_passes(engine):
    """tiles x 129 words are more than two passes of the scan workgroup."""
    rng = np.random.default_rng(1300)
    n = (2 * SCAN_PASS // 129 + 2) * tile(128) - 37
    T, tiles, work = cgck.steer_plan(n, 128)
    assert T == tile(128) and tiles * 129 > 2 * SCAN_PASS and work == 4 * tiles * 129 and n < 400_000
    queue = mixed_bytes(rng, n, 128)
    queue[n // 3:n // 2] = 5                   # columns of zeros in most bins
    check(engine, queue, 128, rng, f"{n} frames, 128 queues")
    check(engine, queue, 128, rng, "qoff alone", names=("qoff",))


# -- 4. the workspace -----------------------------------------------------------------

def test_dirty_workspace(engine):
    rng = np.random.default_rng(1400)
    n = 2 * tile(7) + 65
    check(engine, mixed_bytes(rng, n, 7), 7, rng, "workspace 0xA5, then 0x00", work_fill=0xA5, twice=0x00)
    check(engine, mixed_bytes(rng, n, 7), 7, rng, "workspace 0xFF", work_fill=0xFF)


# -- 5. output subsets, bounds, alignment, names --------------------------------------

@pytest.mark.parametrize("names", [("qoff",), ("perm",), ("slot",), ("desc_out",), ALL, ("qoff", "desc_out"),
                                   ("perm", "slot")])
def test_output_subsets(engine, names):
    rng = np.random.default_rng(1500 + len(names))
    for n in (300, tile(7) + 1):
        check(engine, mixed_bytes(rng, n, 7), 7, rng, f"outputs {names}, n {n}", names=names)


def test_descriptor_alignment(engine):
    """desc_in and desc_out one descriptor (12 bytes) past a 16-byte boundary."""
    rng = np.random.default_rng(1600)
    for n in (257, tile(7) + 1):
        check(engine, mixed_bytes(rng, n, 7), 7, rng, f"descriptors at +12, n {n}", shift=12)


def test_kernel_names(engine):
    rng = np.random.default_rng(1700)
    T = tile(8)
    for n in (1, 256, T):
        assert cgck.steer_work_bytes(n, 8) == 0
        queue = mixed_bytes(rng, n, 8)
        desc = descs(rng, n)
        got, kern = steer(engine, queue, 8, desc, null_work=True)
        assert kern == "steer_one_kernel<true, true, true>", kern
        judge(got, queue, 8, desc, f"n {n}, work NULL")
    queue = mixed_bytes(rng, T + 1, 8)
    desc = descs(rng, T + 1)
    assert cgck.steer_work_bytes(T + 1, 8) == 4 * 2 * 9
    got, kern = steer(engine, queue, 8, desc)
    assert kern == "steer_scatter_kernel<true, true, true>", kern
    judge(got, queue, 8, desc, "n T + 1")


# -- 6. hash and steer ----------------------------------------------------------------

@pytest.fixture(scope="module")
def key():
    return np.frombuffer(bytes.fromhex(load_golden("rss_frames.json")["key"]), np.uint8).copy()


SEED = np.arange(128, dtype=np.uint32) * 3 + 5        # qcount before the call: running counters


def fused(eng, key, batch, qn, hf=cgck.RSS_TCP | cgck.RSS_UDP):
    """cgck_rss_steer_desc over a host batch: the rss arrays, the steer arrays
    and the device buffers the end-to-end test goes on with (the caller frees)."""
    buf, desc = batch[0], batch[1]
    n = len(desc)
    d = Guarded(eng, buf.nbytes).put(buf)
    dd = Guarded(eng, 12 * n).put(desc)
    rss = {"hash": Guarded(eng, 4 * n, 0xEE), "kind": Guarded(eng, n, 0xEE), "queue": Guarded(eng, n, 0xEE),
           "qcount": Guarded(eng, 4 * 128).put(SEED)}
    st = {"qoff": Guarded(eng, 4 * (qn + 2), 0xEE), "perm": Guarded(eng, 4 * n, 0xEE),
          "slot": Guarded(eng, 4 * n, 0xEE), "desc_out": Guarded(eng, 12 * n, 0xEE)}
    assert cgck.steer_work_bytes(n, qn) == 0
    eng.rss_steer_desc(d.ptr, dd.ptr, n, cgck.Engine.rss_spec(key, 0xFFFFFFFF, hf, qn), rss["queue"].ptr,
                       hash=rss["hash"].ptr, kind=rss["kind"].ptr, qcount=rss["qcount"].ptr,
                       **{x: st[x].ptr for x in st})
    assert eng.last_kernel == "steer_one_kernel<true, true, true>", eng.last_kernel
    got = {x: rss[x].get(np.uint32 if x in ("hash", "qcount") else np.uint8, x) for x in rss}
    got.update({x: st[x].get(np.uint32, x) for x in st})
    got["desc_out"] = got["desc_out"].reshape(n, 3)
    same(d.get(np.uint8, "frames"), buf, "the frame bytes after the call")
    same(dd.get(np.uint8, "desc"), desc.view(np.uint8), "the descriptors after the call")
    return got, (d, dd, *rss.values(), *st.values()), st


@pytest.mark.parametrize("frames", ["classes", "fuzz"])
def test_fused(engine, port, key, frames):
    rng = np.random.default_rng(1800 + len(frames))
    fr = RB.all_classes(rng) if frames == "classes" else RB.fuzz(rng, 300)
    qn, hf = 8, cgck.RSS_TCP | cgck.RSS_UDP
    for batch in (RB.packed(rng, fr, 3), RB.slotted(rng, fr, 2048, 14)):
        buf, desc, offs, lens = batch
        h, kind, queue = rssref.expect(port, buf, offs, lens, key, hf, queue_num=qn)
        assert np.count_nonzero(queue == rssref.NO_QUEUE) > 0 and len(set(queue.tolist())) == qn + 1
        got, bufs, _ = fused(engine, key, batch, qn, hf)
        try:
            same(got["hash"], h, f"hash, {frames}")
            same(got["kind"], kind, f"kind, {frames}")
            same(got["queue"], queue, f"queue, {frames}")
            judge({x: got[x] for x in ALL}, queue, qn, desc.view(np.uint32).reshape(-1, 3), f"steer, {frames}")
            same(got["qcount"][:qn] - SEED[:qn], np.diff(got["qoff"])[:qn], f"qcount deltas, {frames}")
            same(got["qcount"][qn:], SEED[qn:], f"qcount past queue_num, {frames}")
        finally:
            for x in bufs:
                x.free()


def test_end_to_end(engine, port, key):
    """Hash and steer a dual-stack burst, verify each bin's slice of desc_out with
    CGCK_VERIFY_TOY | CGCK_MIXED, and read the results back through perm."""
    rng = np.random.default_rng(1900)
    qn, flags = 8, cgck.VERIFY_TOY | cgck.MIXED
    batch = RB.packed(rng, RB.fuzz(rng, 500), 5)
    buf, desc, offs, lens = batch
    n = len(desc)
    eout, ever = mixedref.expect(port, buf, offs, lens, flags)
    assert len(set(ever.tolist())) > 2
    queue = rssref.expect(port, buf, offs, lens, key, cgck.RSS_TCP | cgck.RSS_UDP, queue_num=qn)[2]
    qoff, perm, slot, _ = steerref.expect(queue, qn)
    got, bufs, st = fused(engine, key, batch, qn)
    o, v = Guarded(engine, 4 * n, 0xEE), Guarded(engine, n, 0xEE)
    try:
        same(got["qoff"], qoff, "qoff")
        same(got["perm"], perm, "perm")
        for q in range(qn + 1):                     # the queues, then the unsteered frames
            lo, cnt = int(got["qoff"][q]), int(got["qoff"][q + 1] - got["qoff"][q])
            assert cnt > 0, "the burst fills every bin"
            engine.desc(bufs[0].ptr, st["desc_out"].ptr + 12 * lo, cnt, flags, o.ptr + 4 * lo, v.ptr + lo)
            assert engine.last_kernel.startswith("lpwx_kernel<"), engine.last_kernel
        out, ver = o.get(np.uint32, "out"), v.get(np.uint8, "verdict")
        same(out, eout[perm], "out in slot order")
        same(ver, ever[perm], "verdict in slot order")
        same(out[slot], eout, "out carried back to arrival order by slot[]")
        same(ver[got["slot"]], ever, "verdict carried back to arrival order by slot[]")
    finally:
        for x in (*bufs, o, v):
            x.free()


# -- 7. arguments ---------------------------------------------------------------------

def test_arguments(engine, key):
    L = cgck.load()
    rng = np.random.default_rng(2000)
    T = tile(8)
    n = 64
    queue = mixed_bytes(rng, n, 8)
    buf = np.zeros(64 * n, np.uint8)
    buf[::64] = 0x45
    desc = np.zeros(n, cgck.DESC_DTYPE)
    desc["frame_off"] = np.arange(n) * 64
    desc["ip_len"] = 64
    dq, dd, db = Guarded(engine, n).put(queue), Guarded(engine, 12 * n).put(desc), Guarded(engine, buf.nbytes).put(buf)
    o = Guarded(engine, 4096, 0xEE)
    w = Guarded(engine, 4096)
    ctx, by = engine.ctx, ctypes.byref
    R, S = cgck.RssRes, cgck.SteerRes
    spec = cgck.Engine.rss_spec(key, queue_num=8)
    res = S(o.ptr, None, None, None)
    full = S(o.ptr, o.ptr + 256, o.ptr + 1024, o.ptr + 2048)
    rss = R(None, None, dq.ptr, None)

    def steer_rc(c=ctx, q=dq.ptr, cnt=n, qn=8, din=dd.ptr, rs=res, work=None):
        return L.cgck_steer(c, q, cnt, qn, din, None if rs is None else by(rs), work, None)

    def fused_rc(c=ctx, base=db.ptr, dsc=dd.ptr, cnt=n, sp=spec, rr=rss, rs=res, work=None):
        return L.cgck_rss_steer_desc(c, base, dsc, cnt, None if sp is None else by(sp),
                                     None if rr is None else by(rr), None if rs is None else by(rs), work, None)

    try:
        for what, rc in (
                ("NULL ctx", steer_rc(c=None)),
                ("NULL queue", steer_rc(q=None)),
                ("NULL res", steer_rc(rs=None)),
                ("every output NULL", steer_rc(rs=S(None, None, None, None))),
                ("queue_num 0", steer_rc(qn=0)),
                ("queue_num 129", steer_rc(qn=129)),
                ("n 2^32", steer_rc(cnt=2 ** 32, work=w.ptr)),
                ("desc_out without desc_in", steer_rc(din=None, rs=full)),
                ("desc_out == desc_in", steer_rc(rs=S(None, None, None, dd.ptr))),
                ("desc_in misaligned", steer_rc(din=dd.ptr + 2, rs=full)),
                ("desc_out misaligned", steer_rc(rs=S(None, None, None, o.ptr + 2))),
                ("work NULL, two tiles", steer_rc(cnt=T + 1)),
                ("fused: NULL ctx", fused_rc(c=None)),
                ("fused: NULL base", fused_rc(base=None)),
                ("fused: NULL desc", fused_rc(dsc=None)),
                ("fused: NULL spec", fused_rc(sp=None)),
                ("fused: NULL rss", fused_rc(rr=None)),
                ("fused: NULL res", fused_rc(rs=None)),
                ("fused: NULL key", fused_rc(sp=cgck.RssSpec(None, 40, 0xFFFFFFFF, 0, 8))),
                ("fused: unknown hf", fused_rc(sp=cgck.Engine.rss_spec(key, hf=4, queue_num=8))),
                ("fused: NULL rss->queue", fused_rc(rr=R(o.ptr, None, None, None))),
                ("fused: queue_num 0", fused_rc(sp=cgck.Engine.rss_spec(key, queue_num=0))),
                ("fused: queue_num 0, no queue", fused_rc(sp=cgck.Engine.rss_spec(key, queue_num=0),
                                                          rr=R(o.ptr, None, None, None))),
                ("fused: queue_num 129", fused_rc(sp=cgck.Engine.rss_spec(key, queue_num=129))),
                ("fused: every steer output NULL", fused_rc(rs=S(None, None, None, None))),
                ("fused: desc_out == desc", fused_rc(rs=S(None, None, None, dd.ptr))),
                ("fused: desc_out misaligned", fused_rc(rs=S(None, None, None, o.ptr + 2))),
                ("fused: n 2^32", fused_rc(cnt=2 ** 32, work=w.ptr)),
                ("fused: work NULL, two tiles", fused_rc(cnt=T + 1))):
            assert rc == EINVAL, (what, rc)
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        engine.strided(db.ptr, n, 64, 0, 64, cgck.GEN_BOTH, w.ptr)
        engine.sync()
        before = engine.last_kernel
        assert not before.startswith("steer_")
        assert steer_rc(cnt=0, rs=full) == 0 and steer_rc(cnt=0, din=None) == 0
        assert fused_rc(cnt=0, rs=full) == 0 and fused_rc(cnt=0, dsc=None) == 0
        engine.sync()
        assert engine.last_kernel == before
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after n == 0")
        same(dq.get(np.uint8, "queue"), queue, "queue[] after n == 0")
        # the same arguments with n > 0 are accepted
        assert steer_rc(rs=full) == 0
        assert engine.last_kernel.startswith(ONE)
        got = o.get(np.uint32, "outputs")
        same(got[:10], steerref.expect(queue, 8)[0], "qoff")
        same(got[64:64 + n], steerref.expect(queue, 8)[1], "perm")
    finally:
        for x in (dq, dd, db, o, w):
            x.free()
