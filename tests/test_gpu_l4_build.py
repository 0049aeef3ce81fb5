"""cgck_l4_build (l4b_kernel, cgck_l4b.hip).  Every output of every call and the
whole frame buffer are compared with the referee (tests/l4bref.py), never with the
library itself, by exact equality.  Every array lies between canary bytes that must
survive, the inputs are read back unchanged, and the frame buffer is a plain
allocation of exactly the burst's bytes, so a frame that ends the burst ends the
allocation."""
import ctypes
import itertools
import socket

import numpy as np
import pytest

import cgck
import l4bbatches as LB
import l4bref as R
import l4ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("raw_out", "desc_out", "cls_out", "count")
CAN, CANARY = 64, 0xC3
NC = 12                                                 # counters allocated: 8 and four that stay untouched
SEED = (np.arange(NC, dtype=np.uint32) * 7 + 3)         # count[] before a call: running counters
DTYPES = {"raw_out": np.uint8, "desc_out": np.uint8, "cls_out": np.uint8, "count": np.uint32}


@pytest.fixture(scope="module", autouse=True, params=[cgck.L4B_STORE_DIRECT, cgck.L4B_STORE_TURNED], ids=["direct", "turned"])
def store(request):
    """Every test of this file runs under both store shapes of l4b_kernel."""
    before = cgck.l4_build_store(request.param)
    yield request.param
    assert cgck.l4_build_store(before) == request.param


def kernel_of(names, store):
    d, x = bool({"raw_out", "desc_out"} & set(names)), bool({"cls_out", "count"} & set(names))
    return "l4b_kernel<%s, %s, %s>" % (("false", "true")[d], ("false", "true")[x], ("false", "true")[store == cgck.L4B_STORE_TURNED])


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
        assert self.buf.ptr % 16 == 0
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
        self.eng, self.n = eng, len(buf)
        self.buf = cgck.DeviceBuffer(max(buf.nbytes, 1))
        assert self.buf.ptr % 16 == 0
        self.buf.upload(buf, stream=eng.stream)
        self.ptr = self.buf.ptr

    def get(self):
        after = np.zeros(self.n, np.uint8)
        self.buf.download(after, stream=self.eng.stream)
        self.eng.sync()
        return after

    def free(self):
        self.buf.free()


def build(eng, buf, slot, seg, flow, cls=None, fidx=None, names=ALL, ip_id0=0, ip_off=0x4000, calls=1, shift=0,
          res=True):
    """cgck_l4_build over host arrays, `calls` times: ({name: array, "buf": the frame
    bytes after}, kernel name).  raw_out, desc_out and cls_out start as 0xEE bytes,
    count as SEED; slot, raw_out and desc_out lie `shift` bytes past a 16-byte
    boundary.  res False: a NULL res."""
    n = len(slot)
    fr = Frames(eng, buf)
    ins = {"slot": Guarded(eng, 12 * n, shift=shift).put(slot), "seg": Guarded(eng, 32 * n).put(seg),
           "flow": Guarded(eng, 48 * len(flow)).put(flow)}
    if cls is not None:
        ins["cls"] = Guarded(eng, n, shift=1).put(cls)
    if fidx is not None:
        ins["fidx"] = Guarded(eng, 4 * n, shift=4).put(fidx)
    sizes = {"raw_out": 12 * n, "desc_out": 12 * n, "cls_out": n, "count": 4 * NC}
    mem = {x: Guarded(eng, sizes[x], 0xEE, shift=shift if x.endswith("_out") and x != "cls_out" else 0) for x in names}
    if "count" in mem:
        mem["count"].put(SEED)
    try:
        for _ in range(calls):
            if res:
                eng.l4_build(fr.ptr, n, ins["slot"].ptr, ins["seg"].ptr, ins["flow"].ptr, len(flow),
                             cls=ins["cls"].ptr if "cls" in ins else None, fidx=ins["fidx"].ptr if "fidx" in ins else None,
                             ip_id0=ip_id0, ip_off=ip_off, **{x: mem[x].ptr for x in names})
            else:
                arg = cgck.L4BuildIn(ins["slot"].ptr, ins["seg"].ptr, ins["cls"].ptr if "cls" in ins else None,
                                     ins["flow"].ptr, ins["fidx"].ptr if "fidx" in ins else None, len(flow), ip_id0, ip_off)
                assert cgck.load().cgck_l4_build(eng.ctx, fr.ptr, n, ctypes.byref(arg), None, None) == 0
        kern = eng.last_kernel
        got = {x: mem[x].get(DTYPES[x], x) for x in names}
        got["buf"] = fr.get()
        for x, a in (("slot", slot), ("seg", seg), ("flow", flow), ("cls", cls), ("fidx", fidx)):
            if x in ins:
                same(ins[x].get(np.uint8, x), np.ascontiguousarray(a).view(np.uint8).reshape(-1), f"{x}[] after the call")
    finally:
        for x in (fr, *ins.values(), *mem.values()):
            x.free()
    return got, kern


def judge(got, exp, ebuf, what, calls=1):
    eraw, edesc, ecls, ecount = exp
    same(got["buf"], ebuf, f"frame bytes, {what}")
    for x in got:
        if x == "raw_out":
            same(got[x], eraw.view(np.uint8), f"raw_out, {what}")
        elif x == "desc_out":
            same(got[x], edesc.view(np.uint8), f"desc_out, {what}")
        elif x == "cls_out":
            same(got[x], ecls, f"cls, {what}")
        elif x == "count":
            want = SEED.copy()
            want[:R.NCOUNT] += np.uint32(calls) * ecount
            same(got[x], want, f"count after {calls} call(s), {what}")


@pytest.fixture(scope="module")
def corpus():
    return LB.Corpus(np.random.default_rng(41))


@pytest.fixture(scope="module")
def tiled700(corpus):
    buf, slot, cls, fidx, seg = LB.tiled(corpus, 700)
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, seg, corpus.flow, cls, fidx, 0xFF00, 0x4000)
    return (buf, slot, cls, fidx, seg), exp, ebuf


# -- 1. the class corpus at every start alignment ---------------------------------------

@pytest.mark.parametrize("align", range(16))
def test_classes_every_alignment(engine, corpus, align, store):
    C = corpus
    buf, slot = LB.lay(C, align)
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, C.seg, C.flow, C.cls, C.fidx, 0xFFC0 + align, 0x4000 if align % 2 else 0)
    assert {int(c) & 15 for c in exp[2]} == set(range(R.NCLASS)) and np.all(exp[3] > 0)
    got, kern = build(engine, buf, slot, C.seg, C.flow, C.cls, C.fidx, ip_id0=0xFFC0 + align,
                      ip_off=0x4000 if align % 2 else 0, shift=4 * (align % 4))
    assert kern == kernel_of(ALL, store), kern
    judge(got, exp, ebuf, f"alignment {align}")


# -- 2. frames packed back to back: neighbours share dwords -----------------------------

@pytest.mark.parametrize("start", [3, 6])
def test_packed_back_to_back(engine, corpus, start):
    """cap == L from `start` on (an odd start gives every odd frame alignment, an
    even one every even): no byte of a neighbour may be touched or lost."""
    buf, slot, cls, fidx, seg = LB.packed(corpus, start)
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, seg, corpus.flow, cls, fidx, 5, 0x4000)
    assert np.all((exp[2] & 15) <= R.UDP) and np.array_equal(exp[0]["ip_len"], slot["ip_len"])
    got, _ = build(engine, buf, slot, seg, corpus.flow, cls, fidx, ip_id0=5)
    judge(got, exp, ebuf, f"packed from byte {start}")


# -- 3. outputs --------------------------------------------------------------------------

@pytest.mark.parametrize("names", [c for r in (0, 1, 2, 3, 4) for c in itertools.combinations(ALL, r)],
                         ids=lambda c: "+".join(c) or "none")
def test_outputs(engine, corpus, tiled700, names, store):
    """Every subset of the outputs, none included; the counters after two calls (+=),
    with the four words past them untouched."""
    (buf, slot, cls, fidx, seg), exp, ebuf = tiled700
    got, kern = build(engine, buf, slot, seg, corpus.flow, cls, fidx, names, ip_id0=0xFF00, calls=2)
    assert tuple(x for x in got if x != "buf") == names and kern == kernel_of(names, store), kern
    judge(got, exp, ebuf, f"outputs {names}", calls=2)
    if "count" in got:
        assert np.all(exp[3] > 0)
        same(got["count"][R.NCOUNT:], SEED[R.NCOUNT:], "count[8..]")


def test_null_res(engine, corpus, tiled700, store):
    (buf, slot, cls, fidx, seg), exp, ebuf = tiled700
    got, kern = build(engine, buf, slot, seg, corpus.flow, cls, fidx, (), ip_id0=0xFF00, res=False)
    assert kern == kernel_of((), store), kern
    judge(got, exp, ebuf, "NULL res")


# -- 4. burst sizes ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_tails(engine, corpus, n, store):
    buf, slot, cls, fidx, seg = LB.tiled(corpus, n)
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, seg, corpus.flow, cls, fidx, n, 0)
    got, kern = build(engine, buf, slot, seg, corpus.flow, cls, fidx, ip_id0=n, ip_off=0)
    assert kern == kernel_of(ALL, store), kern
    judge(got, exp, ebuf, f"n {n}")


def test_product_shape(engine, corpus, store):
    """With nothing pinned the call runs the product's shape, one of the two."""
    buf, slot, cls, fidx, seg = LB.tiled(corpus, 321)
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, seg, corpus.flow, cls, fidx, 7, 0x4000)
    assert cgck.l4_build_store(cgck.L4B_STORE_DEFAULT) == store
    try:
        got, kern = build(engine, buf, slot, seg, corpus.flow, cls, fidx, ip_id0=7)
    finally:
        assert cgck.l4_build_store(store) == cgck.L4B_STORE_DEFAULT
    assert kern in (kernel_of(ALL, cgck.L4B_STORE_DIRECT), kernel_of(ALL, cgck.L4B_STORE_TURNED)), kern
    judge(got, exp, ebuf, "the product's shape")


def test_three_passes(engine, corpus, store):
    """Above twice what one pass of the grid covers, plus a step and a frame: every
    wave runs three steps.  The burst is a piece repeated; the expectation is the
    piece's, with the ids of each repeat (LB.with_ids)."""
    C = corpus
    per_pass = engine.l4_build_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024
    n = 2 * per_pass + 65
    assert n * 128 < 128_000_000
    piece = 3 * C.m * 8                                 # whole periods of the tiled layout, half a MiB of frames
    buf, sp, cls, fidx, seg = LB.tiled(C, piece)
    ebuf = buf.copy()
    eraw, edesc, ecls, _ = R.build(ebuf, sp, seg, C.flow, cls, fidx, 0, 0x4000)
    reps = -(-n // piece)
    id0 = 0xFFF0
    fr = Frames(engine, np.tile(buf, reps)[:n * 128])
    L, st = cgck.load(), engine.stream
    sizes = {"slot": 12 * n, "seg": 32 * n, "cls": n, "fidx": 4 * n, "raw_out": 12 * n, "desc_out": 12 * n, "cls_out": n,
             "count": 4 * NC}
    dev = {x: cgck.DeviceBuffer(2 * CAN + sz) for x, sz in sizes.items()}
    flow = Guarded(engine, 48 * LB.NFLOW).put(C.flow)
    try:
        for x, d in dev.items():
            assert L.cgck_memset(d.ptr, CANARY, 2 * CAN + sizes[x], st) == 0
            assert L.cgck_memset(d.ptr + CAN, 0xEE, sizes[x], st) == 0
        dev["count"].upload(SEED, off=CAN, stream=st)
        for a in range(0, n, piece):
            k = min(piece, n - a)
            d = sp[:k].copy()
            d["frame_off"] += np.uint64(128 * a)
            dev["slot"].upload(d, off=CAN + 12 * a, stream=st)
            dev["seg"].upload(seg[:k], off=CAN + 32 * a, stream=st)
            dev["cls"].upload(cls[:k], off=CAN + a, stream=st)
            dev["fidx"].upload(fidx[:k], off=CAN + 4 * a, stream=st)
        engine.sync()
        engine.l4_build(fr.ptr, n, dev["slot"].ptr + CAN, dev["seg"].ptr + CAN, flow.ptr, LB.NFLOW, cls=dev["cls"].ptr + CAN,
                        fidx=dev["fidx"].ptr + CAN, ip_id0=id0, ip_off=0x4000,
                        **{x: dev[x].ptr + CAN for x in ALL})
        assert engine.last_kernel == kernel_of(ALL, store), engine.last_kernel

        def fetch(x, off, count, dtype):
            got = np.zeros(count, dtype)
            dev[x].download(got, off=off, stream=st)
            engine.sync()
            return got

        after = fr.get()
        total = np.zeros(R.NCOUNT, np.uint64)
        for a in range(0, n, piece):
            k = min(piece, n - a)
            want = LB.with_ids(ebuf, edesc, ecls, id0 + a)
            same(after[128 * a:128 * (a + k)], want[:128 * k], f"frame bytes, frames {a} ..")
            for x, e in (("raw_out", eraw), ("desc_out", edesc)):
                d = e[:k].copy()
                d["frame_off"] += np.uint64(128 * a)
                same(fetch(x, CAN + 12 * a, 12 * k, np.uint8), d.view(np.uint8), f"{x}, frames {a} ..")
            same(fetch("cls_out", CAN + a, k, np.uint8), ecls[:k], f"cls, frames {a} ..")
            total += R.counts(ecls[:k])
        want = SEED.copy()
        want[:R.NCOUNT] += total.astype(np.uint32)
        same(fetch("count", CAN, NC, np.uint32), want, "count")
        for x, d in dev.items():
            for off in (0, CAN + sizes[x]):
                assert np.all(fetch(x, off, CAN, np.uint8) == CANARY), f"{x}: bytes outside the array were written"
        flow.get(np.uint8, "flow")
    finally:
        for d in (fr, flow, *dev.values()):
            d.free()


# -- 5. the NULL forms of cls and fidx ---------------------------------------------------

def test_cls_and_fidx_forms(engine, corpus):
    """cls NULL (every frame TCP) and fidx NULL (frame k uses flow[k]); every frame on
    one flow; a random permutation of per-frame flows."""
    C = corpus
    rng = np.random.default_rng(43)
    n = 300
    buf, slot, _, _, _ = LB.tiled(C, n)
    slot["ip_len"] = 120                                # room for every header here and its 9 bytes
    seg = np.array([LB.seg(rng, opt=int(k) % 8, th_flags=LB.SYN, pay_len=(0, 0, 9)[int(k) % 3]) for k in range(n)], R.SEG_DTYPE)
    cls = np.array([(R.SEG_TCP, R.SEG_UDP, R.SEG_TCP, 7)[k % 4] for k in range(n)], np.uint8)
    flow = C.flow[np.array(LB.GOOD)[rng.integers(0, 4, n)]].copy()
    flow["laddr"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.uint32)
    for what, c, f, fl in (("cls NULL, fidx NULL", None, None, flow), ("fidx NULL", cls, None, flow),
                           ("cls NULL", None, perm, flow), ("one flow", cls, np.full(n, 2, np.uint32), flow[:3]),
                           ("a permutation", cls, perm, flow), ("fidx NULL, nflow below n", cls, None, flow[:n - 70])):
        ebuf = buf.copy()
        exp = R.build(ebuf, slot, seg, fl, c, f, 1, 0x4000)
        assert (exp[3][R.BADFLOW] > 0) == (what == "fidx NULL, nflow below n")
        got, _ = build(engine, buf, slot, seg, fl, c, f, ip_id0=1)
        judge(got, exp, ebuf, what)


# -- 6. composition ----------------------------------------------------------------------

def test_build_fill_l2_verify_l4(engine, corpus):
    """cgck_l4_build -> cgck_desc(... | CGCK_STORE) over the frames with payload, per
    family -> cgck_l2_desc over raw_out -> cgck_desc(VERIFY_TOY | MIXED) and
    cgck_l4_desc over its descriptors: the descriptors are desc_out, every verdict is
    0 and the records are the ones that went in."""
    C = corpus
    rng = np.random.default_rng(44)
    n, stride = 300, 2048
    fidx = np.array([(LB.V4T if k % 5 == 0 else LB.V4) + (k % 3 == 1) for k in range(n)], np.uint32)      # V6 = V4 + 1, V6T = V4T + 1
    cls = np.array([R.SEG_UDP if k % 4 == 3 else R.SEG_TCP for k in range(n)], np.uint8)
    seg = np.array([LB.seg(rng, opt=k % 8 if cls[k] == R.SEG_TCP else 0, th_flags=LB.SYN | (LB.ACK if k % 2 else 0),
                           pay_len=(0, 0, 1, 700, 1401)[k % 5]) for k in range(n)], R.SEG_DTYPE)
    slot = np.zeros(n, R.DESC_DTYPE)
    slot["frame_off"], slot["l3_off"], slot["ip_len"] = np.arange(n) * stride, np.arange(n) % 4, 1600
    buf = rng.integers(0, 256, n * stride, dtype=np.uint8)
    ebuf = buf.copy()
    eraw, edesc, ecls, _ = R.build(ebuf, slot, seg, C.flow, cls, fidx, 77, 0x4000)
    assert np.all((ecls & 15) <= R.UDP) and {int(c) >> 4 for c in ecls} == {0, 1, 2, 3}
    R.fill(ebuf, edesc, ecls)

    fr = Frames(engine, buf)
    ins = [Guarded(engine, 12 * n).put(slot), Guarded(engine, 32 * n).put(seg), Guarded(engine, 48 * LB.NFLOW).put(C.flow),
           Guarded(engine, n).put(cls), Guarded(engine, 4 * n).put(fidx)]
    raw, desc, d1 = (Guarded(engine, 12 * n, 0xEE) for _ in range(3))
    co, ver, out = Guarded(engine, n, 0xEE), Guarded(engine, n, 0xEE), Guarded(engine, 4 * n, 0xEE)
    sg, c4 = Guarded(engine, 32 * n, 0xEE), Guarded(engine, n, 0xEE)
    subs = []
    try:
        engine.l4_build(fr.ptr, n, ins[0].ptr, ins[1].ptr, ins[2].ptr, LB.NFLOW, cls=ins[3].ptr, fidx=ins[4].ptr, ip_id0=77,
                        ip_off=0x4000, raw_out=raw.ptr, desc_out=desc.ptr, cls_out=co.ptr)
        gdesc, gcls = desc.get(R.DESC_DTYPE, "desc_out"), co.get(np.uint8, "cls")
        same(gdesc.view(np.uint8), edesc.view(np.uint8), "desc_out")
        same(gcls, ecls, "cls")
        for six in (0, cgck.IP6):                       # the fill: the frames with payload, per family
            sel = ((gcls & R.PAYLOAD) != 0) & (((gcls & R.IP6) != 0) == bool(six))
            m = int(np.count_nonzero(sel))
            assert m > 30
            sd, so = Guarded(engine, 12 * m).put(gdesc[sel]), Guarded(engine, 4 * m, 0xEE)
            subs += [sd, so]
            engine.desc(fr.ptr, sd.ptr, m, cgck.L4 | cgck.ZERO_FIELDS | cgck.STORE | six, so.ptr)
        engine.l2_desc(fr.ptr, raw.ptr, n, desc_out=d1.ptr)
        engine.desc(fr.ptr, d1.ptr, n, cgck.VERIFY_TOY | cgck.MIXED, out.ptr, ver.ptr)
        engine.l4_desc(fr.ptr, d1.ptr, n, seg=sg.ptr, cls=c4.ptr)
        same(fr.get(), ebuf, "frame bytes after build and fill")
        same(raw.get(np.uint8, "raw_out"), eraw.view(np.uint8), "raw_out")
        same(d1.get(np.uint8, "l2_desc's descriptors"), edesc.view(np.uint8), "cgck_l2_desc(raw_out) against desc_out")
        same(ver.get(np.uint8, "verdict"), np.zeros(n, np.uint8), "verdicts")
        eseg, ec4, _, _ = l4ref.expect(ebuf, edesc)
        same(c4.get(np.uint8, "l4 cls"), ec4, "cgck_l4_desc's classes")
        gs = sg.get(l4ref.SEG_DTYPE, "seg")
        same(gs.view(np.uint8), eseg.view(np.uint8), "cgck_l4_desc's records against its referee")
        tcp = cls == R.SEG_TCP
        for f in ("sport", "dport", "pay_len"):
            same(gs[f], seg[f], f"seg.{f} read back")
        for f in ("seq", "ack", "win", "th_flags", "opt"):
            same(gs[f][tcp], seg[f][tcp], f"seg.{f} read back")
        for f, bit in (("mss", R.MSS), ("wscale", R.WS), ("ts_val", R.TS), ("ts_ecr", R.TS)):
            on = tcp & ((seg["opt"] & bit) != 0)
            same(gs[f][on], seg[f][on], f"seg.{f} read back")
        for x in ins:
            x.get(np.uint8, "an input")
    finally:
        for x in (fr, *ins, raw, desc, d1, co, ver, out, sg, c4, *subs):
            x.free()


# -- 7. a SYN burst from a dst-cache build, and the hash of its replies ------------------

def test_syn_burst_from_dst_cache(engine):
    key = np.frombuffer(bytes.fromhex(load_golden("rss.json")["keys"]["freebsd"]), np.uint8).copy()
    ent = engine.dst_cache_host(cgck.Engine.dst_params((0x0A000001, 0x0A000003), (0x0A010001, 0x0A010002),
                                                       socket.htons(80), 4, 1, key), 300)
    n = len(ent)
    assert n > 100
    rng = np.random.default_rng(45)
    raw = ent.view(np.uint8).reshape(n, 16)
    out_flow, in_flow = np.zeros(n, R.FLOW_DTYPE), np.zeros(n, R.FLOW_DTYPE)
    for f, a, b, src, dst in ((out_flow, 0, 4, (2, 0, 0, 0, 0, 2), (2, 0, 0, 0, 0, 1)), (in_flow, 4, 0, (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2))):
        f["eth_dst"], f["eth_src"], f["ttl"] = dst, src, 64
        f["laddr"][:, :4], f["faddr"][:, :4] = raw[:, a:a + 4], raw[:, b:b + 4]
    syn = np.zeros(n, R.SEG_DTYPE)                      # tcp_output.c:255-302: a SYN carries MSS, WS and timestamps
    syn["sport"], syn["dport"], syn["seq"] = ent["lport"], ent["fport"], rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    syn["th_flags"], syn["win"], syn["opt"], syn["mss"], syn["wscale"] = LB.SYN, 0xFFFF, 7, 1460, 7
    syn["ts_val"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    rep = syn.copy()                                    # the peer's SYN | ACK: addresses and ports swapped
    rep["sport"], rep["dport"], rep["ack"], rep["th_flags"] = syn["dport"], syn["sport"], syn["seq"] + np.uint32(1), LB.SYN | LB.ACK
    rep["ts_ecr"] = syn["ts_val"]
    slot = np.zeros(n, R.DESC_DTYPE)
    slot["frame_off"], slot["ip_len"] = np.arange(n) * 128, 128
    for what, seg, flow in (("SYNs", syn, out_flow), ("replies", rep, in_flow)):
        buf = np.full(n * 128, LB.POISON, np.uint8)
        ebuf = buf.copy()
        exp = R.build(ebuf, slot, seg, flow, None, None, 0xFF80, 0x4000)
        assert np.all(exp[2] == R.TCP) and np.all(exp[0]["ip_len"] == 14 + 20 + 40)
        got, _ = build(engine, buf, slot, seg, flow, ip_id0=0xFF80)
        judge(got, exp, ebuf, what)
    # cgck_l4_desc over the replies the library built: the hash is the entry's own
    fr = Frames(engine, got["buf"])
    dd, hh, cc = Guarded(engine, 12 * n).put(got["desc_out"]), Guarded(engine, 4 * n, 0xEE), Guarded(engine, n, 0xEE)
    try:
        engine.l4_desc(fr.ptr, dd.ptr, n, hash=hh.ptr, cls=cc.ptr)
        same(hh.get(np.uint32, "hash"), ent["hash"], "hash of the replies against the entries' SO_HASH")
        same(cc.get(np.uint8, "cls"), np.full(n, l4ref.TCP, np.uint8), "cls of the replies")
    finally:
        for x in (fr, dd, hh, cc):
            x.free()


# -- 8. arguments ------------------------------------------------------------------------

def test_arguments(engine, corpus, tiled700, store):
    L = cgck.load()
    C = corpus
    n = 64
    (buf, slot, cls, fidx, seg), _, _ = tiled700
    buf, slot, cls, fidx, seg = buf[:n * 128], slot[:n], cls[:n], fidx[:n], seg[:n]
    ebuf = buf.copy()
    exp = R.build(ebuf, slot, seg, C.flow, cls, fidx, 3, 0xFFFF)
    fr = Frames(engine, buf)
    sl, sg, fl = Guarded(engine, 12 * n).put(slot), Guarded(engine, 32 * n).put(seg), Guarded(engine, 48 * LB.NFLOW).put(C.flow)
    cl, fi = Guarded(engine, n).put(cls), Guarded(engine, 4 * n).put(fidx)
    o = Guarded(engine, 4096, 0xEE)
    ctx, by, I, O = engine.ctx, ctypes.byref, cgck.L4BuildIn, cgck.L4BuildRes
    assert o.ptr % 16 == 0 and sg.ptr % 16 == 0 and fl.ptr % 16 == 0
    full = O(o.ptr, o.ptr + 1024, o.ptr + 2048, o.ptr + 3072)

    def arg(slot=sl.ptr, seg=sg.ptr, flow=fl.ptr):
        return I(slot, seg, cl.ptr, flow, fi.ptr, LB.NFLOW, 3, 0xFFFF)     # every ip_off is legal

    def rc(c=ctx, base=fr.ptr, cnt=n, a=arg(), rs=full):
        return L.cgck_l4_build(c, base, cnt, None if a is None else by(a), None if rs is None else by(rs), None)

    try:
        for what, r in (("NULL ctx", rc(c=None)), ("NULL base", rc(base=None)), ("NULL in", rc(a=None)),
                        ("NULL slot", rc(a=arg(slot=None))), ("NULL seg", rc(a=arg(seg=None))), ("NULL flow", rc(a=arg(flow=None))),
                        ("slot misaligned", rc(a=arg(slot=sl.ptr + 2))), ("seg at +8", rc(a=arg(seg=sg.ptr + 8))),
                        ("seg at +4", rc(a=arg(seg=sg.ptr + 4))), ("flow at +8", rc(a=arg(flow=fl.ptr + 8))),
                        ("raw_out misaligned", rc(rs=O(o.ptr + 2, None, None, None))),
                        ("desc_out misaligned", rc(rs=O(None, o.ptr + 1, None, None))),
                        ("raw_out is slot", rc(rs=O(sl.ptr, o.ptr, None, None))),
                        ("desc_out is slot", rc(rs=O(o.ptr, sl.ptr, None, None))),
                        ("raw_out is desc_out", rc(rs=O(o.ptr, o.ptr, o.ptr + 2048, None))),
                        ("n == 0, NULL base", rc(cnt=0, base=None)), ("n == 0, seg misaligned", rc(cnt=0, a=arg(seg=sg.ptr + 8))),
                        ("n == 0, raw_out is desc_out", rc(cnt=0, rs=O(o.ptr, o.ptr, None, None)))):
            assert r == EINVAL, (what, r)
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after the refused calls")
        same(fr.get(), buf, "slots after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        engine.l4_desc(fr.ptr, sl.ptr, n, cls=o.ptr + 3584)
        engine.sync()
        before = engine.last_kernel
        assert not before.startswith("l4b_")
        assert rc(cnt=0) == 0 and rc(cnt=0, a=arg(slot=None, seg=None, flow=None)) == 0 and rc(cnt=0, rs=None) == 0
        engine.sync()
        assert engine.last_kernel == before
        same(o.get(np.uint8, "outputs")[:3584], np.full(3584, 0xEE, np.uint8), "outputs after n == 0")
        same(fr.get(), buf, "slots after n == 0")
        # the same arguments with n > 0 are accepted
        assert rc() == 0 and engine.last_kernel.startswith("l4b_kernel") and engine.last_kernel == kernel_of(ALL, store)
        got = o.get(np.uint8, "outputs")
        same(got[:12 * n], exp[0].view(np.uint8), "raw_out")
        same(got[1024:1024 + 12 * n], exp[1].view(np.uint8), "desc_out")
        same(got[2048:2048 + n], exp[2], "cls")
        same(got[3072:3072 + 4 * R.NCOUNT].view(np.uint32), np.uint32(0xEEEEEEEE) + exp[3], "count (running from 0xEEEEEEEE)")
        same(got[3072 + 4 * R.NCOUNT:3584], np.full(512 - 4 * R.NCOUNT, 0xEE, np.uint8), "the words past count[8)")
        same(fr.get(), ebuf, "frame bytes")
        for x, a in ((sl, slot), (sg, seg), (fl, C.flow), (cl, cls), (fi, fidx)):
            same(x.get(np.uint8, "an input"), np.ascontiguousarray(a).view(np.uint8).reshape(-1), "an input after the calls")
    finally:
        for x in (fr, sl, sg, fl, cl, fi, o):
            x.free()
