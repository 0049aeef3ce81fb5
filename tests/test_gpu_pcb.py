"""cgck_pcb_build and cgck_pcb_lookup (pcbb_kernel, pcbl_kernel: cgck_pcb.hip).  Every
output of every call is compared with the referee (tests/pcbref.py), never with the
library itself, by exact equality.  Every array, the table included, lies between
canary bytes that must survive and starts as 0xEE bytes, the inputs are read back
unchanged, and the frame buffer is a plain allocation of exactly the burst's bytes.
Every test runs under the four values of cgck_test_pcb_mode: the product's table,
every key chained from the table's last slot, and both again with 4-byte slots."""
import ctypes
import itertools

import numpy as np
import pytest

import cgck
import l4bref
import pcbbatches as PB
import pcbref as R

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("idx", "fidx", "kind", "count")
CAN, CANARY = 64, 0xC3
NC = 10                                                 # counters allocated: 6 and four that stay untouched
SEED = (np.arange(NC, dtype=np.uint32) * 5 + 2)         # count[] before a call: running counters
DTYPES = {"idx": np.uint32, "fidx": np.uint32, "kind": np.uint8, "count": np.uint32}


@pytest.fixture(scope="module", autouse=True, params=range(4), ids=["tag", "tag-chain", "idx", "idx-chain"])
def mode(request):
    m = (request.param & 1) | (cgck.PCB_MODE_UNTAGGED if request.param & 2 else 0)
    before = cgck.pcb_mode(m)
    yield m
    assert cgck.pcb_mode(before) == m


def kernel_of(names, mode):
    i, x = bool({"idx", "fidx"} & set(names)), bool({"kind", "count"} & set(names))
    return "pcbl_kernel<%s, %s, %s>" % (("false", "true")[i], ("false", "true")[x], ("true", "false")[bool(mode & 2)])


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
        self.buf = cgck.DeviceBuffer(max(buf.nbytes, 1))
        assert self.buf.ptr % 16 == 0
        self.buf.upload(np.ascontiguousarray(buf), stream=eng.stream)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free()


class DevTable:
    """A Table's arrays on the device and the cgck_pcb_t over them; the table's bytes
    start as `fill`."""

    def __init__(self, eng, t, use_bound=True, fill=0xEE):
        self.t, self.eng = t, eng
        self.bytes = cgck.pcb_table_bytes(len(t.conn))
        self.conn = Guarded(eng, 12 * len(t.conn), shift=4).put(t.conn)
        self.flow = Guarded(eng, 48 * len(t.flow)).put(t.flow)
        self.table = Guarded(eng, self.bytes, fill)
        self.bound = Guarded(eng, 4 * R.NBOUND, shift=8).put(t.bound) if use_bound and t.bound is not None else None
        self.pcb = cgck.Pcb(self.conn.ptr, len(t.conn), self.flow.ptr, len(t.flow), self.table.ptr, self.bytes,
                            self.bound.ptr if self.bound else None)

    def build(self, stat=True):
        """cgck_pcb_build; stat as the call wrote it over 0xEE bytes."""
        st = Guarded(self.eng, 16, 0xEE, shift=4) if stat else None
        try:
            self.eng.pcb_build(self.pcb, st.ptr if st else None)
            return st.get(np.uint32, "stat") if st else None
        finally:
            if st:
                st.free()

    def check(self):
        """The inputs unchanged, nothing written around the table."""
        same(self.conn.get(np.uint8, "conn"), self.t.conn.view(np.uint8).reshape(-1), "conn[] after the calls")
        same(self.flow.get(np.uint8, "flow"), self.t.flow.view(np.uint8).reshape(-1), "flow[] after the calls")
        self.table.get(np.uint8, "table")
        if self.bound:
            same(self.bound.get(np.uint32, "bound"), self.t.bound, "bound[] after the calls")

    def free(self):
        for x in (self.conn, self.flow, self.table, self.bound):
            if x:
                x.free()


def look(eng, dt, buf, desc, seg, cls, names=ALL, calls=1, shift=0):
    """cgck_pcb_lookup over host arrays, `calls` times: ({name: array}, kernel name).
    idx, fidx and kind start as 0xEE bytes, count as SEED; desc, idx and fidx lie
    `shift` bytes past a 16-byte boundary."""
    n = len(desc)
    fr = Frames(eng, buf)
    ins = {"desc": Guarded(eng, 12 * n, shift=shift).put(desc), "seg": Guarded(eng, 32 * n).put(seg)}
    if cls is not None:
        ins["cls"] = Guarded(eng, n, shift=1).put(cls)
    sizes = {"idx": 4 * n, "fidx": 4 * n, "kind": n, "count": 4 * NC}
    mem = {x: Guarded(eng, sizes[x], 0xEE, shift=shift if x in ("idx", "fidx") else 0) for x in names}
    if "count" in mem:
        mem["count"].put(SEED)
    try:
        for _ in range(calls):
            eng.pcb_lookup(fr.ptr, ins["desc"].ptr, ins["seg"].ptr, n, dt.pcb, cls=ins["cls"].ptr if "cls" in ins else None,
                           **{x: mem[x].ptr for x in names})
        kern = eng.last_kernel
        got = {x: mem[x].get(DTYPES[x], x) for x in names}
        for x, a in (("desc", desc), ("seg", seg), ("cls", cls)):
            if x in ins:
                same(ins[x].get(np.uint8, x), np.ascontiguousarray(a).view(np.uint8).reshape(-1), f"{x}[] after the call")
    finally:
        for x in (fr, *ins.values(), *mem.values()):
            x.free()
    return got, kern


def judge(got, exp, what, calls=1):
    eidx, efidx, ekind, ecount = exp
    for x in got:
        if x == "count":
            want = SEED.copy()
            want[:R.NCOUNT] += np.uint32(calls) * ecount
            same(got[x], want, f"count after {calls} call(s), {what}")
        else:
            same(got[x], {"idx": eidx, "fidx": efidx, "kind": ekind}[x], f"{x}, {what}")


def expect(t, b, cls="own", bound="own"):
    return R.lookup(b.buf, b.desc, b.seg, b.cls if isinstance(cls, str) else cls, t.conn, t.flow,
                    t.bound if isinstance(bound, str) else bound)


@pytest.fixture(scope="module")
def corpus():
    cs = PB.corpus()
    return cs, [expect(c.table, c.burst) for c in cs]


@pytest.fixture(scope="module")
def mixed(corpus):
    cs, ex = corpus
    assert cs[-1].name == "mixed"
    return cs[-1], ex[-1]


# -- 1. the corpus: every table class, desc at shifts 0, 4, 8, 12 -------------------------

@pytest.mark.parametrize("i", range(6))
def test_corpus(engine, corpus, i, mode):
    cs, ex = corpus
    c, exp = cs[i], ex[i]
    dt = DevTable(engine, c.table)
    try:
        same(dt.build(), R.table(c.table.conn, c.table.flow)[1], f"stat, {c.name}")
        assert engine.last_kernel == "pcbb_kernel<%s>" % ("true", "false")[bool(mode & 2)]
        b = c.burst
        got, kern = look(engine, dt, b.buf, b.desc, b.seg, b.cls, calls=2, shift=4 * (i % 4))
        assert kern == kernel_of(ALL, mode), kern
        judge(got, exp, c.name, calls=2)
        same(got["count"][R.NCOUNT:], SEED[R.NCOUNT:], "count[6..]")
        same(dt.build(), R.table(c.table.conn, c.table.flow)[1], "stat of a second build: written, not accumulated")
        dt.check()
    finally:
        dt.free()


# -- 2. build sizes -----------------------------------------------------------------------

def plain_table(rng, nconn):
    """nconn distinct tuples of one flow, with an unused entry, a bad one and a copy of
    entry 0 at the end where there is room."""
    conn = np.zeros(nconn, R.CONN_DTYPE)
    conn["lport"], conn["fport"], conn["proto"] = [PB.be16(5000 + j) for j in range(nconn)], PB.be16(80), 6
    if nconn >= 63:
        conn["proto"][nconn - 3] = 0
        conn["flow"][nconn - 2] = 1
        conn[nconn - 1] = conn[0]
    return PB.Table(f"plain {nconn}", conn, [PB.flow_rec(rng, False, bytes([10, 0, 0, 1]), PB.FADDR)], PB.bound_ports(nconn))


@pytest.mark.parametrize("nconn", [0, 1, 63, 64, 65, 300, 8193])
def test_build_sizes(engine, nconn, mode):
    """One workgroup and a lane, a wave and its neighbours, several workgroups, a table
    past 2^13; with mode bit 0 one chain of all entries that wraps at the last slot."""
    rng = np.random.default_rng(70 + nconn)
    t = plain_table(rng, nconn)
    want = [j for j in (0, 1, 30, 62, 63, 64, 150, 299, 4095, 4096, 8100, 8192) if j < nconn and int(t.conn["proto"][j])
            and int(t.conn["flow"][j]) == 0]
    specs = [("hit", t.spec(j), None) for j in want]
    s = (False, 6, bytes([10, 0, 0, 1]), PB.FADDR, PB.be16(5000), PB.be16(80))
    specs += [("miss", s[:4] + (PB.be16(5000 + nconn + 5), s[5]), None), ("miss", s[:2] + (bytes([10, 0, 0, 2]),) + s[3:], None),
              ("bound", s[:4] + (PB.be16(80), s[5]), None), ("skip", s, ("cls", 3)), ("none", s, ("len", 19))]
    b = PB.burst(specs, rng)
    exp = expect(t, b)
    assert (R.HIT in exp[2]) == (nconn > 0) and {R.MISS, R.BOUND, R.SKIP, R.NONE_} <= {int(x) for x in exp[2]}
    dt = DevTable(engine, t)
    try:
        stat = R.table(t.conn, t.flow)[1]
        assert int(stat.sum()) == nconn and (nconn < 63 or stat[1:].tolist() == [1, 1, 1])
        same(dt.build(), stat, f"stat, nconn {nconn}")
        got, _ = look(engine, dt, b.buf, b.desc, b.seg, b.cls)
        judge(got, exp, f"nconn {nconn}")
        dt.check()
    finally:
        dt.free()


# -- 3. burst sizes -----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tails(engine, mixed, n, mode):
    c, exp = mixed
    m = len(c.burst.desc)
    buf, desc, seg, cls = PB.tiled(c.burst, n)
    buf = buf[:int(desc["frame_off"][-1]) + PB.SLOT]
    want = R.lookup(buf, desc, seg, cls, c.table.conn, c.table.flow, c.table.bound)
    k = np.arange(n) % m
    assert np.array_equal(want[0], exp[0][k]) and np.array_equal(want[2], exp[2][k])
    dt = DevTable(engine, c.table)
    try:
        dt.build(stat=False)
        got, kern = look(engine, dt, buf, desc, seg, cls, shift=4 * (n % 4))
        assert kern == kernel_of(ALL, mode), kern
        judge(got, want, f"n {n}")
        dt.check()
    finally:
        dt.free()


def test_three_passes(engine, mixed, mode):
    """Above twice what one pass of the grid covers, plus a step and a frame: every
    wave runs three steps.  The burst is the mixed class repeated; so is the
    expectation."""
    c, exp = mixed
    per_pass = engine.pcb_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024
    n, m = 2 * per_pass + 65, len(c.burst.desc)
    assert n * PB.SLOT < 128_000_000
    reps = -(-n // m)
    k = np.arange(n)
    fr = Frames(engine, np.tile(c.burst.buf, reps)[:n * PB.SLOT])
    desc = np.zeros(n, l4bref.DESC_DTYPE)
    desc["frame_off"] = (k // m) * len(c.burst.buf) + c.burst.desc["frame_off"][k % m]
    desc["l3_off"], desc["ip_len"] = c.burst.desc["l3_off"][k % m], c.burst.desc["ip_len"][k % m]
    L, st = cgck.load(), engine.stream
    sizes = {"desc": 12 * n, "seg": 32 * n, "cls": n, "idx": 4 * n, "fidx": 4 * n, "kind": n, "count": 4 * NC}
    dev = {x: cgck.DeviceBuffer(2 * CAN + sz) for x, sz in sizes.items()}
    dt = DevTable(engine, c.table)
    try:
        for x, d in dev.items():
            assert L.cgck_memset(d.ptr, CANARY, 2 * CAN + sizes[x], st) == 0
            assert L.cgck_memset(d.ptr + CAN, 0xEE, sizes[x], st) == 0
        piece = max(m, (16384 // m) * m)                # uploads in pieces below 1 MiB
        for a in range(0, n, piece):
            e = min(a + piece, n)
            dev["desc"].upload(desc[a:e], off=CAN + 12 * a, stream=st)
            dev["seg"].upload(c.burst.seg[k[a:e] % m], off=CAN + 32 * a, stream=st)
            dev["cls"].upload(c.burst.cls[k[a:e] % m], off=CAN + a, stream=st)
        dev["count"].upload(SEED, off=CAN, stream=st)
        dt.build(stat=False)
        engine.pcb_lookup(fr.ptr, dev["desc"].ptr + CAN, dev["seg"].ptr + CAN, n, dt.pcb, cls=dev["cls"].ptr + CAN,
                          **{x: dev[x].ptr + CAN for x in ALL})
        assert engine.last_kernel == kernel_of(ALL, mode), engine.last_kernel

        def fetch(x, off, count, dtype):
            got = np.zeros(count, dtype)
            for a in range(0, count, 1 << 18):          # in pieces of at most 1 MiB
                dev[x].download(got[a:a + (1 << 18)], off=off + a * got.itemsize, stream=st)
            engine.sync()
            return got

        same(fetch("idx", CAN, n, np.uint32), exp[0][k % m], "idx")
        same(fetch("fidx", CAN, n, np.uint32), exp[1][k % m], "fidx")
        kind = exp[2][k % m]
        same(fetch("kind", CAN, n, np.uint8), kind, "kind")
        rem = n % m                                     # whole repeats of the class and the first `rem` frames once more
        want = SEED.copy()
        want[:R.NCOUNT] += np.uint32(n // m) * exp[3] + R.lookup(c.burst.buf, c.burst.desc[:rem], c.burst.seg[:rem], c.burst.cls[:rem],
                                                                   c.table.conn, c.table.flow, c.table.bound)[3]
        same(fetch("count", CAN, NC, np.uint32), want, "count")
        for x in dev:
            for off in (0, CAN + sizes[x]):
                assert np.all(fetch(x, off, CAN, np.uint8) == CANARY), f"{x}: bytes outside the array were written"
        dt.check()
    finally:
        for d in (fr, dt, *dev.values()):
            d.free()


# -- 4. outputs, cls NULL, bound NULL -----------------------------------------------------

@pytest.mark.parametrize("names", [c for r in (1, 2, 3, 4) for c in itertools.combinations(ALL, r)], ids="+".join)
def test_outputs(engine, mixed, names, mode):
    """Every subset of the outputs; the counters after two calls (+=), with the four
    words past them untouched."""
    c, exp = mixed
    b = c.burst
    dt = DevTable(engine, c.table)
    try:
        dt.build(stat=False)
        got, kern = look(engine, dt, b.buf, b.desc, b.seg, b.cls, names, calls=2)
        assert tuple(got) == names and kern == kernel_of(names, mode), kern
        judge(got, exp, f"outputs {names}", calls=2)
        if "count" in got:
            same(got["count"][R.NCOUNT:], SEED[R.NCOUNT:], "count[6..]")
    finally:
        dt.free()


@pytest.mark.parametrize("what", ["cls NULL", "bound NULL", "both NULL"])
def test_null_cls_and_bound(engine, mixed, what, mode):
    c, _ = mixed
    b = c.burst
    cls = None if what != "bound NULL" else b.cls
    bound = None if what != "cls NULL" else c.table.bound
    exp = expect(c.table, b, cls=cls, bound=bound)
    assert (R.BOUND in exp[2]) == (bound is not None) and (R.SKIP in exp[2]) == (cls is not None)
    dt = DevTable(engine, c.table, use_bound=bound is not None)
    try:
        dt.build(stat=False)
        got, _ = look(engine, dt, b.buf, b.desc, b.seg, cls)
        judge(got, exp, what)
        dt.check()
    finally:
        dt.free()


# -- 5. a table the library did not build -------------------------------------------------

@pytest.mark.parametrize("fill", ["0x00", "0xFF", "random"])
def test_foreign_table(engine, corpus, fill, mode):
    """The call returns, no canary moves, every reported HIT is a true key match, and
    a frame that is not looked up or has no connection gets what the referee says."""
    cs, ex = corpus
    c, exp = cs[2], ex[2]
    b, t = c.burst, c.table
    dt = DevTable(engine, t)
    try:
        raw = {"0x00": np.zeros(dt.bytes, np.uint8), "0xFF": np.full(dt.bytes, 0xFF, np.uint8),
               "random": np.random.default_rng(81).integers(0, 256, dt.bytes, dtype=np.uint8)}[fill]
        dt.table.put(raw)
        got, _ = look(engine, dt, b.buf, b.desc, b.seg, b.cls)
        same(dt.table.get(np.uint8, "table"), raw, "the table after a lookup")
        eidx, efidx, ekind, _ = exp
        for k in range(len(ekind)):
            gk, gi = int(got["kind"][k]), int(got["idx"][k])
            if gk == R.HIT:
                o = int(b.desc["frame_off"][k]) + int(b.desc["l3_off"][k])
                assert R.true_hit(b.buf[o:o + int(b.desc["ip_len"][k])], b.cls[k], b.seg[k], t.conn, t.flow, gi), k
                assert int(got["fidx"][k]) == int(t.conn["flow"][gi])
            elif ekind[k] == R.HIT:                     # a hit the foreign table cost: what rules 4 and 5 give
                assert gk in (R.MISS, R.BOUND) and int(got["fidx"][k]) == R.NOIDX, k
            else:
                assert (gk, gi, int(got["fidx"][k])) == (int(ekind[k]), int(eidx[k]), int(efidx[k])), k
        assert int(got["count"][:5].sum() - SEED[:5].sum()) == len(ekind)
        if fill == "0xFF":                              # an empty table: no hit at all
            assert R.HIT not in got["kind"]
        dt.check()
    finally:
        dt.free()


# -- 6. the last address byte is the allocation's last byte -------------------------------

@pytest.mark.parametrize("align", range(16))
def test_last_byte_of_the_allocation(engine, mixed, align, mode):
    c, _ = mixed
    dt = DevTable(engine, c.table)
    try:
        dt.build(stat=False)
        for six in (False, True):
            b = PB.tail_burst(c.table, align, six, np.random.default_rng(90 + align))
            o = int(b.desc["frame_off"][2]) + int(b.desc["l3_off"][2])
            assert o % 16 == align and o + (40 if six else 20) == len(b.buf)
            exp = expect(c.table, b)
            assert exp[2].tolist() == [R.HIT, R.MISS, R.HIT]
            got, _ = look(engine, dt, b.buf, b.desc, b.seg, b.cls, shift=4 * (align % 4))
            judge(got, exp, f"alignment {align}, IPv{6 if six else 4}")
    finally:
        dt.free()


# -- 7. composition on the device ---------------------------------------------------------

def test_build_desc_lookup_build(engine, mode):
    """cgck_l4_build -> cgck_l4_desc -> cgck_pcb_lookup: fidx out is fidx in for unique
    tuples; that fidx then drives a second cgck_l4_build, the replies."""
    rng = np.random.default_rng(95)
    nflow, n = 200, 300
    flow = np.zeros(nflow, l4bref.FLOW_DTYPE)           # our table: laddr is ours, the received frame's destination
    for f in range(nflow):
        six = f % 3 == 0
        flow[f] = PB.flow_rec(rng, six, bytes([10, 0, f // 100, f % 100]) + bytes(12 if six else 0),
                              bytes([10, 9, 0, f % 7]) + bytes(12 if six else 0))
    conn = np.zeros(nflow, R.CONN_DTYPE)
    conn["flow"], conn["lport"], conn["fport"] = np.arange(nflow), PB.be16(7000), PB.be16(80)
    conn["proto"] = np.where(np.arange(nflow) % 4 == 1, 17, 6)
    t = PB.Table("unique", conn, flow, None)
    peer = flow.copy()
    peer["laddr"], peer["faddr"] = flow["faddr"], flow["laddr"]
    fidx = rng.integers(0, nflow, n).astype(np.uint32)
    seg = np.zeros(n, l4bref.SEG_DTYPE)
    seg["sport"], seg["dport"], seg["th_flags"], seg["seq"] = PB.be16(80), PB.be16(7000), 0x12, rng.integers(0, 2 ** 32, n)
    cls = np.where(conn["proto"][fidx] == 17, l4bref.SEG_UDP, l4bref.SEG_TCP).astype(np.uint8)
    slot = np.zeros(n, l4bref.DESC_DTYPE)
    slot["frame_off"], slot["l3_off"], slot["ip_len"] = np.arange(n) * 128, np.arange(n) % 4, 120
    rep = seg.copy()                                    # our answers: the ports swapped, an ACK
    rep["sport"], rep["dport"], rep["th_flags"], rep["ack"] = seg["dport"], seg["sport"], 0x10, seg["seq"] + np.uint32(1)
    ebuf = np.zeros(n * 128, np.uint8)
    l4bref.build(ebuf, slot, rep, flow, cls, fidx, 9, 0x4000)

    fr, fr2 = Frames(engine, np.zeros(n * 128, np.uint8)), Guarded(engine, n * 128, 0)
    ins = [Guarded(engine, 12 * n).put(slot), Guarded(engine, 32 * n).put(seg), Guarded(engine, 48 * nflow).put(peer),
           Guarded(engine, n).put(cls), Guarded(engine, 4 * n).put(fidx), Guarded(engine, 32 * n).put(rep)]
    desc, sg, c4 = Guarded(engine, 12 * n, 0xEE), Guarded(engine, 32 * n, 0xEE), Guarded(engine, n, 0xEE)
    out, kind = Guarded(engine, 4 * n, 0xEE), Guarded(engine, n, 0xEE)
    dt = DevTable(engine, t)
    try:
        same(dt.build(), [nflow, 0, 0, 0], "stat")
        engine.l4_build(fr.ptr, n, ins[0].ptr, ins[1].ptr, ins[2].ptr, nflow, cls=ins[3].ptr, fidx=ins[4].ptr, ip_id0=1,
                        ip_off=0x4000, desc_out=desc.ptr)
        engine.l4_desc(fr.ptr, desc.ptr, n, seg=sg.ptr, cls=c4.ptr)
        engine.pcb_lookup(fr.ptr, desc.ptr, sg.ptr, n, dt.pcb, cls=c4.ptr, fidx=out.ptr, kind=kind.ptr)
        engine.l4_build(fr2.ptr, n, ins[0].ptr, ins[5].ptr, dt.flow.ptr, nflow, cls=c4.ptr, fidx=out.ptr, ip_id0=9, ip_off=0x4000)
        same(kind.get(np.uint8, "kind"), np.full(n, R.HIT, np.uint8), "kind")
        same(out.get(np.uint32, "fidx"), fidx, "fidx out against fidx in")
        same(fr2.get(np.uint8, "the replies"), ebuf, "the frames the second cgck_l4_build wrote from the looked-up fidx")
        dt.check()
    finally:
        for x in (fr, fr2, *ins, desc, sg, c4, out, kind, dt):
            x.free()


# -- 8. arguments -------------------------------------------------------------------------

def test_arguments(engine, mixed, mode):
    L, by = cgck.load(), ctypes.byref
    c, exp = mixed
    b, t = c.burst, c.table
    n = len(b.desc)
    fr = Frames(engine, b.buf)
    dd, sg, cl = Guarded(engine, 12 * n).put(b.desc), Guarded(engine, 32 * n).put(b.seg), Guarded(engine, n).put(b.cls)
    o = Guarded(engine, 4096, 0xEE)
    dt = DevTable(engine, t)
    ctx = engine.ctx
    full = cgck.PcbRes(o.ptr, o.ptr + 1024, o.ptr + 2048, o.ptr + 3072)
    P = dt.pcb
    fields = [f for f, _ in cgck.Pcb._fields_]

    def pcb(**kw):
        return cgck.Pcb(**{**{f: getattr(P, f) for f in fields}, **kw})

    def rc(c=ctx, base=fr.ptr, desc=dd.ptr, seg=sg.ptr, cnt=n, p=P, rs=full):
        return L.cgck_pcb_lookup(c, base, desc, seg, cl.ptr, cnt, None if p is None else by(p), None if rs is None else by(rs), None)

    def rb(c=ctx, p=P, stat=None):
        return L.cgck_pcb_build(c, None if p is None else by(p), stat, None)

    try:
        dt.build(stat=False)
        tbl = dt.table.get(np.uint8, "table")
        bad_pcbs = (("conn misaligned", pcb(conn=P.conn + 2)), ("flow at +8", pcb(flow=P.flow + 8)),
                    ("table at +8", pcb(table=P.table + 8)), ("bound misaligned", pcb(bound=P.bound + 2)),
                    ("nconn above 1 << 30", pcb(nconn=(1 << 30) + 1, table_bytes=1 << 40)), ("NULL conn", pcb(conn=None)),
                    ("NULL flow", pcb(flow=None)), ("NULL table", pcb(table=None)), ("table_bytes short", pcb(table_bytes=dt.bytes - 1)),
                    ("table_bytes 0", pcb(table_bytes=0)))
        cases = [("NULL ctx", rc(c=None)), ("NULL base", rc(base=None)), ("NULL pcb", rc(p=None)), ("NULL res", rc(rs=None)),
                 ("NULL desc", rc(desc=None)), ("NULL seg", rc(seg=None)), ("every output NULL", rc(rs=cgck.PcbRes())),
                 ("desc misaligned", rc(desc=dd.ptr + 2)), ("seg at +8", rc(seg=sg.ptr + 8)), ("seg at +4", rc(seg=sg.ptr + 4)),
                 ("idx misaligned", rc(rs=cgck.PcbRes(o.ptr + 2, None, None, None))),
                 ("n == 0, NULL base", rc(cnt=0, base=None)), ("n == 0, every output NULL", rc(cnt=0, rs=cgck.PcbRes())),
                 ("build: NULL ctx", rb(c=None)), ("build: NULL pcb", rb(p=None)), ("build: stat misaligned", rb(stat=o.ptr + 2))]
        cases += [(f"lookup: {w}", rc(p=p)) for w, p in bad_pcbs] + [(f"build: {w}", rb(p=p)) for w, p in bad_pcbs]
        cases += [(f"lookup, n == 0: {w}", rc(cnt=0, p=p)) for w, p in bad_pcbs[:3]]
        for what, r in cases:
            assert r == EINVAL, (what, r)
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after the refused calls")
        same(dt.table.get(np.uint8, "table"), tbl, "the table after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        before = engine.last_kernel
        assert before.startswith("pcbb_kernel")
        assert rc(cnt=0) == 0 and rc(cnt=0, desc=None, seg=None) == 0
        engine.sync()
        assert engine.last_kernel == before
        same(o.get(np.uint8, "outputs"), np.full(4096, 0xEE, np.uint8), "outputs after n == 0")
        # the same arguments with n > 0 are accepted
        assert rc() == 0 and engine.last_kernel == kernel_of(ALL, mode)
        got = o.get(np.uint8, "outputs")
        same(got[:4 * n].view(np.uint32), exp[0], "idx")
        same(got[1024:1024 + 4 * n].view(np.uint32), exp[1], "fidx")
        same(got[2048:2048 + n], exp[2], "kind")
        same(got[3072:3072 + 4 * R.NCOUNT].view(np.uint32), np.uint32(0xEEEEEEEE) + exp[3], "count (running from 0xEEEEEEEE)")
        same(got[3072 + 4 * R.NCOUNT:3584], np.full(512 - 4 * R.NCOUNT, 0xEE, np.uint8), "the words past count[6)")
        dt.check()
    finally:
        for x in (fr, dd, sg, cl, o, dt):
            x.free()
