"""cgck_l4_reply and cgck_l4_reply_packed (l4r_kernel: cgck_l4r.hip).  Every output of
every call is compared with the referee (tests/l4rref.py), never with the library
itself, by exact equality.  Every array lies between canary bytes that must survive
(64 bytes: more than one record past n) and starts as 0xEE bytes, the inputs are read
back unchanged, and the frame buffer is a plain allocation of exactly the burst's
bytes."""
import ctypes
import itertools

import numpy as np
import pytest

import cgck
import l4bref
import l4rbatches as LB
import l4rref as R
import pcbref
import rxcorpus

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL = ("seg", "flow", "cls", "queue", "count")
SELECTORS = ("cls", "kind", "verdict", "l2cls")
CAN, CANARY, POISON = 64, 0xC3, 0xA5
NC = 12                                                 # counters allocated: 8 and four that stay untouched
SEED = (np.arange(NC, dtype=np.uint32) * 7 + 3)         # count[] before a call: running counters
DTYPES = {"seg": R.SEG_DTYPE, "flow": R.FLOW_DTYPE, "cls": np.uint8, "queue": np.uint8, "count": np.uint32}
SIZE = {"seg": 32, "flow": 48, "cls": 1, "queue": 1}


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
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
        self.eng, self.want = eng, np.ascontiguousarray(buf)
        self.buf = cgck.DeviceBuffer(max(buf.nbytes, 1))
        assert self.buf.ptr % 16 == 0
        self.buf.upload(self.want, stream=eng.stream)
        self.ptr = self.buf.ptr

    def check(self):
        got = np.zeros_like(self.want)
        if got.nbytes:
            self.buf.download(got, stream=self.eng.stream)
            self.eng.sync()
        same(got, self.want, "the frames after the calls")

    def free(self):
        self.buf.free()


def kernel_of(names, at=None, shape=cgck.L4R_STORE_DEFAULT):
    rec, x = bool({"seg", "flow"} & set(names)), bool({"cls", "queue", "count"} & set(names))
    a = 0 if at is None else 2 if rec and shape == cgck.L4R_STORE_TURNED else 1
    return "l4r_kernel<%s, %s, %d>" % (("false", "true")[rec], ("false", "true")[x], a)


def blank(n):
    """What seg, flow and cls hold before a call."""
    return {x: np.full(n * SIZE[x], 0xEE, np.uint8).view(DTYPES[x]) for x in ("seg", "flow", "cls")}


def run(eng, b, vm=0, flags=0, names=ALL, drop=(), at=None, calls=1, shift=0, packed=False, link=LB.LINK):
    """cgck_l4_reply (or _packed) over Burst b, `calls` times: ({name: array}, kernel
    name).  The outputs start as 0xEE bytes, count as SEED; desc, at and count lie
    `shift` bytes past a 16-byte boundary.  packed adds "at" and "qoff"."""
    n = len(b.desc)
    fr = Frames(eng, b.buf)
    ins = {"desc": (Guarded(eng, 12 * n, shift=shift).put(b.desc), b.desc), "seg": (Guarded(eng, 32 * n).put(b.seg), b.seg)}
    for i, x in enumerate(SELECTORS):
        if x not in drop:
            ins[x] = (Guarded(eng, n, shift=i + 1).put(getattr(b, x)), getattr(b, x))
    if at is not None:
        ins["at"] = (Guarded(eng, 4 * n, shift=shift).put(np.asarray(at, np.uint32)), np.asarray(at, np.uint32))
    mem = {x: Guarded(eng, 4 * NC if x == "count" else n * SIZE[x], 0xEE, shift=shift if x == "count" else 0) for x in names}
    if "count" in mem:
        mem["count"].put(SEED)
    pk = {}
    if packed:
        wb = cgck.steer_work_bytes(n, 1)
        pk = {"queue": Guarded(eng, n, 0xEE), "at": Guarded(eng, 4 * n, 0xEE, shift=shift), "qoff": Guarded(eng, 12, 0xEE, shift=4)}
        if wb:
            pk["work"] = Guarded(eng, wb, 0xEE)
    try:
        sel = {x: ins[x][0].ptr if x in ins else None for x in SELECTORS}
        outs = {{"seg": "seg_out", "flow": "flow_out", "cls": "cls_out"}.get(x, x): mem[x].ptr for x in names}
        for _ in range(calls):
            if packed:
                eng.l4_reply_packed(fr.ptr, n, ins["desc"][0].ptr, ins["seg"][0].ptr, link, pk["queue"].ptr, pk["at"].ptr,
                                    pk["qoff"].ptr, work=pk["work"].ptr if "work" in pk else None, vmask=vm, flags=flags,
                                    **sel, **outs)
            else:
                eng.l4_reply(fr.ptr, n, ins["desc"][0].ptr, ins["seg"][0].ptr, link, at=ins["at"][0].ptr if at is not None else None,
                             vmask=vm, flags=flags, **sel, **outs)
        kern = eng.last_kernel
        got = {x: mem[x].get(DTYPES[x], x) for x in names}
        if packed:
            got["at"], got["qoff"] = pk["at"].get(np.uint32, "pk.at"), pk["qoff"].get(np.uint32, "pk.qoff")
            got["pk.queue"] = pk["queue"].get(np.uint8, "pk.queue")
            if "work" in pk:
                pk["work"].get(np.uint8, "work")
        for x, (g, a) in ins.items():
            same(g.get(np.uint8, x), np.ascontiguousarray(a).view(np.uint8).reshape(-1), f"{x}[] after the call")
        fr.check()
    finally:
        for x in (fr, *(g for g, _ in ins.values()), *mem.values(), *pk.values()):
            x.free()
    return got, kern


def judge(got, exp, what, calls=1):
    for x in got:
        if x == "count":
            want = SEED.copy()
            want[:R.NCOUNT] += np.uint32(calls) * exp["count"]
            same(got[x], want, f"count after {calls} call(s), {what}")
        elif x == "pk.queue":
            same(got[x], exp["queue"], f"pk.queue, {what}")
        elif got[x].dtype.names:
            same(got[x].view(np.uint8), np.ascontiguousarray(exp[x]).view(np.uint8), f"{x} (bytes), {what}")
        else:
            same(got[x], exp[x], f"{x}, {what}")


def expect(b, vm, flags, drop=(), at=None):
    return R.reply(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, at=at, before=blank(len(b.desc)), **b.sel(drop))


@pytest.fixture(scope="module")
def corpus():
    return LB.corpus()


@pytest.fixture(params=[cgck.L4R_STORE_OWN, cgck.L4R_STORE_TURNED], ids=["own", "turned"])
def shape(request):
    before = cgck.l4_reply_store(request.param)
    yield request.param
    assert cgck.l4_reply_store(before) == request.param


# -- 1. the corpus under every (vmask, flags) pair; burst sizes ----------------------------

@pytest.mark.parametrize("i", range(len(LB.CONFIGS)))
def test_corpus(engine, corpus, i):
    vm, flags = LB.CONFIGS[i]
    got, kern = run(engine, corpus, vm, flags, calls=2, shift=4 * (i % 4))
    assert kern == kernel_of(ALL), kern
    judge(got, expect(corpus, vm, flags), f"vmask {vm}, flags {flags}", calls=2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tails(engine, corpus, n):
    vm, flags = LB.CONFIGS[n % len(LB.CONFIGS)]
    b = LB.tiled(corpus, n)
    got, _ = run(engine, b, vm, flags, shift=4 * (n % 4))
    judge(got, expect(b, vm, flags), f"n {n}")


def test_three_steps(engine, corpus):
    """Twice what one pass of the grid covers and a frame: every wave runs three steps.
    The descriptors alias the corpus frames; so does the expectation."""
    vm, flags = 5, R.NO_MCAST
    per_pass = engine.l4_reply_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024
    n, m = 2 * per_pass + 1, len(corpus.desc)
    k = np.arange(n) % m
    e = expect(corpus, vm, flags)
    fr = Frames(engine, corpus.buf)
    L, st = cgck.load(), engine.stream
    ins = {"desc": corpus.desc[k], "seg": corpus.seg[k], **{x: getattr(corpus, x)[k] for x in SELECTORS}}
    sizes = {"desc": 12 * n, "seg": 32 * n, **{x: n for x in SELECTORS}, "oseg": 32 * n, "oflow": 48 * n, "ocls": n,
             "oqueue": n, "ocount": 4 * NC}
    dev = {x: cgck.DeviceBuffer(2 * CAN + sz) for x, sz in sizes.items()}

    def fetch(x, off, count, dtype):
        got = np.zeros(count, dtype)
        step = (1 << 20) // got.itemsize                # in pieces of at most 1 MiB
        for a in range(0, count, step):
            dev[x].download(got[a:a + step], off=off + a * got.itemsize, stream=st)
        engine.sync()
        return got

    try:
        for x, d in dev.items():
            assert L.cgck_memset(d.ptr, CANARY, 2 * CAN + sizes[x], st) == 0
            assert L.cgck_memset(d.ptr + CAN, 0xEE, sizes[x], st) == 0
        for x, a in ins.items():
            step = (1 << 20) // a.itemsize
            for o in range(0, n, step):
                dev[x].upload(a[o:o + step], off=CAN + o * a.itemsize, stream=st)
        dev["ocount"].upload(SEED, off=CAN, stream=st)
        p = {x: dev[x].ptr + CAN for x in dev}
        engine.l4_reply(fr.ptr, n, p["desc"], p["seg"], LB.LINK, cls=p["cls"], kind=p["kind"], verdict=p["verdict"],
                        l2cls=p["l2cls"], vmask=vm, flags=flags, seg_out=p["oseg"], flow_out=p["oflow"], cls_out=p["ocls"],
                        queue=p["oqueue"], count=p["ocount"])
        assert engine.last_kernel == kernel_of(ALL), engine.last_kernel
        same(fetch("oseg", CAN, 32 * n, np.uint8), e["seg"][k].view(np.uint8), "seg")
        same(fetch("oflow", CAN, 48 * n, np.uint8), e["flow"][k].view(np.uint8), "flow")
        same(fetch("ocls", CAN, n, np.uint8), e["cls"][k], "cls")
        same(fetch("oqueue", CAN, n, np.uint8), e["queue"][k], "queue")
        want = SEED.copy()
        want[:R.NCOUNT] += R.counts(e["cls"][k])
        same(fetch("ocount", CAN, NC, np.uint32), want, "count")
        for x in dev:
            for off in (0, CAN + sizes[x]):
                assert np.all(fetch(x, off, CAN, np.uint8) == CANARY), f"{x}: bytes outside the array were written"
        for x, a in ins.items():
            same(fetch(x, CAN, sizes[x], np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), f"{x}[] after the call")
        fr.check()
    finally:
        for d in (fr, *dev.values()):
            d.free()


# -- 2. outputs, selectors ------------------------------------------------------------------

@pytest.mark.parametrize("names", [c for r in range(1, 6) for c in itertools.combinations(ALL, r)], ids="+".join)
def test_outputs(engine, corpus, names):
    """Every non-empty subset of the outputs; the counters after two calls (+=), with
    the words past them untouched."""
    vm, flags = 4, R.NO_RST
    got, kern = run(engine, corpus, vm, flags, names, calls=2)
    assert tuple(got) == names and kern == kernel_of(names), kern
    judge(got, expect(corpus, vm, flags), f"outputs {names}", calls=2)


@pytest.mark.parametrize("drop", [(x,) for x in SELECTORS] + [SELECTORS], ids="+".join)
def test_null_selectors(engine, corpus, drop):
    vm, flags = 7, R.NO_RST | R.NO_MCAST
    e = expect(corpus, vm, flags, drop)
    assert not np.array_equal(e["cls"], expect(corpus, vm, flags)["cls"])       # the selector mattered
    got, _ = run(engine, corpus, vm, flags, drop=drop)
    judge(got, e, f"NULL {drop}")


# -- 3. at ----------------------------------------------------------------------------------

def targets(kind, n, rng):
    at = {"identity": np.arange(n), "reversal": np.arange(n)[::-1], "permutation": rng.permutation(n)}[kind].astype(np.int64)
    out = rng.choice(n, n // 5, replace=False)          # a fifth of the frames go nowhere
    at[out] = np.where(np.arange(len(out)) % 3 == 0, 0xFFFFFFFF, n + np.arange(len(out)) * 7)
    at[out[:2]] = (n, n + 1)                            # the first index past the arrays
    return at.astype(np.uint32)


@pytest.mark.parametrize("kind", ["identity", "reversal", "permutation"])
@pytest.mark.parametrize("n", [0, 257])
def test_at(engine, corpus, kind, n, shape):
    """seg, flow and cls land at at[k]; queue stays at k; a frame with at[k] >= n writes
    none of the three (its would-be targets keep 0xEE) and is still counted."""
    vm, flags = 0, R.NO_MCAST
    b = corpus if n == 0 else LB.tiled(corpus, n)
    at = targets(kind, len(b.desc), np.random.default_rng(17))
    e = expect(b, vm, flags, at=at)
    kept = np.setdiff1d(np.arange(len(b.desc)), at[at < len(b.desc)])
    assert len(kept) == len(b.desc) // 5 and np.all(e["cls"][kept] == 0xEE)
    got, kern = run(engine, b, vm, flags, at=at, shift=4)
    assert kern == kernel_of(ALL, at, shape), kern
    judge(got, e, f"at: {kind}")
    for names in (("seg",), ("flow", "count"), ("cls", "queue")):
        got, kern = run(engine, b, vm, flags, names, at=at)
        assert kern == kernel_of(names, at, shape), kern
        judge(got, e, f"at: {kind}, outputs {names}")


# -- 4. the packed form ---------------------------------------------------------------------

def packed_case(corpus, what):
    if what == "corpus":
        return corpus
    if what == "5000 frames":                           # above one tile of the steer: three launches and a workspace
        return LB.tiled(corpus, 5000)
    b = LB.tiled(corpus, len(corpus.desc))
    if what == "R = 0":
        b.kind[:] = cgck.PCB_HIT
    else:
        keep = np.nonzero(R.per_frame(b.buf, b.desc, b.seg, LB.LINK, vm=7, flags=0, **b.sel())[0] & 15 == R.RST)[0]
        b.desc, b.seg = b.desc[keep], b.seg[keep]
        b.cls, b.kind, b.verdict, b.l2cls = b.cls[keep], b.kind[keep], b.verdict[keep], b.l2cls[keep]
    return b


@pytest.mark.parametrize("what", ["corpus", "R = 0", "R = n", "5000 frames"])
def test_packed(engine, corpus, what, shape):
    vm, flags = 7, 0
    b = packed_case(corpus, what)
    n = len(b.desc)
    e = R.packed(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, **b.sel())
    nrst = int(e["qoff"][1])
    assert {"R = 0": nrst == 0, "R = n": nrst == n and n > 20}.get(what, 0 < nrst < n)
    assert (cgck.steer_work_bytes(n, 1) != 0) == (what == "5000 frames")
    assert np.all(e["cls"][:nrst] & 15 == R.RST) and np.all(e["cls"][nrst:] & 15 != R.RST)
    got, kern = run(engine, b, vm, flags, calls=2, packed=True, shift=4)
    assert kern == kernel_of(ALL, e["at"], shape), kern
    judge(got, e, f"packed, {what}", calls=2)           # two calls: the counters are counted once a call
    got, _ = run(engine, b, vm, flags, ("seg", "flow", "cls"), packed=True)
    judge(got, e, f"packed without queue and count, {what}")


# -- 5. alignment ---------------------------------------------------------------------------

@pytest.mark.parametrize("align", range(16))
def test_last_byte_of_the_allocation(engine, align):
    for six in (False, True):
        b = LB.tail_burst(align, six, np.random.default_rng(40 + align))
        o = int(b.desc["frame_off"][2]) + int(b.desc["l3_off"][2])
        assert o % 16 == align and o + (40 if six else 20) == len(b.buf)
        e = expect(b, 7, 0)
        assert np.all(e["cls"] & 15 == R.RST) and (e["cls"] & R.IP6 != 0).tolist() == [six, not six, six]
        got, _ = run(engine, b, 7, 0, shift=4 * (align % 4))
        judge(got, e, f"alignment {align}, IPv{6 if six else 4}")


# -- 6. the round trip ----------------------------------------------------------------------

def replay_ring(port, buf, rx, n, slot, id0):
    fns = port.fn_pointers()
    tx = np.full(n * slot, POISON, np.uint8)
    res, _, txs, _ = port.replay_rx_rsp(fns[0], fns[1], buf.copy(), rx.view(np.uint8), n, 2, 2, tx, slot, n,
                                        np.zeros(2048, np.uint8), rxcorpus.LADDR, None, id0)
    acc = int(np.count_nonzero(res == port.R_ACCEPT))
    assert txs.tolist() == [acc, 0, acc, 0, 0, 0] and 0 < acc
    return tx, acc


@pytest.mark.parametrize("source", ["built", "replay burst"])
def test_round_trip(engine, port, source, shape):
    """A receive burst, then cgck_desc (the verify), cgck_l4_desc, cgck_pcb_lookup against
    a small table, cgck_l4_reply_packed and cgck_l4_build on the device: the transmit
    ring equals the reference replay's (tcp_input without a PCB, tcp_respond, ip_output),
    ip_id included.  built: the receive burst is cgck_l4_build's own, from the peers'
    flows.  replay burst: the IPv4 burst of the CPU test, bad sums, short segments and
    bad offsets included."""
    rng = np.random.default_rng(96)
    slot, id0 = 128, 0xFFF0
    eng = engine
    table = None
    if source == "built":
        n = 150
        peer = np.zeros(n, l4bref.FLOW_DTYPE)           # the peers: their frames' source is foreign, the destination ours
        peer["eth_dst"], peer["eth_src"], peer["ttl"] = (2, 0, 0, 0, 0, 2), (2, 0, 0, 0, 0, 1), 64
        peer["laddr"][:, :4] = [(10, 9, k // 100, k % 100) for k in range(n)]
        peer["faddr"][:, :4] = [(10, 0, 0, 1 + k % 4) for k in range(n)]
        seg = np.zeros(n, l4bref.SEG_DTYPE)
        seg["sport"], seg["dport"] = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
        seg["seq"], seg["ack"], seg["win"] = rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 65536, n)
        seg["th_flags"] = np.array((0x02, 0x10, 0x12, 0x18, 0x11, 0x00, 0x01, 0x03, 0x04, 0x14))[np.arange(n) % 10]
        seg["opt"] = np.where(seg["th_flags"] & 2, np.arange(n) % 8, (np.arange(n) % 2) * 4)
        seg["mss"], seg["wscale"], seg["ts_val"], seg["ts_ecr"] = 1460, 7, rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n)
        rxslot = np.zeros(n, l4bref.DESC_DTYPE)
        rxslot["frame_off"], rxslot["l3_off"], rxslot["ip_len"] = np.arange(n) * 128, np.arange(n) % 4, 120
        hbuf = np.zeros(n * 128, np.uint8)
        _, rx, _, _ = l4bref.build(hbuf, rxslot, seg, peer, None, None, 77, 0x4000)
        table = (peer, seg, rxslot)
    else:
        frames = LB.replay_frames(np.random.default_rng(93), port)
        n = len(frames)
        hbuf, rx = rxcorpus.ring([p for _, p in frames])
    want, acc = replay_ring(port, hbuf, rx, n, slot, id0)
    assert acc == n if source == "built" else acc < n

    # a small table of connections no frame of the burst belongs to
    conn = np.zeros(8, pcbref.CONN_DTYPE)
    conn["flow"], conn["lport"], conn["fport"], conn["proto"] = np.arange(8) % 2, 1 + np.arange(8), 2, 6
    flow = np.zeros(2, l4bref.FLOW_DTYPE)
    flow["laddr"][:, :4], flow["faddr"][:, :4] = (192, 168, 0, 1), (192, 168, 0, 2)
    link = np.zeros(1, R.FLOW_DTYPE)[0]
    link["eth_dst"], link["eth_src"], link["ttl"] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2), 64
    txslot = np.zeros(n, l4bref.DESC_DTYPE)
    txslot["frame_off"], txslot["ip_len"] = np.arange(n) * slot, slot

    G = lambda nbytes, fill=0xEE, **kw: Guarded(eng, nbytes, fill, **kw)
    fr = Frames(eng, np.zeros_like(hbuf) if source == "built" else hbuf)
    ring = G(n * slot, POISON)
    d = {"rx": G(12 * n), "seg": G(32 * n), "cls": G(n), "ver": G(n), "kind": G(n), "rseg": G(32 * n), "rflow": G(48 * n),
         "rcls": G(n), "queue": G(n), "at": G(4 * n), "qoff": G(12, shift=4), "count": G(4 * R.NCOUNT, 0),
         "conn": G(12 * 8).put(conn), "flow": G(48 * 2).put(flow), "table": G(cgck.pcb_table_bytes(8)), "tx": G(12 * n).put(txslot)}
    try:
        if source == "built":
            peer, seg, rxslot = table
            ins = [G(12 * n).put(rxslot), G(32 * n).put(seg), G(48 * n).put(peer)]
            eng.l4_build(fr.ptr, n, ins[0].ptr, ins[1].ptr, ins[2].ptr, n, ip_id0=77, ip_off=0x4000, desc_out=d["rx"].ptr)
            d.update({f"in{i}": x for i, x in enumerate(ins)})
        else:
            d["rx"].put(rx)
        pcb = cgck.Pcb(d["conn"].ptr, 8, d["flow"].ptr, 2, d["table"].ptr, cgck.pcb_table_bytes(8), None)
        eng.pcb_build(pcb)
        eng.desc(fr.ptr, d["rx"].ptr, n, cgck.VERIFY_BSD, verdict=d["ver"].ptr)
        eng.l4_desc(fr.ptr, d["rx"].ptr, n, seg=d["seg"].ptr, cls=d["cls"].ptr)
        eng.pcb_lookup(fr.ptr, d["rx"].ptr, d["seg"].ptr, n, pcb, cls=d["cls"].ptr, kind=d["kind"].ptr)
        eng.l4_reply_packed(fr.ptr, n, d["rx"].ptr, d["seg"].ptr, link, d["queue"].ptr, d["at"].ptr, d["qoff"].ptr,
                            cls=d["cls"].ptr, kind=d["kind"].ptr, verdict=d["ver"].ptr, vmask=R.vmask(2, 2),
                            seg_out=d["rseg"].ptr, flow_out=d["rflow"].ptr, cls_out=d["rcls"].ptr, count=d["count"].ptr)
        eng.l4_build(ring.ptr, n, d["tx"].ptr, d["rseg"].ptr, d["rflow"].ptr, n, cls=d["rcls"].ptr, ip_id0=id0, ip_off=0x4000)
        same(ring.get(np.uint8, "the transmit ring"), want, "the transmit ring against the replay's")
        same(d["qoff"].get(np.uint32, "qoff"), np.array([0, acc, n], np.uint32), "qoff")
        cnt = d["count"].get(np.uint32, "count")
        assert int(cnt[R.RST]) == acc and int(cnt[:R.NCLASS].sum()) == n and int(cnt[7]) == 0
        assert int(cnt[R.NOTMISS]) == 0 and (int(cnt[R.DROPPED]) > 0 and int(cnt[R.SKIP]) > 0) == (source != "built")
        for x in d.values():
            x.get(np.uint8, "an array of the chain")    # no canary moved
    finally:
        for x in (fr, ring, *d.values()):
            x.free()


# -- 7. arguments ---------------------------------------------------------------------------

def test_arguments(engine, corpus):
    L, by = cgck.load(), ctypes.byref
    b = corpus
    n = len(b.desc)
    fr = Frames(engine, b.buf)
    dd, sg = Guarded(engine, 12 * n).put(b.desc), Guarded(engine, 32 * n).put(b.seg)
    o = Guarded(engine, 65536, 0xEE)
    at = Guarded(engine, 4 * n).put(np.arange(n, dtype=np.uint32))
    ctx = engine.ctx
    SEG, FLOW, CLS, QUEUE, COUNT, PKQ, PKAT, PKOFF = (o.ptr + 8192 * i for i in range(8))
    full = cgck.L4ReplyRes(SEG, FLOW, CLS, QUEUE, COUNT)
    fields = [f for f, _ in cgck.L4ReplyIn._fields_]
    A = cgck.L4ReplyIn(dd.ptr, sg.ptr, None, None, None, None, None, cgck.Flow.of(LB.LINK), 7, 0)

    def arg(**kw):
        a = cgck.L4ReplyIn(**{**{f: getattr(A, f) for f in fields}, **{k: v for k, v in kw.items() if k != "link_flags"}})
        if "link_flags" in kw:
            a.link.flags = kw["link_flags"]
        return a

    def rc(c=ctx, base=fr.ptr, cnt=n, a=A, rs=full):
        return L.cgck_l4_reply(c, base, cnt, None if a is None else by(a), None if rs is None else by(rs), None)

    PK = cgck.L4ReplyPack(PKQ, PKAT, PKOFF, None)

    def rp(c=ctx, base=fr.ptr, cnt=n, a=A, rs=full, pk=PK):
        return L.cgck_l4_reply_packed(c, base, cnt, None if a is None else by(a), None if rs is None else by(rs),
                                      None if pk is None else by(pk), None)

    try:
        shared = lambda f: [("NULL ctx", f(c=None)), ("NULL base", f(base=None)), ("NULL in", f(a=None)), ("NULL res", f(rs=None)),
                            ("NULL desc", f(a=arg(desc=None))), ("NULL seg", f(a=arg(seg=None))),
                            ("every output NULL", f(rs=cgck.L4ReplyRes())), ("desc misaligned", f(a=arg(desc=dd.ptr + 2))),
                            ("seg in at +8", f(a=arg(seg=sg.ptr + 8))), ("seg in at +4", f(a=arg(seg=sg.ptr + 4))),
                            ("count misaligned", f(rs=cgck.L4ReplyRes(None, None, None, None, COUNT + 2))),
                            ("seg out at +8", f(rs=cgck.L4ReplyRes(SEG + 8, None, None, None, None))),
                            ("flow out at +8", f(rs=cgck.L4ReplyRes(None, FLOW + 8, None, None, None))),
                            ("link.flags 4", f(a=arg(link_flags=4))), ("link.flags 0x83", f(a=arg(link_flags=0x83))),
                            ("flags 4", f(a=arg(flags=4))), ("flags 1 << 31", f(a=arg(flags=1 << 31))),
                            ("seg out is seg in", f(rs=cgck.L4ReplyRes(sg.ptr, None, None, None, None))),
                            ("n == 0, NULL base", f(cnt=0, base=None)), ("n == 0, every output NULL", f(cnt=0, rs=cgck.L4ReplyRes())),
                            ("n == 0, flags 4", f(cnt=0, a=arg(flags=4)))]
        cases = [(f"reply: {w}", r) for w, r in shared(rc)] + [(f"packed: {w}", r) for w, r in shared(rp)]
        cases += [("reply: at misaligned", rc(a=arg(at=at.ptr + 2))), ("packed: NULL pk", rp(pk=None)),
                  ("packed: NULL queue", rp(pk=cgck.L4ReplyPack(None, PKAT, PKOFF, None))),
                  ("packed: NULL at", rp(pk=cgck.L4ReplyPack(PKQ, None, PKOFF, None))),
                  ("packed: NULL qoff", rp(pk=cgck.L4ReplyPack(PKQ, PKAT, None, None))),
                  ("packed: at misaligned", rp(pk=cgck.L4ReplyPack(PKQ, PKAT + 2, PKOFF, None))),
                  ("packed: qoff misaligned", rp(pk=cgck.L4ReplyPack(PKQ, PKAT, PKOFF + 1, None))),
                  ("packed: work misaligned", rp(pk=cgck.L4ReplyPack(PKQ, PKAT, PKOFF, PKQ + 2))),
                  ("packed: in.at given", rp(a=arg(at=at.ptr))),
                  ("packed: NULL work above a tile", rp(cnt=4097)), ("packed: n above 0xFFFFFFFF", rp(cnt=1 << 32))]
        for what, r in cases:
            assert r == EINVAL, (what, r)
        blank_ = np.full(65536, 0xEE, np.uint8)
        same(o.get(np.uint8, "outputs"), blank_, "outputs after the refused calls")
        # n == 0 returns 0, launches nothing (the last kernel's name stays) and writes nothing
        engine.l4_desc(fr.ptr, dd.ptr, n, cls=o.ptr + 60000)
        before = engine.last_kernel
        assert before.startswith("l4d_kernel")
        assert rc(cnt=0) == 0 and rc(cnt=0, a=arg(desc=None, seg=None)) == 0 and rp(cnt=0) == 0
        engine.sync()
        assert engine.last_kernel == before
        blank_[60000:60000 + n] = o.get(np.uint8, "outputs")[60000:60000 + n]
        same(o.get(np.uint8, "outputs"), blank_, "outputs after n == 0")
        # the template's IP6 bit is ignored, and the same arguments with n > 0 are accepted
        assert rc(a=arg(link_flags=3)) == 0 and engine.last_kernel == kernel_of(ALL)
        got = o.get(np.uint8, "outputs")
        e = R.reply(b.buf, b.desc, b.seg, LB.LINK, vm=7)
        same(got[:32 * n], e["seg"].view(np.uint8), "seg")
        same(got[8192:8192 + 48 * n], e["flow"].view(np.uint8), "flow")
        same(got[16384:16384 + n], e["cls"], "cls")
        same(got[24576:24576 + n], e["queue"], "queue")
        same(got[32768:32768 + 4 * R.NCOUNT].view(np.uint32), np.uint32(0xEEEEEEEE) + e["count"], "count (running from 0xEEEEEEEE)")
        same(got[32768 + 4 * R.NCOUNT:40960], blank_[32768 + 4 * R.NCOUNT:40960], "the words past count[8)")
        same(got[40960:60000], blank_[40960:60000], "the packed form's arrays")
        fr.check()
    finally:
        for x in (fr, dd, sg, o, at):
            x.free()
