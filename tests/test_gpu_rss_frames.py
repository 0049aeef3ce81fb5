"""Per-frame Toeplitz RSS hashes of receive bursts (rssf_kernel, cgck_rssf.hip)
through cgck_rss_strided, cgck_rss_desc and cgck_rss_desc_host.  Every frame of
every batch is compared with the referee (tests/rssref.py over the oracle's
port) or the reference-made fixture (tests/golden/rss_frames.json), never with
the library itself: hash, kind, queue and the queue counters by exact equality.
The referee hashes each batch once per hf; a masked hash and a queue id follow
from its full hash by the contract (hash & mask, then % queue_num)."""
import ctypes

import numpy as np
import pytest

import cgck
import ip6ref
import rssbatches as RB
import rssref
import rxcorpus
from conftest import load_golden

pytestmark = pytest.mark.gpu

RSSF = "rssf_kernel<"
EINVAL = -22
TCP, UDP = cgck.RSS_TCP, cgck.RSS_UDP
HFS = (0, TCP, TCP | UDP)
FULL = 0xFFFFFFFF
ALL = ("hash", "kind", "queue", "qcount")
SEED = np.arange(128, dtype=np.uint32) * 3 + 5       # qcount before the call: running counters


@pytest.fixture(scope="module")
def key():
    return np.frombuffer(bytes.fromhex(load_golden("rss_frames.json")["key"]), np.uint8).copy()


class Burst:
    """A host batch uploaded once: frames, descriptors (at +0 and +4 of a
    16-byte boundary) and output arrays sized for it."""

    def __init__(self, eng, buf, desc):
        self.eng, self.n, self.buf = eng, len(desc), buf
        n = self.n
        self.d = cgck.DeviceBuffer(max(buf.nbytes, 16))
        self.dd = cgck.DeviceBuffer(2 * desc.nbytes + 64)
        self.at = (0, (desc.nbytes + 15) // 16 * 16 + 16 + 4)
        self.o = {"hash": cgck.DeviceBuffer(4 * n), "kind": cgck.DeviceBuffer(n), "queue": cgck.DeviceBuffer(n),
                  "qcount": cgck.DeviceBuffer(4 * 128)}
        self.d.upload(buf, stream=eng.stream)
        for a in self.at:
            self.dd.upload(desc, off=a, stream=eng.stream)

    def free(self):
        for x in (self.d, self.dd, *self.o.values()):
            x.free()

    def outs(self, names, queue_num):
        """Output arrays preset to values no result has (a frame the kernel skipped shows)."""
        names = [x for x in names if queue_num or x in ("hash", "kind")]
        fill = {"hash": np.full(self.n, 0xDEADBEEF, np.uint32), "kind": np.full(self.n, 0xEE, np.uint8),
                "queue": np.full(self.n, 0xEE, np.uint8), "qcount": SEED.copy()}
        for x in names:
            self.o[x].upload(fill[x], stream=self.eng.stream)
        return names, {x: fill[x].copy() for x in names}

    def fetch(self, names, got):
        for x in names:
            self.o[x].download(got[x], stream=self.eng.stream)
        after = np.zeros_like(self.buf)
        self.d.download(after, stream=self.eng.stream)
        self.eng.sync()
        assert np.array_equal(after, self.buf), "the frame bytes changed"
        return got

    def desc(self, key, hf, mask=FULL, queue_num=0, names=ALL, shift=0, key_size=None):
        names, got = self.outs(names, queue_num)
        spec = cgck.Engine.rss_spec(key, mask, hf, queue_num, key_size)
        self.eng.rss_desc(self.d.ptr, self.dd.ptr + self.at[shift // 4], self.n, spec,
                          **{x: self.o[x].ptr for x in names})
        kern = self.eng.last_kernel
        assert kern == f"rssf_kernel<true, {'true' if queue_num else 'false'}>", kern
        return self.fetch(names, got)


def same(got, exp, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]}, " \
                          f"want {np.asarray(exp)[bad[:5]]}"


def judge(got, ref, mask, queue_num, what):
    """got: the arrays a call returned; ref: the referee's (full hash, kind)."""
    h, kind = ref[0] & np.uint32(mask), ref[1]
    ok = rssref.hashed(kind)
    queue = np.where(ok, h % max(queue_num, 1), rssref.NO_QUEUE).astype(np.uint8)
    assert not np.any(h[~ok]) and not np.any(kind[~ok] & (rssref.RSS_L4 | rssref.RSS_IP6))
    exp = {"hash": h, "kind": kind, "queue": queue}
    for x in got:
        if x == "qcount":
            want = SEED.copy()
            want[:queue_num] += np.bincount(queue[ok], minlength=128).astype(np.uint32)[:queue_num]
            same(got[x], want, f"qcount, {what}")
        else:
            same(got[x], exp[x], f"{x}, {what}")


def refs(port, batch, key, key_size=None):
    buf, _, offs, lens = batch
    return {hf: rssref.expect(port, buf, offs, lens, key, hf, key_size=key_size)[:2] for hf in HFS}


# -- 1. the fixture -------------------------------------------------------------------

def test_fixture(engine, key):
    g = load_golden("rss_frames.json")
    rng = np.random.default_rng(5)
    ms = [np.frombuffer(bytes.fromhex(v["frame"]), np.uint8) for v in g["ms"]]
    frames = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in g["frames"]]
    for lay in (lambda f: RB.packed(rng, f, 0), lambda f: RB.packed(rng, f, 3), lambda f: RB.slotted(rng, f, 2048, 14)):
        b = Burst(engine, *lay(ms)[:2])
        try:
            for hf, field in ((TCP, "tcp"), (TCP | UDP, "tcp"), (0, "ip"), (UDP, "ip")):
                got = b.desc(key, hf, names=("hash", "kind"))
                same(got["hash"], [v[field] for v in g["ms"]], f"published tuples, hf {hf}")
                l4 = cgck.RSS_L4 if hf & TCP else 0
                same(got["kind"], [l4 | (cgck.RSS_IP6 if v["frame"][0] == "6" else 0) for v in g["ms"]], "kinds")
        finally:
            b.free()
        b = Burst(engine, *lay(frames)[:2])
        try:
            for name, s in g["sets"].items():
                got = b.desc(key, s["hf"], queue_num=8)
                judge(got, (np.array(s["hash"], np.uint32), np.array(s["kind"], np.uint8)), FULL, 8, f"fixture {name}")
        finally:
            b.free()


# -- 2. every class, every layout and argument ----------------------------------------

LAYOUTS = ("packed0", "packed1", "packed2", "packed3", "slots")


@pytest.fixture(scope="module")
def class_frames():
    frames = RB.all_classes(np.random.default_rng(31))
    have = set().union(*(RB.tags(f) for f in frames))
    assert RB.REQUIRED <= have, sorted(RB.REQUIRED - have)
    return frames


@pytest.mark.parametrize("layout", LAYOUTS)
def test_classes(engine, port, key, class_frames, layout):
    """The class batch against the referee over descriptor alignment, hf, mask
    and queue_num, every output asked for."""
    rng = np.random.default_rng(100 + LAYOUTS.index(layout))
    batch = RB.slotted(rng, class_frames, 2048, 14) if layout == "slots" else \
        RB.packed(rng, class_frames, int(layout[-1]))
    ref = refs(port, batch, key)
    b = Burst(engine, batch[0], batch[1])
    try:
        for shift in (0, 4):
            for hf in HFS:
                for mask in (FULL, 0x7F):
                    for qn in (0, 1, 3, 8, 128):
                        got = b.desc(key, hf, mask, qn, shift=shift)
                        judge(got, ref[hf], mask, qn, f"{layout} shift {shift} hf {hf} mask {mask:#x} qn {qn}")
    finally:
        b.free()


def test_output_subsets(engine, port, key, class_frames):
    """Each output pointer present or absent (hash == NULL with only queue among them)."""
    rng = np.random.default_rng(120)
    batch = RB.packed(rng, class_frames, 2)
    ref = refs(port, batch, key)[TCP | UDP]
    b = Burst(engine, batch[0], batch[1])
    try:
        for bits in range(1, 16):
            names = tuple(x for i, x in enumerate(ALL) if bits >> i & 1)
            got = b.desc(key, TCP | UDP, 0x7F, 8, names)
            assert tuple(got) == names
            judge(got, ref, 0x7F, 8, f"outputs {names}")
        for names in (("hash",), ("kind",), ("hash", "kind")):
            judge(b.desc(key, TCP | UDP, FULL, 0, names), ref, FULL, 0, f"outputs {names}, no queues")
    finally:
        b.free()


# -- 3. steps and the grid ------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_step_edges(engine, port, key, n):
    rng = np.random.default_rng(200 + n)
    for batch in (RB.packed(rng, RB.fuzz(rng, n), n % 16), RB.slotted(rng, RB.fuzz(rng, n), 2048, 14)):
        ref = refs(port, batch, key)
        b = Burst(engine, batch[0], batch[1])
        try:
            for hf in HFS:
                judge(b.desc(key, hf, FULL, 5), ref[hf], FULL, 5, f"n {n} hf {hf}")
        finally:
            b.free()


def test_many_workgroups(engine, port, key):
    """About 5,000 frames: several workgroups add into the same counters, which
    hold other values before the call."""
    rng = np.random.default_rng(300)
    frames = RB.fuzz(rng, 5003)
    kinds = np.array([rssref.tuple_of(f, len(f), TCP | UDP)[0] for f in frames])
    assert np.count_nonzero(rssref.hashed(kinds)) >= 0.6 * len(frames)
    batch = RB.packed(rng, frames, 6)
    ref = refs(port, batch, key)
    b = Burst(engine, batch[0], batch[1])
    try:
        for hf, qn in ((TCP | UDP, 8), (TCP, 128), (0, 3)):
            got = b.desc(key, hf, FULL, qn)
            judge(got, ref[hf], FULL, qn, f"5003 frames hf {hf} qn {qn}")
            ok = rssref.hashed(got["kind"])
            same(got["qcount"][:qn], SEED[:qn] + np.bincount(got["queue"][ok], minlength=qn).astype(np.uint32),
                 "qcount = seed + bincount(queue[valid])")
    finally:
        b.free()


SLOT, SLOT_L3 = 128, 14                 # three-pass burst: a frame at byte 14 of its 128-byte slot
PERIOD = 64 * 15                        # whole steps, and no divisor of a pass (a power of two)
CAN, CANARY = 64, 0xC3


@pytest.fixture(scope="module")
def slot_period(port, key):
    """One period of the three-pass burst: class and fuzz frames that fit a slot,
    laid out, with the referee's full hash and kind under TCP | UDP."""
    rng = np.random.default_rng(1000)
    frames = [f for f in RB.fuzz(rng, 800) + RB.all_classes(rng) + RB.fuzz(rng, 800) if len(f) <= SLOT - SLOT_L3]
    assert len(frames) >= PERIOD
    frames = frames[:PERIOD]
    buf, desc, offs, lens = RB.slotted(rng, frames, SLOT, SLOT_L3)
    buf = np.ascontiguousarray(buf[:PERIOD * SLOT])            # slotted()'s tail past the last slot is not part of it
    assert np.all((offs & 15) == SLOT_L3) and int((offs + lens).max()) <= buf.nbytes
    h, kind = rssref.expect(port, buf, offs, lens, key, TCP | UDP)[:2]
    return frames, buf, desc, h, kind


def test_three_passes(engine, key, slot_period):
    """Above twice what one pass of the grid covers, plus a step and a frame: every
    wave runs three steps, so both prefetch depths carry real frames and run dry
    (the zero chunk past the end).  The period does not divide a pass, so the
    steps of one wave hold different frames."""
    frames, pbuf, pdesc, h, kind = slot_period
    ok = rssref.hashed(kind)
    assert np.count_nonzero(ok) >= 0.6 * PERIOD
    L4, IP6 = rssref.RSS_L4, rssref.RSS_IP6
    opts4 = [i for i, f in enumerate(frames) if len(f) and f[0] >> 4 == 4 and f[0] & 15 > 5 and kind[i] == L4]
    chain6 = [i for i, f in enumerate(frames) if kind[i] == IP6 | L4 and rssref.walk6(f, len(f))[0] > 40]
    frag = [i for i, f in enumerate(frames) if ok[i] and RB.tags(f) & {"v4_mf", "v4_off", "v6_frag_direct", "v6_frag_chain"}]
    assert opts4 and chain6 and frag, "IPv4 options before the ports, an IPv6 chain before them, a fragment"
    qn = 5
    queue = np.where(ok, h % qn, rssref.NO_QUEUE).astype(np.uint8)

    per_pass = engine.l2_pass_frames()
    assert per_pass % 256 == 0 and per_pass >= 1024 and per_pass % PERIOD != 0 and (2 * per_pass) % PERIOD != 0
    n = 2 * per_pass + 65
    assert n * SLOT < 128_000_000
    reps = (1 << 20) // (PERIOD * SLOT)                # periods a piece: under 1 MiB of frame bytes
    piece = reps * PERIOD
    # Frames and descriptors go up and the results come down a piece at a time:
    # the host never holds an array of the whole burst.
    L, st = cgck.load(), engine.stream
    sizes = {"frames": SLOT * n, "desc": 12 * n, "hash": 4 * n, "kind": n, "queue": n, "qcount": 4 * 128}
    dev = {x: cgck.DeviceBuffer(2 * CAN + sz) for x, sz in sizes.items()}
    try:
        for x, d in dev.items():
            assert L.cgck_memset(d.ptr, CANARY, 2 * CAN + sizes[x], st) == 0
            assert L.cgck_memset(d.ptr + CAN, 0xEE, sizes[x], st) == 0
        dev["qcount"].upload(SEED, off=CAN, stream=st)
        fpiece, dpiece = np.tile(pbuf, reps), np.tile(pdesc, reps)
        dpiece["frame_off"] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(PERIOD * SLOT), PERIOD)
        for a in range(0, n, piece):
            k = min(piece, n - a)
            d = dpiece[:k].copy()
            d["frame_off"] += np.uint64(SLOT * a)
            dev["frames"].upload(fpiece[:SLOT * k], off=CAN + SLOT * a, stream=st)
            dev["desc"].upload(d, off=CAN + 12 * a, stream=st)
        engine.sync()
        base = dev["frames"].ptr + CAN
        assert base % 16 == 0
        engine.rss_desc(base, dev["desc"].ptr + CAN, n, cgck.Engine.rss_spec(key, FULL, TCP | UDP, qn),
                        **{x: dev[x].ptr + CAN for x in ALL})
        assert engine.last_kernel == "rssf_kernel<true, true>", engine.last_kernel

        def fetch(x, off, count, dtype):
            got = np.zeros(count, dtype)
            dev[x].download(got, off=off, stream=st)
            engine.sync()
            return got

        eh, ek, eq = np.tile(h, reps), np.tile(kind, reps), np.tile(queue, reps)
        for a in range(0, n, piece):
            k = min(piece, n - a)
            same(fetch("hash", CAN + 4 * a, k, np.uint32), eh[:k], f"hash, frames {a} ..")
            same(fetch("kind", CAN + a, k, np.uint8), ek[:k], f"kind, frames {a} ..")
            same(fetch("queue", CAN + a, k, np.uint8), eq[:k], f"queue, frames {a} ..")
            same(fetch("frames", CAN + SLOT * a, SLOT * k, np.uint8), fpiece[:SLOT * k], f"frame bytes, frames {a} ..")
            gd = fetch("desc", CAN + 12 * a, k, cgck.DESC_DTYPE)
            assert np.array_equal(gd["ip_len"], dpiece["ip_len"][:k]) and int(gd["frame_off"][k - 1]) == SLOT * (a + k - 1)
        want = SEED.copy()
        want[:qn] += ((n // PERIOD) * np.bincount(queue[ok], minlength=qn)
                      + np.bincount(queue[:n % PERIOD][ok[:n % PERIOD]], minlength=qn)).astype(np.uint32)
        same(fetch("qcount", CAN, 128, np.uint32), want, "qcount")
        for x, d in dev.items():
            for off in (0, CAN + sizes[x]):
                assert np.all(fetch(x, off, CAN, np.uint8) == CANARY), f"{x}: bytes outside the array were written"
    finally:
        for d in dev.values():
            d.free()


# -- 4. the strided form --------------------------------------------------------------

@pytest.mark.parametrize("stride,l3", [(64, 0), (64, 14), (2048, 0), (2048, 14)])
def test_strided(engine, port, key, stride, l3):
    n = 257
    for six in (False, True):
        for ip_len in (40, 44, 60, 64):
            rng = np.random.default_rng(400 + stride + l3 + ip_len + six)
            frames = []
            for i in range(n):
                pr = (6, 17, 6, 17, 1)[i % 5]
                if six:
                    frames.append(ip6ref.packet(rng, ip_len, pr if pr != 1 else 58,
                                                ((RB.H, 8),) if i % 7 == 3 else ((RB.F, 8),) if i % 7 == 5 else ()))
                else:
                    frames.append(RB.v4(rng, ip_len, pr, (5, 5, 6, 5, 10, 5)[i % 6], (0, 0, RB.DF, 0, RB.MF)[i % 5]))
            buf, _, offs, lens = RB.lay(rng, frames, np.arange(n, dtype=np.int64) * stride + l3, tail=0)
            assert buf.nbytes == (n - 1) * stride + l3 + ip_len       # the last frame ends the allocation
            ref = refs(port, (buf, None, offs, lens), key)
            d = cgck.DeviceBuffer(buf.nbytes)
            o = {"hash": cgck.DeviceBuffer(4 * n), "kind": cgck.DeviceBuffer(n), "queue": cgck.DeviceBuffer(n),
                 "qcount": cgck.DeviceBuffer(512)}
            try:
                d.upload(buf, stream=engine.stream)
                for hf, qn in ((TCP | UDP, 8), (TCP, 0), (0, 3)):
                    names = ALL if qn else ALL[:2]
                    got = {"hash": np.zeros(n, np.uint32), "kind": np.zeros(n, np.uint8),
                           "queue": np.zeros(n, np.uint8), "qcount": SEED.copy()}
                    got = {x: got[x] for x in names}
                    if qn:
                        o["qcount"].upload(SEED, stream=engine.stream)
                    engine.rss_strided(d.ptr, n, stride, l3, ip_len, cgck.Engine.rss_spec(key, 0x7F, hf, qn),
                                       **{x: o[x].ptr for x in names})
                    assert engine.last_kernel == f"rssf_kernel<false, {'true' if qn else 'false'}>"
                    for x in names:
                        o[x].download(got[x], stream=engine.stream)
                    engine.sync()
                    judge(got, ref[hf], 0x7F, qn, f"strided {stride}+{l3} ip_len {ip_len} v{6 if six else 4} hf {hf}")
            finally:
                for x in (d, *o.values()):
                    x.free()


# -- 5. one lane of a step in the second load round, and the reverse ------------------

@pytest.mark.parametrize("kind", ["alt", "runs", "one6", "one4"])
def test_patterns(engine, port, key, kind):
    rng = np.random.default_rng(500 + len(kind))
    frames = RB.pattern(rng, kind, 200)
    t = [rssref.tuple_of(f, len(f), TCP | UDP)[0] for f in frames]
    assert all(k & rssref.RSS_L4 for k in t), "every frame of a pattern hashes its ports"
    for batch in (RB.packed(rng, frames, 0), RB.packed(rng, frames, 9), RB.slotted(rng, frames, 2048, 14)):
        ref = refs(port, batch, key)
        b = Burst(engine, batch[0], batch[1])
        try:
            for hf in (TCP | UDP, TCP):
                judge(b.desc(key, hf, FULL, 8), ref[hf], FULL, 8, f"{kind} hf {hf}")
        finally:
            b.free()


# -- 6. keys --------------------------------------------------------------------------

@pytest.mark.parametrize("size", [40, 52, 16, 2])
def test_key_sizes(engine, port, size):
    rng = np.random.default_rng(600 + size)
    k = rng.integers(0, 256, max(size, 4), dtype=np.uint8)     # key[0..3] is always read
    batch = RB.packed(rng, RB.fuzz(rng, 300), 1)
    ref = refs(port, batch, k, key_size=size)
    b = Burst(engine, batch[0], batch[1])
    try:
        for hf in HFS:
            judge(b.desc(k, hf, FULL, 8, key_size=size), ref[hf], FULL, 8, f"key size {size} hf {hf}")
    finally:
        b.free()


def test_table_growth(engine, port, key):
    """One context: 12-byte tuples (tables for 12 positions), frames (36), the
    tuples again under another key (12 again), frames again under that key."""
    rng = np.random.default_rng(700)
    eng = cgck.Engine(0)
    key2 = rng.integers(0, 256, 40, dtype=np.uint8)
    tup = rng.integers(0, 256, 12 * 1000, dtype=np.uint8)
    frames = [ip6ref.packet(rng, 64 + i % 9, (6, 17)[i % 2], ((RB.H, 8),) if i % 4 == 0 else ()) for i in range(300)]
    batch = RB.packed(rng, frames, 0)
    dt, dh = cgck.DeviceBuffer(tup.nbytes), cgck.DeviceBuffer(4000)
    b = Burst(eng, batch[0], batch[1])
    try:
        dt.upload(tup, stream=eng.stream)
        for k in (key, key2):
            eng.toeplitz(dt.ptr, 1000, 12, 12, k, dh.ptr)
            h = np.zeros(1000, np.uint32)
            dh.download(h, stream=eng.stream)
            eng.sync()
            same(h, port.toeplitz_batch(tup, 1000, 12, 12, k), "12-byte tuples")
            ref = refs(port, batch, k)[TCP | UDP]
            assert np.all(ref[1] == (rssref.RSS_IP6 | rssref.RSS_L4))
            judge(b.desc(k, TCP | UDP, FULL, 8), ref, FULL, 8, "IPv6 frames after 12-byte tuples")
    finally:
        for x in (dt, dh):
            x.free()
        b.free()
        eng.close()


# -- 7. nothing outside a frame matters -----------------------------------------------

def test_bytes_outside_frames(engine, port, key, class_frames):
    rng = np.random.default_rng(800)
    frames = class_frames + RB.pattern(rng, "alt", 64)
    gaps = np.cumsum([0] + [len(f) + 1 + i % 23 for i, f in enumerate(frames)])[:-1]      # 1..23 bytes between frames
    for batch in (RB.slotted(rng, frames, 2048, 14), RB.lay(rng, frames, gaps)):
        buf, desc, offs, lens = batch
        ref = refs(port, batch, key)[TCP | UDP]
        res = []
        for other in (buf, RB.refill(rng, buf, offs, lens), RB.refill(rng, buf, offs, lens)):
            b = Burst(engine, other, desc)
            try:
                res.append(b.desc(key, TCP | UDP, FULL, 8))
            finally:
                b.free()
        judge(res[0], ref, FULL, 8, "first filler")
        for r in res[1:]:
            for x in ALL:
                same(r[x], res[0][x], f"{x} under another filler")


# -- 8. the host form -----------------------------------------------------------------

def test_desc_host(engine, port, key):
    """Pageable memory, registered memory, and a burst server open: the referee's
    values, the frame bytes unchanged, the host counters incremented."""
    rng = np.random.default_rng(900)
    buf, desc, offs, lens = RB.packed(rng, RB.fuzz(rng, 700), 0)
    ref = refs(port, (buf, desc, offs, lens), key)
    L = cgck.load()
    raw, ring, size = rxcorpus.registered_copy(buf)
    for mode in ("pageable", "registered", "server"):
        mem = ring if mode == "registered" else buf.copy()
        if mode == "registered":
            assert L.cgck_host_register(ring.ctypes.data, size) == 0
        if mode == "server":
            engine.burst_open(max_pkts=2048, max_bytes=4 << 20)
        try:
            for hf, qn in ((TCP | UDP, 8), (0, 0)):
                n = len(desc)
                got = {"hash": np.full(n, 0xDEADBEEF, np.uint32), "kind": np.full(n, 0xEE, np.uint8)}
                if qn:
                    got.update(queue=np.full(n, 0xEE, np.uint8), qcount=SEED.copy())
                engine.rss_desc_host(mem[:buf.nbytes], desc, cgck.Engine.rss_spec(key, 0x7F, hf, qn), **got)
                assert engine.last_kernel.startswith(RSSF), (mode, engine.last_kernel)
                judge(got, ref[hf], 0x7F, qn, f"desc_host {mode} hf {hf}")
                same(mem[:buf.nbytes], buf, f"desc_host bytes, {mode}")
        finally:
            if mode == "server":
                engine.burst_close()
            if mode == "registered":
                assert L.cgck_host_unregister(ring.ctypes.data) == 0
    del ring, raw


# -- 9. arguments ---------------------------------------------------------------------

def test_arguments(engine, key):
    L = cgck.load()
    n = 4
    buf = np.zeros(4096, np.uint8)
    buf[::64] = 0x45
    desc = np.zeros(n, cgck.DESC_DTYPE)
    desc["frame_off"] = np.arange(n) * 64
    desc["ip_len"] = 64
    d, dd, o = cgck.DeviceBuffer(4096), cgck.DeviceBuffer(64), cgck.DeviceBuffer(1024)
    host = np.zeros(256, np.uint32)
    ctx, by = engine.ctx, ctypes.byref
    R, spec = cgck.RssRes, cgck.Engine.rss_spec

    def calls(c, base, dsc, sp, rs, cnt=n):
        """The three entry points with the same spec / res (the host form over host arrays)."""
        hrs = None if rs is None else by(R(*(host.ctypes.data if x else None for x in (rs.hash, rs.kind, rs.queue, rs.qcount))))
        return (L.cgck_rss_strided(c, base, cnt, 64, 0, 64, sp, None if rs is None else by(rs), None),
                L.cgck_rss_desc(c, base, dsc, cnt, sp, None if rs is None else by(rs), None),
                L.cgck_rss_desc_host(c, None if base is None else buf.ctypes.data, buf.nbytes,
                                     None if dsc is None else desc.ctypes.data, cnt, sp, hrs))

    try:
        d.upload(buf, stream=engine.stream)
        dd.upload(desc, stream=engine.stream)
        engine.sync()
        good, res = spec(key), R(o.ptr, None, None, None)
        nokey = cgck.RssSpec(None, 40, FULL, 0, 0)
        for what, got in (
                ("NULL ctx", calls(None, d.ptr, dd.ptr, by(good), res)),
                ("NULL spec", calls(ctx, d.ptr, dd.ptr, None, res)),
                ("NULL res", calls(ctx, d.ptr, dd.ptr, by(good), None)),
                ("NULL key", calls(ctx, d.ptr, dd.ptr, by(nokey), res)),
                ("NULL base", calls(ctx, None, dd.ptr, by(good), res)),
                ("NULL base, n 0", calls(ctx, None, dd.ptr, by(good), res, 0)),
                ("no output", calls(ctx, d.ptr, dd.ptr, by(good), R(None, None, None, None))),
                ("hf bit 2", calls(ctx, d.ptr, dd.ptr, by(spec(key, hf=4)), res)),
                ("hf bit 31", calls(ctx, d.ptr, dd.ptr, by(spec(key, hf=TCP | 1 << 31)), res)),
                ("queue_num 129", calls(ctx, d.ptr, dd.ptr, by(spec(key, queue_num=129)), R(o.ptr, None, o.ptr + 512, None))),
                ("queue without queue_num", calls(ctx, d.ptr, dd.ptr, by(good), R(o.ptr, None, o.ptr + 512, None))),
                ("qcount without queue_num", calls(ctx, d.ptr, dd.ptr, by(good), R(None, None, None, o.ptr)))):
            assert got == (EINVAL,) * 3, (what, got)
        # with n > 0 a NULL desc (the strided form has none)
        assert calls(ctx, d.ptr, None, by(good), res)[1:] == (EINVAL, EINVAL)
        assert L.cgck_rss_strided(ctx, d.ptr, 1, 1 << 17, 0, 65536, by(good), by(res), None) == EINVAL
        far = desc.copy()
        far["frame_off"][3] = buf.nbytes - 63
        hres = R(host.ctypes.data, None, None, None)
        assert L.cgck_rss_desc_host(ctx, buf.ctypes.data, buf.nbytes, far.ctypes.data, n, by(good), by(hres)) == EINVAL
        far["frame_off"][3] = buf.nbytes - 64
        assert L.cgck_rss_desc_host(ctx, buf.ctypes.data, buf.nbytes, far.ctypes.data, n, by(good), by(hres)) == 0
        # n == 0 returns 0 and launches nothing (the last kernel's name stays)
        assert L.cgck_strided(ctx, d.ptr, n, 64, 0, 64, cgck.GEN_BOTH, o.ptr, None, None, None) == 0
        engine.sync()
        before = engine.last_kernel
        assert not before.startswith(RSSF)
        assert calls(ctx, d.ptr, dd.ptr, by(good), res, 0) == (0, 0, 0)
        assert calls(ctx, d.ptr, None, by(good), res, 0) == (0, 0, 0)
        assert engine.last_kernel == before
        assert calls(ctx, d.ptr, dd.ptr, by(spec(key, queue_num=128)), R(o.ptr, None, o.ptr + 512, None)) == (0, 0, 0)
        engine.sync()
        assert engine.last_kernel.startswith(RSSF)
    finally:
        for x in (d, dd, o):
            x.free()
