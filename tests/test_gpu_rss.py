"""GPU parity of the Toeplitz RSS row: the gfx950
kernels (cgck_rss.hip, through the C-ABI) against the fixtures made from the
reference's own toeplitz_hash / rss_hash4 (tests/golden/rss.json) and against
the oracle restatement on the same bytes.  Integer work: bit-exact.  The second
half takes cgck_toeplitz and cgck_dst_cache to their kernels' edges under canaries
(alignment, group and pass edges, the table cache, caps on tile edges, the
argument rules)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import cgck
import toepbatches as TB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    with open(os.path.join(GOLDEN, "rss.json")) as f:
        return json.load(f)


def hexa(s):
    return np.frombuffer(bytes.fromhex(s), np.uint8).copy()


def test_dropin_ms_vectors(engine, g):
    key = hexa(g["freebsd_rss_key"])
    for v in g["ms_vectors"]:
        d = hexa(v["data_hex"])
        assert cgck.toeplitz_hash(d, key) == v["ipv4_tcp"]
        assert cgck.toeplitz_hash(d, key, 8) == v["ipv4"]
        assert cgck.rss_hash4(v["laddr"], v["faddr"], v["lport"], v["fport"], key) == v["rss_hash4"]


def test_dropin_grid(engine, g):
    t = g["toeplitz_grid"]
    buf, key = hexa(t["data_hex"]), hexa(t["key_hex"])
    for ks, row in zip(t["key_sizes"], t["hash"]):
        got = [cgck.toeplitz_hash(buf, key, c, ks) for c in t["cnts"]]
        assert got == row, f"key_size {ks}"


def test_dropin_negative_cnt(engine, g):
    key = hexa(g["freebsd_rss_key"])
    assert cgck.toeplitz_hash(np.zeros(4, np.uint8), key, -3) == 0


def run_batch(engine, host, n, stride, cnt, key, mask=0xFFFFFFFF, off=0, key_size=None):
    d = cgck.DeviceBuffer(max(host.nbytes + off, 16))
    o = cgck.DeviceBuffer(4 * max(n, 1))
    d.upload(host, off=off, stream=engine.stream)
    engine.toeplitz(d.ptr + off, n, stride, cnt, key, o.ptr, mask=mask, key_size=key_size)
    out = np.zeros(n, np.uint32)
    o.download(out, stream=engine.stream)
    engine.sync()
    return out


def test_batch_tuples12(engine, g):
    key = hexa(g["freebsd_rss_key"])
    d = hexa(g["tuples12"]["data_hex"])
    out = run_batch(engine, d, 4096, 12, 12, key)
    assert out.tolist() == g["tuples12"]["hash"]
    out7 = run_batch(engine, d, 4096, 12, 12, key, mask=0x7F)
    assert np.array_equal(out7, out & 0x7F)


@pytest.mark.parametrize("n,stride,cnt,off,ks", [
    (1000, 16, 12, 0, 40),      # padded records, dword path
    (777, 36, 36, 0, 52),       # IPv6 4-tuple, dword path
    (513, 13, 13, 0, 40),       # byte path, odd stride
    (300, 12, 12, 1, 40),       # misaligned base: byte path
    (200, 40, 40, 0, 64),       # table past the LDS limit: global-table path
    (50, 128, 100, 0, 16),      # long records, short key (zeros shifted in)
    (64, 12, 12, 0, 2),         # key_size < 4 still reads key[0..3]
    (33, 0, 12, 0, 40),         # stride 0: every record the same bytes
    (100, 8, 0, 0, 40),         # cnt 0: hash 0
])
def test_batch_shapes(engine, port, n, stride, cnt, off, ks):
    rng = np.random.default_rng(n * 7 + cnt)
    host = rng.integers(0, 256, max(n * stride, cnt, 1), dtype=np.uint8)
    key = rng.integers(0, 256, max(ks, 4), dtype=np.uint8)
    out = run_batch(engine, host, n, stride, cnt, key, off=off, key_size=ks)
    exp = port.toeplitz_batch(host, n, stride, cnt, key, key_size=ks)
    assert np.array_equal(out, exp)


@pytest.mark.parametrize("mask", [0xFFFFFFFF, 0x7F])
def test_batch_dense_ring_wrap(engine, port, mask):
    """The default dense-tuple kernel (toeplitz12x4_ab_kernel<12>, one block per
    CU) over more 256-group chunks than its register ring holds per block, a
    partial last chunk and an n % 4 tail handed to the per-record kernel:
    n = 4*256*CUs*13 + 4*37 + 3 with CUs = 256 (MI355X), compared in full."""
    n = 4 * 256 * 256 * 13 + 4 * 37 + 3
    rng = np.random.default_rng(1213)
    host = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    key = rng.integers(0, 256, 40, dtype=np.uint8)
    out = run_batch(engine, host, n, 12, 12, key, mask=mask)
    exp = port.toeplitz_batch(host, n, 12, 12, key, mask=mask)
    assert np.array_equal(out, exp)


def test_batch_empty(engine, g):
    key = hexa(g["freebsd_rss_key"])
    engine.toeplitz(None, 0, 12, 12, key, None)
    engine.sync()


def test_key_switch(engine, g):
    """The context's cached tables follow the key of each call."""
    d = hexa(g["tuples12"]["data_hex"])
    k1 = hexa(g["freebsd_rss_key"])
    k2 = hexa(g["keys"]["random52"])
    a1 = run_batch(engine, d, 4096, 12, 12, k1)
    b = run_batch(engine, d, 4096, 12, 12, k2)
    a2 = run_batch(engine, d, 4096, 12, 12, k1)
    assert np.array_equal(a1, a2) and not np.array_equal(a1, b)
    assert a1.tolist() == g["tuples12"]["hash"]


def params(g, s):
    key = hexa(g["keys"][s["key"]])
    return cgck.Engine.dst_params(s["laddr"], s["faddr"], s["fport"], s["queue_num"],
                                  s["queue_id"], key)


@pytest.mark.parametrize("idx", range(15))
def test_dst_sets(engine, g, idx):
    s = g["dst_sets"][idx]
    e = engine.dst_cache_host(params(g, s), s["cap"])
    assert len(e) == s["count"], s["name"]
    assert hashlib.sha256(e.tobytes()).hexdigest() == s["sha256"], s["name"]
    if len(e):
        assert e[:32].tobytes().hex() == s["head"]
        assert e[-32:].tobytes().hex() == s["tail"]


def test_dst_device_variant_repeat(engine, g, port):
    """Device out/count, asynchronous, run twice on the same scratch (the
    control and look-back words are re-zeroed per launch)."""
    s = g["dst_sets"][5]
    p = params(g, s)
    out = cgck.DeviceBuffer(16 * s["cap"])
    cnt = cgck.DeviceBuffer(4)
    for _ in range(2):
        out_h = np.zeros(s["cap"], cgck.DST_DTYPE)
        c = np.zeros(1, np.uint32)
        engine.dst_cache(p, out.ptr, s["cap"], cnt.ptr)
        cnt.download(c, stream=engine.stream)
        out.download(out_h, stream=engine.stream)
        engine.sync()
        assert int(c[0]) == s["count"]
        assert hashlib.sha256(out_h[:c[0]].tobytes()).hexdigest() == s["sha256"]


def test_dst_random_configs(engine, port):
    """Random small ranges, queue counts and caps against the restated loop."""
    rng = np.random.default_rng(5)
    for _ in range(12):
        l0 = int(rng.integers(0, 1 << 31))
        f0 = int(rng.integers(0, 1 << 31))
        nl, nf = int(rng.integers(1, 3)), int(rng.integers(1, 90))
        qn, qi = int(rng.integers(0, 20)), int(rng.integers(0, 20))
        if rng.integers(0, 4) == 0:
            qi = 128 + int(rng.integers(0, 100))
        cap = int(rng.integers(1, 400000))
        fport = int(rng.integers(0, 1 << 16))
        key = rng.integers(0, 256, 40, dtype=np.uint8)
        exp = port.dst_cache(l0, l0 + nl - 1, f0, f0 + nf - 1, fport, qn, qi, key, cap)
        got = engine.dst_cache_host(cgck.Engine.dst_params((l0, l0 + nl - 1), (f0, f0 + nf - 1),
                                                           fport, qn, qi, key), cap)
        assert np.array_equal(got, exp), (l0, nl, f0, nf, qn, qi, cap)


def test_dst_errors(engine, g):
    s = g["dst_sets"][0]
    with pytest.raises(cgck.CgckError, match="cap"):
        engine.dst_cache_host(params(g, s), 0)
    bad = dict(s, laddr=[s["laddr"][1] + 1, s["laddr"][1]])
    with pytest.raises(cgck.CgckError, match="min > max"):
        engine.dst_cache_host(params(g, bad), 10)


@pytest.mark.slow
def test_batch_full_size_sample(engine, g, port):
    """16M dense 12-byte tuples (the bench shape): device output checked on a
    strided 1/256 sample plus the first 4096 against the restatement."""
    n = 16 << 20
    key = hexa(g["freebsd_rss_key"])
    d = cgck.DeviceBuffer(n * 12)
    o = cgck.DeviceBuffer(4 * n)
    engine.synth_strided(d.ptr, n * 12 // 1500, 1500, 1500, 77)   # random bytes (tail too)
    engine.toeplitz(d.ptr, n, 12, 12, key, o.ptr)
    host = np.zeros(n * 12, np.uint8)
    out = np.zeros(n, np.uint32)
    d.download(host, stream=engine.stream)
    o.download(out, stream=engine.stream)
    engine.sync()
    idx = np.concatenate([np.arange(4096), np.arange(4096, n, 256)])
    sub = np.ascontiguousarray(host.reshape(n, 12)[idx]).reshape(-1)
    exp = port.toeplitz_batch(sub, len(idx), 12, 12, key)
    assert np.array_equal(out[idx], exp)


# ---------------------------------------------------------------------------------------
# Kernel edges (inputs and the dispatch rule: tests/toepbatches.py; the conditions they
# rest on: tests/test_rss_edges_cpu.py).  Every output lies between canary bytes and
# starts as 0xEE, every comparison is exact and against the referee (oracle.port()),
# never the library, and the kernel name of every launch is asserted.
# ---------------------------------------------------------------------------------------

EINVAL = -22
CAN, CANARY = 64, 0xC3
DST_KERNEL = {True: "dst_cache_kernel<true>", False: "dst_cache_kernel<false>"}


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


@pytest.fixture(scope="module")
def fkey(g):
    return hexa(g["keys"]["freebsd"])


def hash_case(eng, port, case, key, mask=0xFFFFFFFF, key_size=None, seed=1):
    """One cgck_toeplitz call over a case of tests/toepbatches.py: data in a plain
    allocation of exactly the records' bytes (plus the shift), out as 0xEE between
    canaries.  Checks the canaries, out against the referee, the kernel name and
    that data reads back unchanged."""
    n, stride, cnt, dshift, oshift = case
    what = f"n {n} stride {stride} cnt {cnt} data +{dshift} out +{oshift} mask {mask:#x}"
    host = TB.records(n, stride, cnt, seed)
    assert host.nbytes == (n - 1) * stride + cnt
    d = cgck.DeviceBuffer(host.nbytes + dshift)
    o = Guarded(eng, 4 * n, 0xEE, oshift)
    try:
        assert d.ptr % 16 == 0 and (o.ptr - oshift) % 16 == 0
        d.upload(host, off=dshift, stream=eng.stream)
        eng.toeplitz(d.ptr + dshift, n, stride, cnt, key, o.ptr, mask=mask, key_size=key_size)
        kern = eng.last_kernel
        got = o.get(np.uint32, what)
        after = np.zeros_like(host)
        d.download(after, off=dshift, stream=eng.stream)
        eng.sync()
    finally:
        d.free()
        o.free()
    same(got, port.toeplitz_batch(host, n, stride, cnt, key, mask=mask, key_size=key_size), f"out, {what}")
    assert kern == TB.expected_kernel(n, stride, cnt, dshift, oshift), what
    assert np.array_equal(after, host), f"data changed, {what}"
    return kern


# -- 1. cgck_toeplitz: alignment and dispatch --------------------------------------------

@pytest.mark.parametrize("dshift", (0, 4, 8, 12, 1))
def test_hash_alignment_and_dispatch(engine, port, fkey, dshift):
    """Dense 12-byte records at every dword shift of data and out: only (0, 0) may
    take the x4 kernel, whose uint4 loads and stores need both on a 16-byte boundary;
    every other shift runs the whole batch on a per-record kernel."""
    cases = [c for c in TB.ALIGN_CASES if c[3] == dshift]
    assert [c[4] for c in cases] == [0, 4, 8, 12]
    for c in cases:
        kern = hash_case(engine, port, c, fkey, seed=2)
        assert kern == (TB.X4 if (c[3], c[4]) == (0, 0) else TB.B_LDS if dshift == 1 else TB.W3)


# -- 2. the x4 kernel's sizes ------------------------------------------------------------

@pytest.mark.parametrize("n", TB.X4_SIZES)
def test_hash_x4_sizes(engine, port, fkey, n):
    """ng = n / 4 in {1, 2, 255, 256, 257} with every n % 4: a partial last 256-group
    block, one group past a full block, the tail on the per-record kernel; n < 4 has
    no group and runs on toeplitz_kernel<3, true> alone."""
    kern = hash_case(engine, port, (n, 12, 12, 0, 0), fkey, seed=3)
    assert kern == (TB.W3 if n < 4 else TB.X4)


# -- 3. cnt and stride -------------------------------------------------------------------

@pytest.mark.parametrize("cnt,stride", TB.GRID)
def test_hash_cnt_stride_grid(engine, port, fkey, cnt, stride):
    """Around cnt 12 and 36, the LDS limit (35, 36, 37), strides that are no multiple
    of 4, overlapping records, stride 0, cnt 0 and 1."""
    hash_case(engine, port, (TB.GRID_N, stride, cnt, 0, 0), fkey, seed=4)


# -- 4. masks on every kernel ------------------------------------------------------------

@pytest.mark.parametrize("which", range(len(TB.KERNELS)), ids=("x4", "w3", "w9", "lds", "global"))
@pytest.mark.parametrize("mask", TB.MASKS)
def test_hash_masks_every_kernel(engine, port, fkey, mask, which):
    """`& mask` in each of the five kernels on its own (the x4 case has an n % 4 tail,
    which toeplitz_kernel<3, true> masks)."""
    assert hash_case(engine, port, TB.MASK_CASES[which], fkey, mask=mask, seed=5) == TB.KERNELS[which]


# -- 5. a second and third pass of the grid-stride loop ----------------------------------

@pytest.mark.parametrize("stride,cnt", TB.PASS_SHAPES)
def test_hash_three_passes(engine, port, fkey, stride, cnt):
    """n = 2 * (records of one pass) + 257 on each toeplitz_kernel instantiation:
    every lane of the first block runs three passes, the rest two.  Overlapping
    records keep the data at a few MB while every record differs."""
    per_pass, groups = engine.rss_pass()
    assert per_pass >= 8 * 256 and per_pass % (8 * 256) == 0 and groups * 8 == per_pass * 12
    n = TB.pass_n(per_pass)
    kern = hash_case(engine, port, (n, stride, cnt, 0, 0), fkey, seed=6)
    assert kern == {12: TB.W3, 36: TB.W9, 13: TB.B_LDS, 37: TB.B_GLB}[cnt]


# -- 6. the context's table cache --------------------------------------------------------

def test_hash_table_cache(port, g, fkey):
    """rss_prepare reuses the tables when the key bytes and max(key_size, 4) are those
    of the last build and the tables are long enough; cgck_dst_cache shares them and
    reads the host copy.  One context, each call against the referee."""
    eng = cgck.Engine(0)
    try:
        A = TB.key_bytes(40, 1)
        A2 = A.copy()
        A2[39] ^= 0x10
        B = hexa(g["keys"]["random52"])
        K4 = TB.key_bytes(4, 2)
        long, short = (TB.GRID_N, 40, 40, 0, 0), (TB.GRID_N, 12, 12, 0, 0)
        # a late key byte reaches the hash only through the tables of bytes >= 35
        h = [port.toeplitz_batch(TB.records(*long[:3], 7), *long[:3], k) for k in (A, A2)]
        assert not np.array_equal(h[0], h[1])

        def dst(key):
            c = TB.EDGE_CONFIGS[1]
            p = cgck.Engine.dst_params(c["laddr"], c["faddr"], c["fport"], c["queue_num"], c["queue_id"], key)
            got = eng.dst_cache_host(p, 3000)
            assert eng.last_kernel == DST_KERNEL[True]
            exp = TB.referee(port, c, key, 3000)
            assert len(exp) == 3000
            same(got.view(np.uint8), exp.view(np.uint8), "dst_cache_host on the shared tables")

        assert hash_case(eng, port, long, A, seed=7) == TB.B_GLB         # 1. A, cnt 40
        assert hash_case(eng, port, short, A, seed=7) == TB.X4           # 2. A, cnt 12: reuse
        hash_case(eng, port, long, A, key_size=16, seed=7)               # 3. A's bytes, key_size 16
        hash_case(eng, port, short, A, key_size=16, seed=7)
        hash_case(eng, port, long, A, seed=7)                            # 4. A, 40 bytes again
        hash_case(eng, port, long, A2, seed=7)                           # 5. byte 39 flipped
        hash_case(eng, port, long, A, seed=7)
        hash_case(eng, port, short, K4, key_size=3, seed=7)              # 6. key_size 3, then 4: the same stream
        hash_case(eng, port, short, K4, key_size=4, seed=7)
        hash_case(eng, port, long, K4, key_size=4, seed=7)
        hash_case(eng, port, short, A, seed=7)                           # 7. A at cnt 12, then grown to 40
        hash_case(eng, port, long, A, seed=7)
        dst(B)                                                           # 8. another key through dst_cache
        hash_case(eng, port, long, A, seed=7)                            # 9. A, cnt 40, after B's 12-byte tables
        dst(A)                                                           # 10. dst_cache on A's longer tables
        hash_case(eng, port, short, A, mask=0x7F, seed=7)
    finally:
        eng.close()


# -- 7. the cnt limit --------------------------------------------------------------------

def test_hash_cnt_limit(port, fkey):
    """cnt 65536 is the longest record taken (a 64 MiB table, freed with the context);
    65537 is refused before anything is read or written."""
    eng = cgck.Engine(0)
    try:
        assert hash_case(eng, port, (3, 1, TB.MAX_CNT, 0, 0), fkey, seed=8) == TB.B_GLB
        L = cgck.load()
        d = cgck.DeviceBuffer(TB.MAX_CNT + 16)
        o = Guarded(eng, 12, 0xEE)
        rc = L.cgck_toeplitz(eng.ctx, d.ptr, 3, 1, TB.MAX_CNT + 1, fkey.ctypes.data, len(fkey), 0xFFFFFFFF, o.ptr, None)
        assert rc == EINVAL
        assert np.all(o.get(np.uint8, "out of the refused call") == 0xEE)
        d.free()
        o.free()
    finally:
        eng.close()


# -- 8. cgck_toeplitz's argument rules ---------------------------------------------------

def test_hash_arguments(engine, port, fkey):
    L = cgck.load()
    assert hash_case(engine, port, (TB.GRID_N, 40, 37, 0, 0), fkey, seed=9) == TB.B_GLB
    d = cgck.DeviceBuffer(48)
    o = Guarded(engine, 16, 0xEE)
    k, ks = fkey.ctypes.data, len(fkey)

    def rc(ctx, data, n, key, out, cnt=12):
        return L.cgck_toeplitz(ctx, data, n, 12, cnt, key, ks, 0xFFFFFFFF, out, None)

    try:
        assert rc(None, d.ptr, 4, k, o.ptr) == EINVAL
        assert rc(engine.ctx, None, 4, k, o.ptr) == EINVAL
        assert rc(engine.ctx, d.ptr, 4, k, None) == EINVAL
        assert rc(engine.ctx, d.ptr, 4, None, o.ptr) == EINVAL
        assert rc(engine.ctx, d.ptr, 0, None, o.ptr) == EINVAL
        assert rc(engine.ctx, None, 0, None, None) == EINVAL
        assert rc(engine.ctx, d.ptr, 4, k, o.ptr, cnt=TB.MAX_CNT + 1) == EINVAL
        assert rc(engine.ctx, None, 0, k, None) == 0                     # nothing to do, nothing launched
        assert rc(engine.ctx, d.ptr, 0, k, o.ptr) == 0
        assert engine.last_kernel == TB.B_GLB, "a refused or empty call renamed the last kernel"
        assert np.all(o.get(np.uint8, "out of the refused and empty calls") == 0xEE)
    finally:
        d.free()
        o.free()


# -- 9. cgck_dst_cache, the device variant -----------------------------------------------

def dst_case(eng, c, key, cap, exp):
    """cgck_dst_cache twice on one context (the scratch is re-zeroed per launch), out
    as 16 * cap bytes of 0xEE and count as 0xEEEEEEEE, both between canaries: count,
    the entries, the untouched rest of out and the kernel name, against `exp` (the
    referee's entries under the same cap)."""
    what = f"{c['name']} cap {cap}"
    filt = c["queue_id"] < 128 and c["queue_num"] > 1
    p = cgck.Engine.dst_params(c["laddr"], c["faddr"], c["fport"], c["queue_num"], c["queue_id"], key)
    out, cnt = Guarded(eng, 16 * cap, 0xEE), Guarded(eng, 4, 0xEE)
    before = eng.last_kernel
    try:
        assert out.ptr % 16 == 0
        for run in range(2):
            eng.dst_cache(p, out.ptr, cap, cnt.ptr)
            assert eng.last_kernel == (DST_KERNEL[filt] if TB.tuples(c) else before), what
            count = int(cnt.get(np.uint32, f"count, {what}")[0])
            got = out.get(np.uint8, f"out, {what}")
            assert count == len(exp), (what, run, count, len(exp))
            same(got[:16 * count], exp.view(np.uint8).reshape(-1), f"entries, {what}, run {run}")
            assert np.all(got[16 * count:] == 0xEE), f"out[count:cap] was written, {what}, run {run}"
            out.put(np.full(16 * cap, 0xEE, np.uint8))
            cnt.put(np.full(4, 0xEE, np.uint8))
    finally:
        out.free()
        cnt.free()


@pytest.mark.parametrize("c", TB.EDGE_CONFIGS, ids=lambda c: c["name"])
def test_dst_caps_on_tile_edges(engine, port, fkey, c):
    """cap equal to a tile's inclusive count, one below and one above, for the tiles
    that end at tuple 8192, 16384 and 131072, and around the whole enumeration: who
    writes *count, when the stop flag rises, and the `at < cap` guard in the tile that
    straddles cap."""
    full = TB.referee(port, c, fkey)
    caps = TB.edge_caps(full, c["laddr"][0], c["faddr"][0], c["nf"])
    assert len(caps) >= 10 and caps[-1] == len(full) + 1
    for cap in caps:
        dst_case(engine, c, fkey, cap, full[:cap])


@pytest.mark.parametrize("c", TB.NF_CONFIGS + TB.LARGE_CONFIGS, ids=lambda c: c["name"])
def test_dst_nf_and_large(engine, port, fkey, c):
    """nf around the cursor's 64-tuple step (1, 2, 3, 32, 128; 60536 and 60537, where
    64 tuples never carry past one port), and nf 70000: 4 237 520 000 tuples in half
    a million tiles, 64-bit tile bases against a 32-bit cursor, stopped early."""
    exp = TB.referee(port, c, fkey, c["cap"])
    assert len(exp) == c["cap"]
    dst_case(engine, c, fkey, c["cap"], exp)


@pytest.mark.parametrize("c", TB.EMPTY_CONFIGS, ids=lambda c: c["name"])
def test_dst_empty(engine, port, fkey, c):
    """n == 0 in the loop's 32-bit arithmetic (nf == 0, nl == 0): the call returns 0,
    a stale count becomes 0 and out is left alone."""
    assert TB.tuples(c) == 0
    dst_case(engine, c, fkey, c["cap"], TB.referee(port, c, fkey, c["cap"]))


def test_dst_arguments(engine, fkey):
    L = cgck.load()
    c = TB.EDGE_CONFIGS[1]
    mk = cgck.Engine.dst_params
    good = mk(c["laddr"], c["faddr"], c["fport"], 4, 1, fkey)
    nokey = mk(c["laddr"], c["faddr"], c["fport"], 4, 1, None)
    lrev = mk((c["laddr"][1], c["laddr"][0]), c["faddr"], c["fport"], 4, 1, fkey)
    frev = mk(c["laddr"], (c["faddr"][1], c["faddr"][0]), c["fport"], 4, 1, fkey)
    out, cnt = Guarded(engine, 16 * 8, 0xEE), Guarded(engine, 4, 0xEE)
    before = engine.last_kernel

    def rc(ctx, p, o, cap, n):
        return L.cgck_dst_cache(ctx, None if p is None else ctypes.byref(p), o, cap, n, None)

    try:
        assert rc(None, good, out.ptr, 8, cnt.ptr) == EINVAL
        assert rc(engine.ctx, None, out.ptr, 8, cnt.ptr) == EINVAL
        assert rc(engine.ctx, good, None, 8, cnt.ptr) == EINVAL
        assert rc(engine.ctx, good, out.ptr, 8, None) == EINVAL
        assert rc(engine.ctx, good, out.ptr, 0, cnt.ptr) == EINVAL
        assert rc(engine.ctx, good, out.ptr, 1 << 31, cnt.ptr) == EINVAL
        assert rc(engine.ctx, nokey, out.ptr, 8, cnt.ptr) == EINVAL
        assert rc(engine.ctx, lrev, out.ptr, 8, cnt.ptr) == EINVAL
        assert rc(engine.ctx, frev, out.ptr, 8, cnt.ptr) == EINVAL
        assert engine.last_kernel == before
        assert np.all(out.get(np.uint8, "out of the refused calls") == 0xEE)
        assert np.all(cnt.get(np.uint8, "count of the refused calls") == 0xEE)
    finally:
        out.free()
        cnt.free()
