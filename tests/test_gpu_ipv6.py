"""CGCK_IP6 on the GPU: the group kernel's full semantics (cksum6_kernel), the
fast families' IPv6 variants (dstr6_kernel, lpd6_kernel, lpa6_kernel), the
dispatcher's routing, the host path and the error returns.  Every comparison
is against the oracle (tests/ip6ref.py: oracle.port().in_cksum over
pseudo-header || segment) or the reference-made fixture
(tests/golden/ipv6.json), never against the library itself."""
import numpy as np
import pytest

import cgck
import ip6ref
from conftest import load_golden
from test_gpu_parity import page_ring

pytestmark = pytest.mark.gpu

LENS = (40, 41, 48, 60, 61, 64, 575, 576, 1279, 1280, 1499, 1500, 1514)
NHS = (6, 17, 58, 59, 253)
GEN6 = cgck.GEN_BOTH | cgck.IP6
ZERO6 = cgck.GEN_BOTH | cgck.ZERO_FIELDS | cgck.IP6
FILL6 = cgck.FILL_BOTH | cgck.IP6
TOY6 = cgck.VERIFY_TOY | cgck.IP6


@pytest.fixture
def pinned(engine):
    """The session's engine pinned to a family (cgck_ctx_set_kernel) for one
    test; no context or stream of this module's own."""
    def get(family):
        engine.set_kernel(family)
        return engine
    yield get
    engine.set_kernel("auto")
    engine.set_desc_len_hint(1500)


def run_desc(eng, buf, desc, flags, want_bad=False):
    """cgck_desc over a host batch: (out, verdict, bytes after, bad[2], kernel)."""
    n = len(desc)
    d = cgck.DeviceBuffer(max(buf.nbytes, 16))
    dd = cgck.DeviceBuffer(max(desc.nbytes, 12))
    o = cgck.DeviceBuffer(4 * n)
    v = cgck.DeviceBuffer(n)
    b = cgck.DeviceBuffer(8)
    d.upload(buf, stream=eng.stream)
    dd.upload(desc, stream=eng.stream)
    b.upload(np.zeros(2, np.uint32), stream=eng.stream)
    eng.desc(d.ptr, dd.ptr, n, flags, o.ptr, v.ptr, b.ptr if want_bad else None)
    kern = eng.last_kernel
    out, ver, bad, after = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(2, np.uint32), np.zeros_like(buf)
    o.download(out, stream=eng.stream)
    v.download(ver, stream=eng.stream)
    b.download(bad, stream=eng.stream)
    if buf.nbytes:
        d.download(after, stream=eng.stream)
    eng.sync()
    for x in (d, dd, o, v, b):
        x.free()
    return out, ver, after, bad, kern


def run_strided(eng, buf, n, stride, l3, ln, flags, verdict=True):
    d = cgck.DeviceBuffer(buf.nbytes)
    o = cgck.DeviceBuffer(4 * n)
    v = cgck.DeviceBuffer(n) if verdict else None
    d.upload(buf, stream=eng.stream)
    eng.strided(d.ptr, n, stride, l3, ln, flags, o.ptr, v.ptr if v else None)
    kern = eng.last_kernel
    out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    o.download(out, stream=eng.stream)
    if v:
        v.download(ver, stream=eng.stream)
    eng.sync()
    for x in (d, o, v):
        if x:
            x.free()
    return out, ver, kern


def same(got, exp, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]}, " \
                          f"want {np.asarray(exp)[bad[:5]]}"


# -- group kernel, descriptors ------------------------------------------------

@pytest.fixture(scope="module")
def fixture_batch():
    """All fixture cases in one descriptor batch, frames back to back."""
    cases = load_golden("ipv6.json")["cases"]
    frames = [np.frombuffer(bytes.fromhex(c["hex"]), np.uint8) for c in cases]
    offs = np.concatenate(([0], np.cumsum([len(f) for f in frames])[:-1])).astype(np.int64)
    buf = np.concatenate(frames + [np.zeros(64, np.uint8)])
    desc = np.zeros(len(cases), cgck.DESC_DTYPE)
    desc["frame_off"] = offs
    desc["l3_off"] = [c["l3_off"] for c in cases]
    desc["ip_len"] = [c["ip_len"] for c in cases]
    return cases, buf, desc


@pytest.mark.parametrize("hint,family", [(1500, "auto"), (64, "auto"), (354, "auto"), (1500, "lpp"),
                                         (1500, "slot2"), (1500, "lpw"), (1500, "dstr"), (1500, "lpd")])
def test_group_fixture_batch(pinned, fixture_batch, hint, family):
    """The reference-made cases through cgck_desc, whatever family the
    dispatcher or a pin would pick for IPv4: a descriptor batch always ends
    in the group kernel's IPv6 variant."""
    cases, buf, desc = fixture_batch
    eng = pinned(family)
    eng.set_desc_len_hint(hint)
    okc = np.array([c["status"] == "ok" for c in cases])
    blen = np.array([cgck.BAD_LEN if c["status"] == "bad_len" else 0 for c in cases], np.uint8)
    for flags, key, vkey in ((ZERO6, "hi_zero", None), (GEN6, "hi_gen", None), (TOY6, "hi_zero", "verdict_toy"),
                             (TOY6 | cgck.V_UDP_ZERO_SKIP | cgck.V_IP_ZERO_IS_FFFF, "hi_zero",
                              "verdict_toy_udp_skip")):
        out, ver, after, bad, kern = run_desc(eng, buf, desc, flags, want_bad=True)
        assert kern.startswith("cksum6_kernel<"), kern
        exp = np.array([c[key] << 16 for c in cases], np.uint32)
        same(out, exp, f"out, flags {flags:#x}")
        assert not np.any(out[~okc])
        wantv = blen if vkey is None else np.array([c[vkey] for c in cases], np.uint8)
        same(ver, wantv, f"verdict, flags {flags:#x}")
        assert np.array_equal(after, buf)          # nothing stored
        assert bad[0] == 0 and bad[1] == np.count_nonzero(wantv & cgck.BAD_L4)


def cross_batch(rng, n, l3, chains=True):
    """n frames in 1600-byte slots at +l3: every (ip_len, nh) pair of LENS x
    NHS in turn; every 5th frame that has room carries HBH(8), every 11th
    HBH(16) + DestOpt(8)."""
    slot = 1600
    buf = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
    desc = np.zeros(n, cgck.DESC_DTYPE)
    for i in range(n):
        combo = i % (len(LENS) * len(NHS))
        ln, nh = LENS[combo % len(LENS)], NHS[combo // len(LENS)]
        chain = ()
        if chains and i % 11 == 10:
            chain = ((0, 16), (60, 8))
        elif chains and i % 5 == 4:
            chain = ((0, 8),)
        buf[i * slot + l3:i * slot + l3 + ln] = ip6ref.packet(rng, ln, nh, chain)
        desc[i] = (i * slot, l3, ln)
    return buf, desc


@pytest.mark.parametrize("l3", [0, 14, 15, 18])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_group_desc_cross(engine, port, n, l3):
    rng = np.random.default_rng(600 + 31 * n + l3)
    buf, desc = cross_batch(rng, n, l3)
    offs, lens = desc["frame_off"].astype(np.int64) + l3, desc["ip_len"]
    for flags in (GEN6, ZERO6, cgck.L4 | cgck.IP6, cgck.IP | cgck.IP6):
        exp, ever, _ = ip6ref.expect(port, buf, offs, lens, flags)
        out, ver, after, _, kern = run_desc(engine, buf, desc, flags)
        assert kern.startswith("cksum6_kernel<"), kern
        same(out, exp, f"out n {n} l3 {l3} flags {flags:#x}")
        same(ver, ever, f"verdict n {n} l3 {l3} flags {flags:#x}")
        assert np.array_equal(after, buf)


# every group shape (<= 80, <= 256, <= 768, <= 1600, above) and the long-packet loop
@pytest.mark.parametrize("ln", LENS + (200, 2000, 9001))
def test_group_strided(pinned, port, ln):
    eng = pinned("group")
    n = 65
    l3 = (0, 14, 15, 18)[ln % 4]
    stride = ln + l3 + (ln % 7)
    rng = np.random.default_rng(ln)
    buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
    for i in range(n):
        chain = ((0, 8),) if i % 5 == 4 else ((51, 24),) if i % 13 == 12 else ()
        buf[i * stride + l3:i * stride + l3 + ln] = ip6ref.packet(rng, ln, NHS[i % 5], chain)
    offs = np.arange(n, dtype=np.int64) * stride + l3
    for flags in (GEN6, TOY6):
        exp, ever, _ = ip6ref.expect(port, buf, offs, [ln] * n, flags)
        out, ver, kern = run_strided(eng, buf, n, stride, l3, ln, flags)
        assert kern.startswith("cksum6_kernel<"), kern
        same(out, exp, f"out len {ln} flags {flags:#x}")
        same(ver, ever, f"verdict len {ln} flags {flags:#x}")


def test_raw_is_unchanged(engine, port):
    """CGCK_RAW | CGCK_IP6 is CGCK_RAW: in_cksum of the whole region."""
    rng = np.random.default_rng(5)
    buf, desc = cross_batch(rng, 65, 15)
    exp = np.array([port.in_cksum(buf, int(d["frame_off"]) + 15, int(d["ip_len"])) for d in desc], np.uint32)
    out, ver, _, _, _ = run_desc(engine, buf, desc, cgck.RAW | cgck.IP6)
    same(out, exp, "raw")
    assert not ver.any()


# -- chains ---------------------------------------------------------------------

def test_chains(engine, port):
    rng = np.random.default_rng(77)
    H, D, R, A, F = 0, 60, 43, 51, 44
    spec = [   # (chain, nh, ip_len, status)
        (((H, 8),), 6, 120, ip6ref.OK), (((H, 16), (D, 8)), 17, 121, ip6ref.OK), (((R, 24),), 58, 99, ip6ref.OK),
        (((A, 24),), 6, 130, ip6ref.OK), (((A, 12), (D, 8)), 17, 88, ip6ref.OK),
        (((F, 8),), 6, 100, ip6ref.NO_L4), (((H, 8), (F, 8)), 17, 100, ip6ref.NO_L4),
        (((H, 8), (D, 16)), 6, 49, ip6ref.BADLEN),        # the second header's bytes are past ip_len
        (((H, 8), (D, 16)), 6, 60, ip6ref.BADLEN),        # the L4 region would start past ip_len
        (((H, 8),), 6, 48 + 17, ip6ref.BADLEN),           # the TCP checksum field does not fit
        (((H, 8),) + ((D, 8),) * 7, 17, 200, ip6ref.OK),  # eight headers
        (((H, 8),) + ((D, 8),) * 8, 17, 200, ip6ref.BADLEN),  # nine
        (((H, 2048),), 6, 40 + 2048 + 41, ip6ref.OK),     # the field far from the header
    ]
    for l3 in (0, 15):
        slot = 2304
        buf = rng.integers(0, 256, len(spec) * slot, dtype=np.uint8)
        desc = np.zeros(len(spec), cgck.DESC_DTYPE)
        for i, (chain, nh, ln, st) in enumerate(spec):
            p = ip6ref.packet(rng, ln, nh, chain)
            assert ip6ref.walk(p, ln)[2] == st, i
            buf[i * slot + l3:i * slot + l3 + ln] = p
            desc[i] = (i * slot, l3, ln)
        offs = desc["frame_off"].astype(np.int64) + l3
        for flags in (ZERO6, FILL6, TOY6):
            exp, ever, eafter = ip6ref.expect(port, buf, offs, desc["ip_len"], flags)
            out, ver, after, bad, _ = run_desc(engine, buf, desc, flags, want_bad=True)
            same(out, exp, f"out l3 {l3} flags {flags:#x}")
            same(ver, ever, f"verdict l3 {l3} flags {flags:#x}")
            same(after, eafter, f"bytes l3 {l3} flags {flags:#x}")
            for i, (_, _, _, st) in enumerate(spec):
                if st != ip6ref.OK:
                    assert out[i] == 0 and ver[i] == (cgck.BAD_LEN if st == ip6ref.BADLEN else 0)
            assert bad[0] == 0


# -- fill, then verify ------------------------------------------------------------

@pytest.mark.parametrize("n,l3", [(63, 14), (257, 15)])
def test_fill_then_verify(engine, port, n, l3):
    rng = np.random.default_rng(n)
    slot = 1600
    buf = rng.integers(0, 256, n * slot + 64, dtype=np.uint8)
    desc = np.zeros(n, cgck.DESC_DTYPE)
    for i in range(n):
        ln, nh = (64, 80, 576, 1279, 1500, 1514)[i % 6], (6, 17, 58)[i % 3]
        chain = ((0, 8),) if i % 4 == 3 and ln > 64 else ()
        p = ip6ref.packet(rng, ln, nh, chain)
        l4, _, st = ip6ref.walk(p, ln)
        assert st == ip6ref.OK
        p[l4 + ip6ref.FIELD[nh]:l4 + ip6ref.FIELD[nh] + 2] = 0      # zeroed fields
        buf[i * slot + l3:i * slot + l3 + ln] = p
        desc[i] = (i * slot, l3, ln)
    offs = desc["frame_off"].astype(np.int64) + l3
    exp, ever, eafter = ip6ref.expect(port, buf, offs, desc["ip_len"], FILL6)
    assert not ever.any() and np.all(exp >> 16)
    out, ver, filled, _, _ = run_desc(engine, buf, desc, FILL6)
    same(out, exp, "fill out")
    assert not ver.any()
    same(filled, eafter, "stored bytes")                  # the oracle's, and nothing else written:
    assert np.array_equal(filled[offs + 10], buf[offs + 10]) and np.array_equal(filled[offs + 11], buf[offs + 11])
    out, ver, after, bad, _ = run_desc(engine, filled, desc, TOY6, want_bad=True)
    assert not ver.any() and bad[0] == 0 and bad[1] == 0
    same(out, exp, "verify out")
    assert np.array_equal(after, filled)
    hit = sorted({0, n // 2, n - 1})
    broken = filled.copy()
    for i in hit:
        broken[offs[i] + desc["ip_len"][i] - 1] ^= 0x40
    out, ver, after, bad, _ = run_desc(engine, broken, desc, TOY6, want_bad=True)
    assert sorted(np.nonzero(ver)[0].tolist()) == hit and np.all(ver[hit] == cgck.BAD_L4)
    assert bad[1] == 3 and bad[0] == 0
    assert np.array_equal(after, broken)                   # verify writes nothing (ip + 10 included)


# -- dstr ---------------------------------------------------------------------------

def synth_ref(port, n, stride, ln, nh, seed):
    buf = port.stream_bytes(0, n * stride, seed)
    ip6ref.stamp_strided(buf, n, stride, ln, nh)
    return buf


@pytest.mark.parametrize("ln,nh", [(1024, 17), (1500, 6)])
@pytest.mark.parametrize("n", [1, 4, 5, 259])
def test_dstr_synth(pinned, port, ln, nh, n):
    """cgck_synth_strided_ip6 frames (regenerated with the oracle's
    stream_bytes) through the pinned dstr family, then the same batch with
    extension headers in every 7th frame."""
    eng = pinned("dstr")
    seed = 0xD6 + n
    d, o, v = cgck.DeviceBuffer(n * ln), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n)
    eng.synth_strided_ip6(d.ptr, n, ln, ln, nh, seed)
    eng.strided(d.ptr, n, ln, 0, ln, GEN6, o.ptr, v.ptr)
    kern = eng.last_kernel
    got, out, ver = np.zeros(n * ln, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    d.download(got, stream=eng.stream)
    o.download(out, stream=eng.stream)
    v.download(ver, stream=eng.stream)
    eng.sync()
    for x in (d, o, v):
        x.free()
    ref = synth_ref(port, n, ln, ln, nh, seed)
    same(got, ref, "synth bytes")
    assert kern.startswith("dstr6_kernel<"), kern
    offs = np.arange(n, dtype=np.int64) * ln
    exp, ever, _ = ip6ref.expect(port, ref, offs, [ln] * n, GEN6)
    same(out, exp, "synth out")
    assert not ver.any()
    # every 7th frame with HBH(8); one each with AH(24) + DestOpt(8), a Fragment
    # header and a header running past the frame (BAD_LEN)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 7):
        ref[i * ln:(i + 1) * ln] = ip6ref.packet(rng, ln, nh, ((0, 8),))
    if n > 3:
        ref[1 * ln:2 * ln] = ip6ref.packet(rng, ln, nh, ((51, 24), (60, 8)))
        ref[2 * ln:3 * ln] = ip6ref.packet(rng, ln, nh, ((44, 8),))
        ref[3 * ln:4 * ln] = ip6ref.packet(rng, ln, nh, ((0, 2048),))
    exp, ever, _ = ip6ref.expect(port, ref, offs, [ln] * n, GEN6)
    for verdict in (True, False):
        out, ver, kern = run_strided(eng, ref, n, ln, 0, ln, GEN6, verdict)
        assert kern.startswith("dstr6_kernel<"), kern
        same(out, exp, f"chains out, verdict {verdict}")
        if verdict:
            same(ver, ever, "chains verdict")
    if n > 3:
        assert ever[3] == cgck.BAD_LEN and exp[2] == 0
    # L4 alone and IP alone take the family too
    for flags in (cgck.L4 | cgck.IP6, cgck.IP | cgck.IP6):
        e2, _, _ = ip6ref.expect(port, ref, offs, [ln] * n, flags)
        out, _, kern = run_strided(eng, ref, n, ln, 0, ln, flags)
        assert kern.startswith("dstr6_kernel<"), kern
        same(out, e2, f"flags {flags:#x}")


def test_dstr_auto_and_fallback(engine, port):
    """The dispatcher's own choice for dense 1500 B IPv6 frames is dstr6; a
    batch it cannot take (field zeroing) is the group kernel's."""
    n, ln = 70, 1500
    ref = synth_ref(port, n, ln, ln, 6, 3)
    offs = np.arange(n, dtype=np.int64) * ln
    for flags, want in ((GEN6, "dstr6_kernel<"), (ZERO6, "cksum6_kernel<")):
        exp, ever, _ = ip6ref.expect(port, ref, offs, [ln] * n, flags)
        out, ver, kern = run_strided(engine, ref, n, ln, 0, ln, flags)
        assert kern.startswith(want), kern
        same(out, exp, f"flags {flags:#x}")


# -- the 64 B lane family -----------------------------------------------------------

_lane_ref = {}


def lane_batch(port, ln, n):
    """stride 64: synth frames (UDP), every 7th with HBH(8), a few other chains."""
    if (ln, n) not in _lane_ref:
        ref = synth_ref(port, n, 64, ln, 17, 0x64)
        rng = np.random.default_rng(ln + n)
        for i in range(0, n, 7):
            ref[i * 64:i * 64 + ln] = ip6ref.packet(rng, ln, (6, 17, 58, 59)[(i // 7) % 4], ((0, 8),))
        for i, chain in ((1, ((51, 12),)), (2, ((44, 8),)), (3, ((0, 32),)), (4, ((0, 8), (60, 8)))):
            if i < n:
                ref[i * 64:i * 64 + ln] = ip6ref.packet(rng, ln, 17, chain)
        offs = np.arange(n, dtype=np.int64) * 64
        exp, ever, _ = ip6ref.expect(port, ref, offs, [ln] * n, GEN6)
        ref.setflags(write=False)
        _lane_ref[ln, n] = ref, exp, ever
    return _lane_ref[ln, n]


@pytest.mark.parametrize("family,kernel", [("lpd", "lpd6_kernel<"), ("lpa", "lpa6_kernel<"), ("auto", "lpd6_kernel<")])
@pytest.mark.parametrize("ln", [60, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_lane64(pinned, port, family, kernel, ln, n):
    ref, exp, ever = lane_batch(port, ln, n)
    eng = pinned(family)
    out, _, kern = run_strided(eng, ref, n, 64, 0, ln, GEN6, verdict=False)
    assert kern.startswith(kernel), kern
    same(out, exp, "out")
    # with verdicts lpd passes the batch on to lpa (lpd_ok)
    out, ver, kern = run_strided(eng, ref, n, 64, 0, ln, GEN6, verdict=True)
    assert kern.startswith("lpa6_kernel<"), kern
    same(out, exp, "out, with verdicts")
    same(ver, ever, "verdict")


def test_lane64_synth_and_fallback(engine, port):
    """cgck_synth_strided_ip6 at stride 64 (ip_len 60, the measured shape),
    and a batch the lane variants do not take (verify) in the group kernel."""
    n, ln = 1000, 60
    for nh in (6, 17, 58, 59):
        d, o = cgck.DeviceBuffer(n * 64), cgck.DeviceBuffer(4 * n)
        engine.synth_strided_ip6(d.ptr, n, 64, ln, nh, 9)
        engine.strided(d.ptr, n, 64, 0, ln, GEN6, o.ptr)
        kern = engine.last_kernel
        got, out = np.zeros(n * 64, np.uint8), np.zeros(n, np.uint32)
        d.download(got, stream=engine.stream)
        o.download(out, stream=engine.stream)
        engine.sync()
        d.free()
        o.free()
        ref = synth_ref(port, n, 64, ln, nh, 9)
        same(got, ref, "synth bytes")
        offs = np.arange(n, dtype=np.int64) * 64
        exp, _, _ = ip6ref.expect(port, ref, offs, [ln] * n, GEN6)
        assert kern.startswith("lpd6_kernel<"), kern
        same(out, exp, f"nh {nh}")
        exp, ever, _ = ip6ref.expect(port, ref, offs, [ln] * n, TOY6)
        out, ver, kern = run_strided(engine, ref, n, 64, 0, ln, TOY6)
        assert kern.startswith("cksum6_kernel<"), kern
        same(out, exp, f"verify out nh {nh}")
        same(ver, ever, f"verify verdict nh {nh}")


# -- host path ----------------------------------------------------------------------

@pytest.mark.parametrize("where,n", [("pageable", 300), ("pageable", 900), ("registered", 300)])
def test_desc_host(engine, port, where, n):
    """cgck_desc_host with CGCK_IP6 while a burst server is open: the batch
    takes the launch path (small pageable: pinned staging; large pageable:
    DMA; registered: read and filled in place) and is exact."""
    eng = engine
    L = cgck.load()
    rng = np.random.default_rng(n)
    buf, desc = cross_batch(rng, n, 14)
    if where == "pageable":    # 300 frames fit the pinned staging (512 KiB), 900 do not
        assert (int(desc["ip_len"].sum()) > 512 << 10) == (n == 900)
    offs = desc["frame_off"].astype(np.int64) + 14
    raw = None
    if where == "registered":
        raw, ring = page_ring(buf.nbytes)
        ring[:buf.nbytes] = buf
        buf = ring[:buf.nbytes]
        assert L.cgck_host_register(ring.ctypes.data, ring.nbytes) == 0
    eng.burst_open(max_pkts=2048, max_bytes=4 << 20)
    try:
        orig = buf.copy()
        for flags in (GEN6, TOY6, FILL6):
            exp, ever, eafter = ip6ref.expect(port, orig, offs, desc["ip_len"], flags)
            out, ver = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xEE, np.uint8)
            eng.desc_host(buf, desc, flags, out, ver)
            assert eng.last_kernel.startswith("cksum6_kernel<"), eng.last_kernel
            same(out, exp, f"{where} out flags {flags:#x}")
            same(ver, ever, f"{where} verdict flags {flags:#x}")
            same(buf, eafter, f"{where} bytes flags {flags:#x}")
    finally:
        eng.burst_close()
        if raw is not None:
            assert L.cgck_host_unregister(ring.ctypes.data) == 0


# -- errors ---------------------------------------------------------------------------

def test_errors(engine):
    L = cgck.load()
    d, o = cgck.DeviceBuffer(4096), cgck.DeviceBuffer(64)
    desc = np.zeros(2, cgck.DESC_DTYPE)
    desc["ip_len"] = 64
    try:
        rc = L.cgck_strided(engine.ctx, d.ptr, 2, 64, 0, 64, cgck.L4 | cgck.L4_NOPSEUDO | cgck.IP6, o.ptr, None, None, None)
        assert rc == -22 and "CGCK_IP6" in cgck.last_error()
        dd = cgck.DeviceBuffer(24)
        rc = L.cgck_desc(engine.ctx, d.ptr, dd.ptr, 2, cgck.L4 | cgck.L4_NOPSEUDO | cgck.IP6, o.ptr, None, None, None)
        assert rc == -22
        dd.free()
        host = np.zeros(4096, np.uint8)
        with pytest.raises(cgck.CgckError, match="CGCK_IP6"):
            engine.desc_host(host, desc, cgck.L4 | cgck.L4_NOPSEUDO | cgck.IP6)
        rc = L.cgck_strided(engine.ctx, d.ptr, 1, 70000, 0, 66000, GEN6, o.ptr, None, None, None)
        assert rc == -22 and "jumbogram" in cgck.last_error()
        out = np.zeros(2, np.uint32)
        engine.burst_open(max_pkts=64, max_bytes=1 << 20)
        try:
            for flags in (GEN6, cgck.RAW | cgck.IP6):
                assert engine.burst_request(d.ptr, 4096, desc, flags, out) == -22
                assert "IPv6" in cgck.last_error()
        finally:
            engine.burst_close()
    finally:
        d.free()
        o.free()
