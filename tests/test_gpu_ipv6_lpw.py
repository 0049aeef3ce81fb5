"""lpw6_kernel (cgck_lpw6.hip): mixed-length CGCK_IP6 descriptor and strided
batches streamed through LDS.  Every packet of every batch is compared with
the referee (tests/ip6ref.py over oracle.port().in_cksum), never with the
library itself, and every test asserts the kernel that ran: lpw6_kernel< where
the streaming kernel is meant, cksum6_kernel< where the batch must fall back.
CGCK_RAW | CGCK_IP6 is CGCK_RAW by the API's contract (include/cgck.h,
test_gpu_ipv6.py::test_raw_is_unchanged): that one flag set reaches the
dispatcher without CGCK_IP6 and streams through lpw_kernel."""
import numpy as np
import pytest

import cgck
import ip6batches as B
import ip6ref

pytestmark = pytest.mark.gpu

GEN6 = cgck.GEN_BOTH | cgck.IP6
ZERO6 = cgck.GEN_BOTH | cgck.ZERO_FIELDS | cgck.IP6
FILL6 = cgck.FILL_BOTH | cgck.IP6
TOY6 = cgck.VERIFY_TOY | cgck.IP6
RAW6 = cgck.RAW | cgck.IP6
FLAG_SETS = (GEN6, cgck.L4 | cgck.IP6, cgck.IP | cgck.IP6, ZERO6, TOY6, TOY6 | cgck.V_UDP_ZERO_SKIP, RAW6)
LPW6 = "lpw6_kernel<"


@pytest.fixture(scope="module")
def lpw():
    """An engine pinned to the lpw family under the packed layout hint."""
    e = cgck.Engine(0, kernel="lpw")
    e.set_desc_layout(cgck.LAYOUT_PACKED)
    yield e
    e.close()


def run(eng, buf, desc, flags, verdict=True, want_bad=False):
    """cgck_desc over a host batch: (out, verdict, bytes after, kernel)."""
    n = len(desc)
    d = cgck.DeviceBuffer(max(buf.nbytes, 16))
    dd = cgck.DeviceBuffer(max(desc.nbytes, 12))
    o = cgck.DeviceBuffer(4 * n)
    v = cgck.DeviceBuffer(n) if verdict else None
    b = cgck.DeviceBuffer(8) if want_bad else None
    try:
        d.upload(buf, stream=eng.stream)
        dd.upload(desc, stream=eng.stream)
        if b:
            b.upload(np.zeros(2, np.uint32), stream=eng.stream)
        eng.desc(d.ptr, dd.ptr, n, flags, o.ptr, v.ptr if v else None, b.ptr if b else None)
        kern = eng.last_kernel
        out, ver, after = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros_like(buf)
        o.download(out, stream=eng.stream)
        if v:
            v.download(ver, stream=eng.stream)
        d.download(after, stream=eng.stream)
        eng.sync()
    finally:
        for x in (d, dd, o, v, b):
            if x:
                x.free()
    return out, ver, after, kern


def want(port, buf, offs, lens, flags):
    """(out, verdict, bytes after) by the referee."""
    if flags & cgck.RAW:
        out = np.array([port.in_cksum(buf, int(o), int(ln)) for o, ln in zip(offs, lens)], np.uint32)
        return out, np.zeros(len(offs), np.uint8), buf
    return ip6ref.expect(port, buf, offs, lens, flags)


def same(got, exp, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]}, " \
                          f"want {np.asarray(exp)[bad[:5]]}"


def check(eng, port, batch, flags, what, verdict=True, kernel=LPW6, want_bad=False):
    buf, desc, offs, lens = batch
    exp, ever, eafter = want(port, buf, offs, lens, flags)
    out, ver, after, kern = run(eng, buf, desc, flags, verdict, want_bad)
    assert kern.startswith("lpw_kernel<" if flags & cgck.RAW and kernel == LPW6 else kernel), (what, kern)
    same(out, exp, f"out, {what}, flags {flags:#x}")
    if verdict:
        same(ver, ever, f"verdict, {what}, flags {flags:#x}")
    same(after, eafter, f"bytes, {what}, flags {flags:#x}")
    return out, ver


# -- 1. packed mixes ------------------------------------------------------------------

NS = (1, 63, 64, 65, 255, 256, 257, 3000)     # the step is 64 packets, the output chunk 256


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_packed_mixes(lpw, port, n, half):
    """Every length class and an IMIX 7:4:1 mix back to back, every nh, first
    offsets 0..15 over the parameters (odd and non-dword a0 follow from the odd
    lengths too); every flag set with a verdict array, GEN6 also without one
    (the deferred 16-byte output store)."""
    first_off = 2 * NS.index(n) + half
    rng = np.random.default_rng(1000 + 2 * n + half)
    lens = rng.choice(np.array(B.LENS + B.IMIX), n)
    batch = B.packed(rng, B.frames_of(rng, lens, B.NHS), first_off)
    for flags in FLAG_SETS:
        check(lpw, port, batch, flags, f"n {n} first_off {first_off}")
    check(lpw, port, batch, GEN6, f"n {n} first_off {first_off}, no verdicts", verdict=False)


# -- 2. extension headers inside streamed steps ---------------------------------------

@pytest.mark.parametrize("first_off", [0, 15])
def test_packed_chains(lpw, port, first_off):
    """test_gpu_ipv6.py::test_chains' cases inside packed steps: every 5th frame
    with HBH(8), every 11th with HBH(16) + DestOpt(8), and once each AH, Routing,
    Fragment, a ninth header, a chain cut by ip_len, a field that does not fit,
    ip_len 39 and 0."""
    rng = np.random.default_rng(77 + first_off)
    n = 330
    lens = [B.LENS[i % len(B.LENS)] for i in range(n)]
    at = [3 + 27 * j for j in range(len(B.SPECIALS))]           # spread over the steps, lane 63/0 among them
    at[4], at[5] = 63, 64
    frames = B.frames_of(rng, lens, B.NHS, chains=True, specials=at)
    st = [ip6ref.walk(f, len(f))[2] for f in frames]
    assert st.count(ip6ref.NO_L4) >= 2 and st.count(ip6ref.BADLEN) >= 6
    batch = B.packed(rng, frames, first_off)
    for flags in (GEN6, ZERO6, TOY6):
        out, ver = check(lpw, port, batch, flags, f"first_off {first_off}")
        for i, s in enumerate(st):
            if s != ip6ref.OK:
                assert out[i] == 0 and ver[i] == (cgck.BAD_LEN if s == ip6ref.BADLEN else 0), i


# -- 3. window edges ------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 6, 7, 8, 9, 16, 42, 43, 46, 47, 56, 57, 58, 64, 80])
def test_window_edge(lpw, port, d):
    """One packed 64-frame step from a 16-byte boundary whose second frame
    starts d bytes before the end of the step's first 8 KiB window: byte 6, the
    first 8 bytes and each protocol's field on either side of the edge."""
    rng = np.random.default_rng(300 + d)
    for nh1 in (6, 17, 58):
        lens = [8192 - d] + [int(x) for x in rng.choice(np.array((64, 65, 131, 576)), 63)]
        nhs = [nh1 if i == 1 else (6, 17, 58)[i % 3] for i in range(64)]
        frames = [ip6ref.packet(rng, ln, nh) for ln, nh in zip(lens, nhs)]
        batch = B.packed(rng, frames, 0)
        assert batch[2][1] == 8192 - d
        for flags in (GEN6, TOY6):
            check(lpw, port, batch, flags, f"d {d} nh {nh1}")


# -- 4. verify ------------------------------------------------------------------------

def test_verify(lpw, port):
    n = 257
    rng = np.random.default_rng(4)
    lens = rng.choice(np.array((64, 80, 575, 576, 1279, 1500, 1514)), n)
    frames = [ip6ref.packet(rng, int(ln), (6, 17, 58)[i % 3], ((0, 8),) if i % 4 == 3 and ln > 64 else ())
              for i, ln in enumerate(lens)]
    buf, desc, offs, lens = B.packed(rng, frames, 5)
    exp, ever, filled = ip6ref.expect(port, buf, offs, lens, FILL6)        # the referee fills the fields
    assert not ever.any() and np.all(exp >> 16) and not np.array_equal(filled, buf)
    out, ver = check(lpw, port, (filled, desc, offs, lens), TOY6, "filled")
    assert not ver.any()
    same(out, exp, "verify out")
    hit = sorted({0, n // 2, n - 1})
    broken = filled.copy()
    for i in hit:
        broken[offs[i] + lens[i] - 1] ^= 0x40
    out, ver = check(lpw, port, (broken, desc, offs, lens), TOY6, "broken")
    assert sorted(np.nonzero(ver)[0].tolist()) == hit and np.all(ver[hit] == cgck.BAD_L4)
    # UDP with a stored 0: bad unless V_UDP_ZERO_SKIP
    udp = [i for i in range(n) if i % 3 == 1][:5]
    zeroed = filled.copy()
    for i in udp:
        l4 = ip6ref.walk(filled[offs[i]:offs[i] + lens[i]], int(lens[i]))[0]
        zeroed[offs[i] + l4 + 6:offs[i] + l4 + 8] = 0
    out, ver = check(lpw, port, (zeroed, desc, offs, lens), TOY6, "udp zero")
    assert sorted(np.nonzero(ver)[0].tolist()) == udp
    out, ver = check(lpw, port, (zeroed, desc, offs, lens), TOY6 | cgck.V_UDP_ZERO_SKIP, "udp zero, skip")
    assert not ver.any()


# -- 5. gathered and fallback steps ---------------------------------------------------

def test_gathered_and_fallback(lpw, port):
    rng = np.random.default_rng(55)
    n = 330
    lens = [B.LENS[i % len(B.LENS)] for i in range(n)]
    frames = B.frames_of(rng, lens, B.NHS, chains=True, specials=[3 + 27 * j for j in range(len(B.SPECIALS))])
    ring = B.slotted(rng, frames, 2048, 14)
    buf, desc, offs, lens_ = B.packed(rng, frames, 9)
    rev = (buf, desc[::-1].copy(), offs[::-1].copy(), lens_[::-1].copy())
    gap = B.lay(rng, frames, np.cumsum([len(f) + (i * 7) % 50 for i, f in enumerate(frames)]))
    for what, batch in (("ring", ring), ("reversed", rev), ("gapped", gap)):
        for flags in (GEN6, ZERO6, TOY6):
            check(lpw, port, batch, flags, what)
        check(lpw, port, batch, GEN6, what + ", no verdicts", verdict=False)
    # 64 frames of 2048 B back to back are exactly 16 windows; of 2064 B, past the
    # limit: computed from global memory.  Then the same followed by a streamed step.
    for ln in (2048, 2064):
        for extra in (0, 64):
            big = [ip6ref.packet(rng, ln, B.NHS[i % 5], B.chain_of(i)) for i in range(64)]
            big += [ip6ref.packet(rng, 576, 6) for _ in range(extra)]
            batch = B.packed(rng, big, 0)
            for flags in (GEN6, TOY6):
                check(lpw, port, batch, flags, f"64 x {ln} + {extra}")


# -- 6. strided -----------------------------------------------------------------------

def test_strided_auto(engine, port):
    n, stride, ln, l3 = 257, 600, 576, 14
    rng = np.random.default_rng(6)
    frames = [ip6ref.packet(rng, ln, B.NHS[i % 5], B.chain_of(i)) for i in range(n)]
    buf, _, offs, lens = B.lay(rng, frames, np.arange(n, dtype=np.int64) * stride + l3, tail=stride)
    d, o, v = cgck.DeviceBuffer(buf.nbytes), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n)
    try:
        d.upload(buf, stream=engine.stream)
        for flags in (GEN6, TOY6, ZERO6):
            exp, ever, _ = ip6ref.expect(port, buf, offs, lens, flags)
            engine.strided(d.ptr, n, stride, l3, ln, flags, o.ptr, v.ptr)
            kern = engine.last_kernel
            out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            o.download(out, stream=engine.stream)
            v.download(ver, stream=engine.stream)
            engine.sync()
            assert kern.startswith("lpw6_kernel<false"), kern
            same(out, exp, f"strided out flags {flags:#x}")
            same(ver, ever, f"strided verdict flags {flags:#x}")
    finally:
        for x in (d, o, v):
            x.free()


# -- 7. dispatch ----------------------------------------------------------------------

def test_dispatch(engine, port):
    rng = np.random.default_rng(7)
    n = 600
    frames = [ip6ref.packet(rng, B.IMIX[i % 12], (6, 17, 58)[i % 3], B.chain_of(i) if B.IMIX[i % 12] > 64 else ())
              for i in rng.permutation(n)]
    batch = B.packed(rng, frames, 0)
    try:
        engine.set_kernel("auto")
        engine.set_desc_layout(cgck.LAYOUT_ANY)
        engine.set_desc_len_hint(354)
        check(engine, port, batch, GEN6, "hint 354")
        check(engine, port, batch, TOY6, "hint 354")
        check(engine, port, batch, GEN6, "hint 354, bad counters", kernel="cksum6_kernel<", want_bad=True)
        check(engine, port, batch, FILL6, "hint 354, fill", kernel="cksum6_kernel<")
        for hint in (200, 1500):
            engine.set_desc_len_hint(hint)
            check(engine, port, batch, GEN6, f"hint {hint}", kernel="cksum6_kernel<")
        # the host path while a burst server is open: the launch path, now lpw6
        engine.set_desc_len_hint(354)
        hb = B.packed(rng, frames[:300], 0)
        buf, desc, offs, lens = hb
        exp, ever, _ = ip6ref.expect(port, buf, offs, lens, GEN6)
        engine.burst_open(max_pkts=2048, max_bytes=4 << 20)
        try:
            out, ver, got = np.full(300, 0xDEADBEEF, np.uint32), np.full(300, 0xEE, np.uint8), buf.copy()
            engine.desc_host(got, desc, GEN6, out, ver)
            assert engine.last_kernel.startswith(LPW6), engine.last_kernel
            same(out, exp, "desc_host out")
            same(ver, ever, "desc_host verdict")
            same(got, buf, "desc_host bytes")
        finally:
            engine.burst_close()
    finally:
        engine.set_desc_len_hint(1500)
        engine.set_desc_layout(cgck.LAYOUT_ANY)
        engine.set_kernel("auto")


# -- 8. generator ---------------------------------------------------------------------

@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("n", [1, 12, 13, 1000])
def test_generator(lpw, port, n, ring):
    stride, l3 = (2048, 14) if ring else (0, 0)
    for nh in (6, 17, 58, 59):
        seed = 0x1A6 + n + nh
        ref, rdesc, offs, lens = B.imix6(port, n, nh, seed, stride, l3)
        nbytes = n * stride if ring else int(cgck.load().cgck_imix_bytes(n))
        assert nbytes >= ref.nbytes
        d, dd, o, v = cgck.DeviceBuffer(nbytes), cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n)
        try:
            if ring:
                lpw.synth_imix_ring_ip6(d.ptr, dd.ptr, n, stride, l3, nh, seed)
            else:
                lpw.synth_imix_ip6(d.ptr, dd.ptr, n, nh, seed)
            lpw.desc(d.ptr, dd.ptr, n, GEN6, o.ptr, v.ptr)
            kern = lpw.last_kernel
            got, gdesc = np.zeros(nbytes, np.uint8), np.zeros(n, cgck.DESC_DTYPE)
            out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            d.download(got, stream=lpw.stream)
            dd.download(gdesc, stream=lpw.stream)
            o.download(out, stream=lpw.stream)
            v.download(ver, stream=lpw.stream)
            lpw.sync()
        finally:
            for x in (d, dd, o, v):
                x.free()
        same(got[:ref.nbytes], ref, f"synth bytes nh {nh}")
        assert gdesc.tobytes() == rdesc.tobytes(), f"descriptors nh {nh}"
        assert kern.startswith(LPW6), kern
        exp, ever, _ = ip6ref.expect(port, ref, offs, lens, GEN6)
        same(out, exp, f"out nh {nh}")
        assert not ver.any() and not ever.any()
