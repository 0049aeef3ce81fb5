"""CGCK_MIXED (lpwx_kernel, cgck_lpwx.hip): batches that mix IPv4, IPv6 and
frames of neither family in one call.  Every packet of every batch is compared
with the referee (tests/mixedref.py over the oracle's port), never with the
library itself: `out`, `verdict`, the `bad` counters and the buffer bytes
(unchanged) by exact equality, and every test asserts that lpwx_kernel ran."""
import numpy as np
import pytest

import cgck
import mixedbatches as MB
import mixedref as MR
from conftest import load_golden

pytestmark = pytest.mark.gpu

MIXED = cgck.MIXED
GEN = cgck.GEN_BOTH | MIXED
ZERO = cgck.GEN_BOTH | cgck.ZERO_FIELDS | MIXED
TOY = cgck.VERIFY_TOY | MIXED
BSD = cgck.VERIFY_BSD | MIXED
FLAG_SETS = (GEN, cgck.L4 | MIXED, cgck.IP | MIXED, ZERO, TOY, BSD)
LPWX = "lpwx_kernel<"
EINVAL = -22


def run(eng, buf, desc, flags, verdict=True, bad=None, desc_shift=0):
    """cgck_desc over a host batch: (out, verdict, bytes after, bad after, kernel).
    desc_shift: the descriptor array's offset from a 16-byte boundary."""
    n = len(desc)
    d = cgck.DeviceBuffer(max(buf.nbytes, 16))
    dd = cgck.DeviceBuffer(desc.nbytes + 16)
    o = cgck.DeviceBuffer(4 * n)
    v = cgck.DeviceBuffer(n) if verdict else None
    b = cgck.DeviceBuffer(8) if bad is not None else None
    try:
        d.upload(buf, stream=eng.stream)
        dd.upload(desc, off=desc_shift, stream=eng.stream)
        if b:
            b.upload(np.asarray(bad, np.uint32), stream=eng.stream)
        eng.desc(d.ptr, dd.ptr + desc_shift, n, flags, o.ptr, v.ptr if v else None, b.ptr if b else None)
        kern = eng.last_kernel
        out, ver, after = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros_like(buf)
        cnt = np.zeros(2, np.uint32)
        o.download(out, stream=eng.stream)
        if v:
            v.download(ver, stream=eng.stream)
        if b:
            b.download(cnt, stream=eng.stream)
        d.download(after, stream=eng.stream)
        eng.sync()
    finally:
        for x in (d, dd, o, v, b):
            if x:
                x.free()
    return out, ver, after, cnt, kern


def same(got, exp, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]}, " \
                          f"want {np.asarray(exp)[bad[:5]]}"


def check(eng, port, batch, flags, what, verdict=True, bad=None, desc_shift=0, exp=None):
    buf, desc, offs, lens = batch
    eout, ever = exp if exp is not None else MR.expect(port, buf, offs, lens, flags)
    out, ver, after, cnt, kern = run(eng, buf, desc, flags, verdict, bad, desc_shift)
    assert kern.startswith(LPWX), (what, kern)
    assert kern.endswith("false>" if desc_shift % 16 else "true>"), (what, kern)
    same(out, eout, f"out, {what}, flags {flags:#x}")
    if verdict:
        same(ver, ever, f"verdict, {what}, flags {flags:#x}")
    same(after, buf, f"bytes, {what}, flags {flags:#x}")
    if bad is not None:
        b0, b1 = MR.counters(ever)
        assert (int(cnt[0]), int(cnt[1])) == (int(bad[0]) + b0, int(bad[1]) + b1), (what, cnt, b0, b1)
    return out, ver


# -- 1. packed batches ----------------------------------------------------------------

NS = (1, 63, 64, 65, 255, 256, 257, 3000)     # the step is 64 packets, the output chunk 256


def class_frames(rng, n):
    """n frames: every class in turn (shuffled), then typical lengths of both families."""
    fr = MB.all_classes(rng)
    while len(fr) < n:
        fr += MB.pattern(rng, "alt", 64)
    return [fr[i] for i in rng.permutation(len(fr))[:n]] if n < len(fr) else fr


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_packed(engine, port, n, half):
    """Every packet class of both families and of neither, back to back, first
    offsets 0..15 over the parameters; every flag set with and without a
    verdict array."""
    first_off = 2 * NS.index(n) + half
    rng = np.random.default_rng(2000 + 2 * n + half)
    batch = MB.packed(rng, class_frames(rng, n), first_off)
    for flags in FLAG_SETS:
        exp = MR.expect(port, batch[0], batch[2], batch[3], flags)
        check(engine, port, batch, flags, f"n {n} first_off {first_off}", exp=exp)
        check(engine, port, batch, flags, f"n {n} first_off {first_off}, no verdicts", verdict=False, exp=exp)


def test_classes(engine, port):
    """Every class once, with valid checksum fields, under the verify sets: the
    stored-zero rules per family (V_IP_ZERO_IS_FFFF and V_UDP_ZERO_SKIP for IPv4
    only), NOT_IP, and BAD_LEN per family."""
    rng = np.random.default_rng(31)
    frames = MB.all_classes(rng)
    have = set().union(*(MB.tags(f) for f in frames))
    assert MB.REQUIRED <= have, sorted(MB.REQUIRED - have)
    buf, desc, offs, lens = MB.packed(rng, frames, 6)
    valid = MB.fill_fields(port, buf, offs, lens)
    fam = MR.family(buf, offs, lens)
    for b in (buf, valid):
        for flags in (TOY, BSD, TOY | cgck.V_UDP_ZERO_SKIP, TOY | cgck.V_IP_ZERO_IS_FFFF):
            out, ver = check(engine, port, (b, desc, offs, lens), flags, "classes", bad=(3, 4))
            assert np.all(ver[fam == 0] == cgck.NOT_IP) and np.all(out[fam == 0] == 0)
            assert np.all(ver[fam == -1] == cgck.BAD_LEN)
            assert not np.any(ver[fam == 6] & cgck.BAD_IP) and not np.any(out[fam == 6] & 0xFFFF)
    out, ver = check(engine, port, (valid, desc, offs, lens), TOY, "valid")
    assert not np.any(ver & (cgck.BAD_IP | cgck.BAD_L4))
    # UDP with a stored 0 under the skip flag: skipped for IPv4, compared and bad for IPv6
    z = valid.copy()
    udp4 = [i for i, f in enumerate(frames) if "v4_p17" in MB.tags(f) and MB.l4_field_at(f) is not None]
    udp6 = [i for i, f in enumerate(frames) if "v6_nh17" in MB.tags(f)]
    assert udp4 and udp6
    for i in udp4 + udp6:
        at = int(offs[i]) + MB.l4_field_at(valid[int(offs[i]):int(offs[i]) + int(lens[i])])
        z[at:at + 2] = 0
    out, ver = check(engine, port, (z, desc, offs, lens), BSD, "udp zero")
    assert not np.any(ver[udp4] & cgck.BAD_L4) and np.all(ver[udp6] == cgck.BAD_L4)


# -- 2. family patterns inside a step -------------------------------------------------

@pytest.mark.parametrize("kind", ["alt", "runs", "one6", "one4"])
def test_patterns(engine, port, kind):
    rng = np.random.default_rng(40 + len(kind))
    frames = MB.pattern(rng, kind, 200)
    for first_off in (0, 9):
        batch = MB.packed(rng, frames, first_off)
        for flags in (GEN, ZERO, TOY):
            check(engine, port, batch, flags, f"{kind} at {first_off}")
    check(engine, port, MB.slotted(rng, frames, 2048, 14), GEN, f"{kind} in slots")


# -- 3. layouts and entry points ------------------------------------------------------

def test_layouts(engine, port):
    """2048 B slots at +14, reordered and gapped descriptors (gathered steps), a
    descriptor array at +4 bytes (read from global memory each step), and steps
    computed from global memory.  64 frames of 1500 B back to back are 6000
    chunks, inside the 16 windows of a step, so that step streams; 64 frames of
    2064 B are past them and take the global-memory path, alone and before a
    streamed step."""
    rng = np.random.default_rng(51)
    frames = class_frames(rng, 330)
    ring = MB.slotted(rng, frames, 2048, 14)
    buf, desc, offs, lens = MB.packed(rng, frames, 9)
    rev = (buf, desc[::-1].copy(), offs[::-1].copy(), lens[::-1].copy())
    gap = MB.lay(rng, frames, np.cumsum([len(f) + (i * 7) % 50 for i, f in enumerate(frames)]))
    for what, batch in (("ring", ring), ("reversed", rev), ("gapped", gap), ("packed", (buf, desc, offs, lens))):
        for flags in (GEN, ZERO, TOY):
            exp = MR.expect(port, batch[0], batch[2], batch[3], flags)
            check(engine, port, batch, flags, what, exp=exp)
            check(engine, port, batch, flags, what + ", descriptors at +4", desc_shift=4, exp=exp, bad=(1, 2))
        check(engine, port, batch, GEN, what + ", no verdicts", verdict=False)
    for ln in (1500, 2064):
        for extra in (0, 70):
            big = [MB.v4(rng, ln, MB.V4_PROTOS[i % 4], 5 + i % 3) if i % 3 else
                   MB.ip6ref.packet(rng, ln, (6, 17, 58)[i % 3], MB.B6.chain_of(i)) for i in range(64)]
            big[5] = MB.other(rng, ln, 0)
            big += MB.pattern(rng, "alt", extra)
            batch = MB.packed(rng, big, 0)
            for flags in (GEN, TOY):
                check(engine, port, batch, flags, f"64 x {ln} + {extra}", bad=(0, 0))
            check(engine, port, batch, GEN, f"64 x {ln} + {extra}, descriptors at +4", desc_shift=4)


@pytest.mark.parametrize("ln,stride,l3", [(256, 256, 0), (576, 600, 14), (1000, 1031, 7)])
def test_strided(engine, port, ln, stride, l3):
    """cgck_strided with the version nibble varied per frame."""
    n = 257
    rng = np.random.default_rng(60 + ln)
    frames = []
    for i in range(n):
        k = (i * 7 + i // 5) % 10
        frames.append(MB.other(rng, ln, (0, 5, 15)[i % 3]) if k == 9 else
                      MB.ip6ref.packet(rng, ln, MB.B6.NHS[i % 5], MB.B6.chain_of(i)) if k % 2 else
                      MB.v4(rng, ln, MB.V4_PROTOS[i % 4], 5 + (i % 4 == 3) * (i % 11)))
    buf, _, offs, lens = MB.lay(rng, frames, np.arange(n, dtype=np.int64) * stride + l3, tail=stride)
    d, o, v, b = cgck.DeviceBuffer(buf.nbytes), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n), cgck.DeviceBuffer(8)
    try:
        d.upload(buf, stream=engine.stream)
        for flags in (GEN, TOY, ZERO):
            exp, ever = MR.expect(port, buf, offs, lens, flags)
            b.upload(np.array([7, 8], np.uint32), stream=engine.stream)
            engine.strided(d.ptr, n, stride, l3, ln, flags, o.ptr, v.ptr, b.ptr)
            kern = engine.last_kernel
            out, ver, cnt, after = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(2, np.uint32), np.zeros_like(buf)
            o.download(out, stream=engine.stream)
            v.download(ver, stream=engine.stream)
            b.download(cnt, stream=engine.stream)
            d.download(after, stream=engine.stream)
            engine.sync()
            assert kern.startswith("lpwx_kernel<false"), kern
            same(out, exp, f"strided out flags {flags:#x}")
            same(ver, ever, f"strided verdict flags {flags:#x}")
            same(after, buf, "strided bytes")
            b0, b1 = MR.counters(ever)
            assert (int(cnt[0]), int(cnt[1])) == (7 + b0, 8 + b1)
    finally:
        for x in (d, o, v, b):
            x.free()


# -- 4. counters ----------------------------------------------------------------------

def test_counters(engine, port):
    """Valid fields everywhere, then every 7th L4 field and every 11th IPv4
    header sum corrupted; the counters are running totals (preloaded non-zero)."""
    rng = np.random.default_rng(70)
    frames = MB.pattern(rng, "alt", 700) + MB.other_classes(rng)
    frames = [frames[i] for i in rng.permutation(len(frames))]
    buf, desc, offs, lens = MB.packed(rng, frames, 3)
    bufv = MB.fill_fields(port, buf, offs, lens)
    out, ver = check(engine, port, (bufv, desc, offs, lens), TOY, "valid", bad=(1000, 0xFFFFFFF0))
    assert not np.any(ver & (cgck.BAD_IP | cgck.BAD_L4))
    hit_l4 = hit_ip = 0
    for i in range(len(frames)):
        o, p = int(offs[i]), bufv[int(offs[i]):int(offs[i]) + int(lens[i])]
        at = MB.l4_field_at(p)
        if i % 7 == 0 and at is not None:
            bufv[o + at] ^= 0x10
            hit_l4 += 1
        if i % 11 == 0 and len(p) and int(p[0]) >> 4 == 4:
            bufv[o + 10] ^= 0x01
            hit_ip += 1
    assert hit_l4 > 50 and hit_ip > 20
    for flags in (TOY, BSD):
        out, ver = check(engine, port, (bufv, desc, offs, lens), flags, "corrupted", bad=(17, 23))
        assert MR.counters(ver) == (hit_ip, hit_l4)
        check(engine, port, (bufv, desc, offs, lens), flags, "corrupted, no verdicts", verdict=False, bad=(17, 23))


# -- 5. argument checks ---------------------------------------------------------------

def test_arguments(engine):
    L = cgck.load()
    n = 4
    buf = np.zeros(4096, np.uint8)
    buf[::64] = 0x45
    desc = np.zeros(n, cgck.DESC_DTYPE)
    desc["frame_off"] = np.arange(n) * 64
    desc["ip_len"] = 64
    d, dd, o = cgck.DeviceBuffer(4096), cgck.DeviceBuffer(64), cgck.DeviceBuffer(64)
    out = np.zeros(n, np.uint32)
    try:
        d.upload(buf, stream=engine.stream)
        dd.upload(desc, stream=engine.stream)
        engine.sync()
        for extra in (cgck.RAW, cgck.IP6, cgck.L4_NOPSEUDO, cgck.STORE):
            for base in (cgck.GEN_BOTH, cgck.L4, cgck.VERIFY_TOY):
                fl = base | MIXED | extra
                assert L.cgck_strided(engine.ctx, d.ptr, n, 64, 0, 64, fl, o.ptr, None, None, None) == EINVAL
                assert L.cgck_desc(engine.ctx, d.ptr, dd.ptr, n, fl, o.ptr, None, None, None) == EINVAL
                assert L.cgck_desc_host(engine.ctx, buf.ctypes.data, buf.nbytes, desc.ctypes.data, n, fl,
                                        out.ctypes.data, None) == EINVAL
        assert L.cgck_strided(engine.ctx, d.ptr, 1, 1 << 17, 0, 65536, GEN, o.ptr, None, None, None) == EINVAL
        assert L.cgck_strided(engine.ctx, d.ptr, n, 64, 0, 64, GEN, o.ptr, None, None, None) == 0
        engine.sync()
        assert engine.last_kernel.startswith(LPWX)
        # pins are ignored: one kernel
        for fam in ("group", "lpp", "slot2", "lpw", "auto"):
            engine.set_kernel(fam)
            assert L.cgck_desc(engine.ctx, d.ptr, dd.ptr, n, GEN, o.ptr, None, None, None) == 0
            engine.sync()
            assert engine.last_kernel.startswith(LPWX), (fam, engine.last_kernel)
        engine.burst_open(max_pkts=256, max_bytes=1 << 20)
        try:
            assert engine.burst_request(d.ptr, 4096, desc, GEN, out) == EINVAL
        finally:
            engine.burst_close()
    finally:
        engine.set_kernel("auto")
        for x in (d, dd, o):
            x.free()


# -- 6. the host path and the fixtures ------------------------------------------------

def test_desc_host(engine, port):
    """cgck_desc_host launches such a batch, with and without a burst server
    open, and leaves the bytes as they are."""
    rng = np.random.default_rng(80)
    buf, desc, offs, lens = MB.packed(rng, class_frames(rng, 300), 0)
    for flags in (GEN, TOY):
        exp, ever = MR.expect(port, buf, offs, lens, flags)
        for server in (False, True):
            if server:
                engine.burst_open(max_pkts=2048, max_bytes=4 << 20)
            try:
                out, ver, got = np.full(300, 0xDEADBEEF, np.uint32), np.full(300, 0xEE, np.uint8), buf.copy()
                engine.desc_host(got, desc, flags, out, ver)
                assert engine.last_kernel.startswith(LPWX), engine.last_kernel
                same(out, exp, f"desc_host out, server {server}")
                same(ver, ever, f"desc_host verdict, server {server}")
                same(got, buf, "desc_host bytes")
            finally:
                if server:
                    engine.burst_close()


def test_golden(engine, port):
    g = load_golden("mixed.json")
    frames = [np.frombuffer(bytes.fromhex(h), np.uint8) for h in g["packets"]]
    rng = np.random.default_rng(90)
    for first_off in (0, 11):
        batch = MB.packed(rng, frames, first_off)
        for name, s in g["sets"].items():
            exp = np.array(s["out"], np.uint32), np.array(s["verdict"], np.uint8)
            check(engine, port, batch, s["flags"], f"golden {name}", exp=exp, bad=(0, 0))


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("n", [1, 12, 60, 4097])
def test_generator(engine, port, n, ring):
    stride, l3 = (2048, 14) if ring else (0, 0)
    seed = 0xD0A1 + n
    ref, rdesc, offs, lens = MB.imix_dual(port, n, seed, stride, l3)
    nbytes = n * stride if ring else int(cgck.load().cgck_imix_bytes(n))
    assert nbytes >= ref.nbytes
    d, dd, o, v = cgck.DeviceBuffer(nbytes), cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n)
    try:
        engine.synth_imix_dual(d.ptr, dd.ptr, n, seed, stride, l3)
        engine.desc(d.ptr, dd.ptr, n, GEN, o.ptr, v.ptr)
        kern = engine.last_kernel
        got, gdesc = np.zeros(nbytes, np.uint8), np.zeros(n, cgck.DESC_DTYPE)
        out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        d.download(got, stream=engine.stream)
        dd.download(gdesc, stream=engine.stream)
        o.download(out, stream=engine.stream)
        v.download(ver, stream=engine.stream)
        engine.sync()
    finally:
        for x in (d, dd, o, v):
            x.free()
    same(got[:ref.nbytes], ref, "synth bytes")
    assert gdesc.tobytes() == rdesc.tobytes(), "descriptors"
    assert kern.startswith(LPWX), kern
    exp, ever = MR.expect(port, ref, offs, lens, GEN)
    same(out, exp, "out")
    assert not ver.any() and not ever.any()
