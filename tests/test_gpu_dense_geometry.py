"""dstr_kernel's per-step geometry (cgck_dense_kernel.inc) is computed once per
wave: a lane's chunk offsets in the slot, the dwords of its first and last
chunk outside the frame, the chunks inside the frame, how many of a full
step's six DMAs are whole KiBs.  All of it depends only on base & 15, stride,
ip_len and the lane, so the cases here walk those: every alignment class of
base + l3_off and stride (mod 16), the length classes (byte-mask tails, the
1280 threshold, the shortest and longest frames, strides below ip_len, groups
whose last chunk sits in different rows), the batch edges (a partial step, a
partial chunk, one chunk per wave, waves that cross chunk boundaries with one
of them finishing on the general path) and the IPv6 variant.

Expected values are the oracle's (oracle/cksum_oracle.c through the `port`
fixture; IPv6: in_cksum over pseudo-header || segment as tests/ip6ref.py),
never the library's.  The engine is pinned to the dstr family."""
import numpy as np
import pytest

import cgck
import ip6ref
from test_gpu_dense import strided_frames

pytestmark = pytest.mark.gpu

FLAGS = (cgck.GEN_BOTH, cgck.RAW, cgck.L4 | cgck.L4_NOPSEUDO)
GEN6 = cgck.GEN_BOTH | cgck.IP6


@pytest.fixture(scope="module")
def dstr_engine():
    e = cgck.Engine(0, kernel="dstr")
    yield e
    e.close()


def run(engine, buf, n, stride, l3, ln, flags, shift=0):
    """The batch on the device, its first byte `shift` bytes into the
    allocation; outputs and verdicts."""
    d = cgck.DeviceBuffer(buf.nbytes + shift)
    o = cgck.DeviceBuffer(4 * n)
    v = cgck.DeviceBuffer(n)
    d.upload(buf, off=shift, stream=engine.stream)
    engine.strided(d.ptr + shift, n, stride, l3, ln, flags, o.ptr, v.ptr)
    kern = engine.last_kernel
    out, ver = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    o.download(out, stream=engine.stream)
    v.download(ver, stream=engine.stream)
    engine.sync()
    for b in (d, o, v):
        b.free()
    return out, ver, kern


def check(engine, port, buf, n, stride, l3, ln, flags, shift=0, what=""):
    exp, ever = port.batch_strided(buf.copy(), n, stride, l3, ln, flags)
    out, ver, kern = run(engine, buf, n, stride, l3, ln, flags, shift)
    assert kern.startswith("dstr_kernel<"), kern
    bad = np.nonzero((out != exp) | (ver != ever))[0]
    assert len(bad) == 0, f"{what} flags {flags:#x}: {len(bad)} mismatches, first {bad[:5]}, " \
                          f"got {out[bad[:5]]} want {exp[bad[:5]]}"
    return ever


# -- alignment classes ------------------------------------------------------------------

# 1031 frames: 16 full chunks of 64 and a last one of 7 (a partial step)
N_ALIGN = 1031


@pytest.mark.parametrize("l3", [0, 4, 8, 12])
@pytest.mark.parametrize("stride,ln", [(1504, 1500), (1508, 1500), (1512, 1500), (1500, 1500),
                                       (64, 60), (68, 60), (72, 60), (76, 60)])
def test_alignment_classes(dstr_engine, port, l3, stride, ln):
    """(base + l3_off) mod 16 x stride mod 16, at the product length and at a
    short one (where a step's span is a fraction of its first KiB)."""
    rng = np.random.default_rng(1000 * l3 + stride)
    buf = strided_frames(rng, N_ALIGN, stride, l3, ln)
    for flags in FLAGS:
        check(dstr_engine, port, buf, N_ALIGN, stride, l3, ln, flags, what=f"l3 {l3} stride {stride}")


@pytest.mark.parametrize("shift", [4, 12])
@pytest.mark.parametrize("stride,ln", [(1500, 1500), (68, 60)])
def test_device_pointer_offset(dstr_engine, port, shift, stride, ln):
    """The device pointer itself 4 and 12 bytes past a 16-byte boundary."""
    rng = np.random.default_rng(shift + stride)
    buf = strided_frames(rng, N_ALIGN, stride, 0, ln)
    for flags in FLAGS:
        check(dstr_engine, port, buf, N_ALIGN, stride, 0, ln, flags, shift=shift, what=f"shift {shift}")


# -- length classes -----------------------------------------------------------------------

# (stride, l3_off, ip_len): len & 3 != 0 (the byte-mask tail) around 1500 and at
# 21, 1279 | 1280 (five chunk rows always inside the frame from 1280 on), the
# longest and the shortest frame, strides below ip_len (frames overlap), and
# 1276 / 1500 / 0: q = 0, 12, 8, 4 in the four groups, so their frames have 80,
# 81, 81, 80 chunks and the last chunk sits in row 4 for two groups, row 5 for
# the others
LENGTHS = [(1500, 0, 1499), (1504, 4, 1501), (1280, 0, 1280), (1280, 8, 1279), (1520, 0, 1520), (1520, 12, 1520),
           (20, 0, 20), (24, 4, 21), (1000, 0, 1200), (1200, 8, 1500), (1500, 0, 1276)]


@pytest.mark.parametrize("stride,l3,ln", LENGTHS)
def test_length_classes(dstr_engine, port, stride, l3, ln):
    """ip_hl 5 mostly, 6..15 in some; frames shorter than their header are
    BAD_LEN (verdicts on in every case)."""
    rng = np.random.default_rng(stride * 7 + ln)
    buf = strided_frames(rng, N_ALIGN, stride, l3, ln, bad_len=ln < 60)
    for flags in FLAGS:
        ever = check(dstr_engine, port, buf, N_ALIGN, stride, l3, ln, flags, what=f"stride {stride} len {ln}")
        if ln < 60 and not flags & cgck.RAW:
            assert np.count_nonzero(ever & cgck.BAD_LEN) > 0


# -- batch edges ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 4099])
def test_batch_edges(dstr_engine, port, n):
    """ip_len = stride = 1500: a partial step, one full step, a partial chunk,
    one full chunk, one frame more, and a wave with one chunk each (4099)."""
    rng = np.random.default_rng(n)
    buf = strided_frames(rng, n, 1500, 0, 1500)
    for flags in FLAGS:
        check(dstr_engine, port, buf, n, 1500, 0, 1500, flags, what=f"n {n}")


def test_waves_cross_chunks(dstr_engine, port):
    """140003 frames are more than 64 x 8 x 256: every wave of the grid walks
    two chunks or more, its ring running across the chunk boundaries, and
    exactly one wave finishes the batch's last, partial chunk."""
    n = 140003
    rng = np.random.default_rng(n)
    buf = strided_frames(rng, n, 1500, 0, 1500)
    for flags in FLAGS:
        check(dstr_engine, port, buf, n, 1500, 0, 1500, flags, what="n 140003")


# -- IPv6 ---------------------------------------------------------------------------------------

def expect6(port, buf, n, stride, ln, nh, chained):
    """GEN_BOTH | IP6 outputs of n frames without extension headers: in_cksum
    over pseudo-header || segment, for all frames at once as one RAW batch of
    the oracle over records (src, dst, length, 0 0 0 nh, segment), which have
    ip_len bytes again.  The frames listed in `chained` (extension headers)
    come from ip6ref.expect, frame by frame."""
    v = buf[:n * stride].reshape(n, stride)
    rec = np.empty((n, ln), np.uint8)
    rec[:, 0:32] = v[:, 8:40]
    seg = ln - 40
    rec[:, 32:40] = (seg >> 24, (seg >> 16) & 255, (seg >> 8) & 255, seg & 255, 0, 0, 0, nh)
    rec[:, 40:] = v[:, 40:ln]
    raw, _ = port.batch_strided(rec.reshape(-1).copy(), n, ln, 0, ln, cgck.RAW)
    exp = (raw & 0xFFFF).astype(np.uint32) << 16
    ever = np.zeros(n, np.uint8)
    for i in chained:
        e1, v1, _ = ip6ref.expect(port, buf, [i * stride], [ln], GEN6)
        exp[i], ever[i] = e1[0], v1[0]
    return exp, ever


@pytest.mark.parametrize("stride,n,nh", [(1500, 140003, 6), (1508, 4099, 17)])
def test_ipv6(dstr_engine, port, stride, n, nh):
    """dstr6_kernel on the same geometry; every 997th frame carries a
    hop-by-hop header (finished from global memory by the frame's lane)."""
    ln = 1500
    rng = np.random.default_rng(stride + n)
    buf = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
    ip6ref.stamp_strided(buf, n, stride, ln, nh)
    chained = list(range(5, n, 997))
    for i in chained:
        buf[i * stride:i * stride + ln] = ip6ref.packet(rng, ln, nh, ((0, 8),))
    exp, ever = expect6(port, buf, n, stride, ln, nh, chained)
    # the batched reference is the frame-by-frame one (first and last frames)
    for i in list(range(0, min(n, 48))) + [n - 1]:
        e1, _, _ = ip6ref.expect(port, buf, [i * stride], [ln], GEN6)
        assert e1[0] == exp[i], i
    out, ver, kern = run(dstr_engine, buf, n, stride, 0, ln, GEN6)
    assert kern.startswith("dstr6_kernel<"), kern
    bad = np.nonzero((out != exp) | (ver != ever))[0]
    assert len(bad) == 0, f"{len(bad)} mismatches, first {bad[:5]}, got {out[bad[:5]]} want {exp[bad[:5]]}"
