"""lpf_kernel (cgck_lpf.hip): lpw's streaming pipeline with the in-place field
stores of CGCK_STORE and the running bad counters, for IPv4 batches of mixed
lengths.  Every case is bit-exact against the oracle referee (port.batch_desc /
port.batch_strided): outputs, verdicts, the whole frame buffer (tail padding
included) and the kernel that ran.  The inputs are validated without a GPU in
test_lpf_batches_cpu.py."""
import numpy as np
import pytest

import cgck
import fillbatches as F
from batches import MIXES
from test_gpu_parity import pack_cases, page_ring, random_batch

pytestmark = pytest.mark.gpu
LPF = "lpf_kernel<"
HINT = 354   # the IMIX set's mean frame length


@pytest.fixture(scope="module")
def lpw():
    """An engine pinned to the lpw family ("lpw" pins lpf too), packed hint."""
    e = cgck.Engine(0, kernel="lpw")
    e.set_desc_layout(cgck.LAYOUT_PACKED)
    yield e
    e.close()


@pytest.fixture
def auto(engine):
    """The shared engine under the automatic choice at the IMIX hint."""
    engine.set_desc_len_hint(HINT)
    engine.set_desc_layout(cgck.LAYOUT_ANY)
    try:
        yield engine
    finally:
        engine.set_desc_layout(cgck.LAYOUT_ANY)
        engine.set_desc_len_hint(1500)


def launch(e, buf, desc, flags, want_out=True, want_ver=True, bad=None, desc_shift=0):
    """Upload, cgck_desc, download: (out | None, verdict | None, the buffer
    after the launch, kernel)."""
    n = len(desc)
    d = cgck.DeviceBuffer(buf.nbytes)
    dd = cgck.DeviceBuffer(desc.nbytes + 16)
    o = cgck.DeviceBuffer(4 * n) if want_out else None
    v = cgck.DeviceBuffer(n) if want_ver else None
    try:
        d.upload(buf, stream=e.stream)
        dd.upload(desc, off=desc_shift, stream=e.stream)
        e.desc(d.ptr, dd.ptr + desc_shift, n, flags, o.ptr if o else None, v.ptr if v else None, bad)
        kernel = e.last_kernel
        out = np.zeros(n, np.uint32) if want_out else None
        ver = np.zeros(n, np.uint8) if want_ver else None
        got = np.empty_like(buf)
        if o:
            o.download(out, stream=e.stream)
        if v:
            v.download(ver, stream=e.stream)
        d.download(got, stream=e.stream)
        e.sync()
    finally:
        for b in (d, dd, o, v):
            if b:
                b.free()
    return out, ver, got, kernel


def check(e, port, buf, desc, flags, want_out=True, want_ver=True, **kw):
    ref = buf.copy()
    exp, ever = port.batch_desc(ref, desc.view(np.uint8), len(desc), flags)
    out, ver, got, kernel = launch(e, buf, desc, flags, want_out, want_ver, **kw)
    if want_out:
        bad = np.nonzero(out != exp)[0]
        assert len(bad) == 0, (f"{len(bad)} outputs differ, first {bad[:5]}: got {out[bad[:5]]} want {exp[bad[:5]]} "
                               f"len {desc['ip_len'][bad[:5]]}")
    if want_ver:
        assert np.array_equal(ver, ever), np.nonzero(ver != ever)[0][:8]
    diff = np.nonzero(got != ref)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]}"
    return kernel


# 1. flag sets x mixes
@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("flags", [cgck.FILL_BOTH, cgck.IP | cgck.ZERO_FIELDS | cgck.STORE,
                                   cgck.VERIFY_BSD | cgck.STORE])
def test_store_batches(lpw, port, mix, flags):
    rng = np.random.default_rng(sum(map(ord, mix)) + flags)
    n = 40 if mix == "jumbo" else 3000   # jumbo: the steps take the global-memory fallback
    buf, desc = F.packed(rng, n, MIXES[mix], first_off=int(rng.integers(0, 16)))
    assert check(lpw, port, buf, desc, flags).startswith(LPF)


# 2. step, chunk and grid edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_step_and_chunk_edges(lpw, port, n):
    rng = np.random.default_rng(n)
    buf, desc = F.packed(rng, n, MIXES["imix"])
    for want_out, want_ver in ((True, True), (True, False), (False, True), (False, False)):
        k = check(lpw, port, buf, desc, cgck.FILL_BOTH, want_out, want_ver)
        assert k.startswith(LPF), k


# 3. chunks shared across lanes, steps and waves
@pytest.mark.parametrize("flags", [cgck.FILL_BOTH, cgck.VERIFY_BSD | cgck.STORE])
def test_shared_chunks(lpw, port, flags):
    rng = np.random.default_rng(33 + flags)
    buf, desc = F.packed(rng, 3000, [20, 21, 26, 40, 70, 577])
    s = F.starts(desc)
    buf[s] = 0x45
    assert set((s % 16).tolist()) == set(range(16))
    assert check(lpw, port, buf, desc, flags).startswith(LPF)


# 4. gathered steps
@pytest.mark.parametrize("n", [64, 1000])
def test_ring_slots(lpw, port, n):
    rng = np.random.default_rng(40 + n)
    buf, desc = F.ring(rng, n, MIXES["imix"])
    assert check(lpw, port, buf, desc, cgck.FILL_BOTH).startswith(LPF)


def test_scattered_odd_offsets(lpw, port):
    rng = np.random.default_rng(44)
    buf, desc = random_batch(rng, 700, 300)
    assert check(lpw, port, buf, desc, cgck.FILL_BOTH).startswith(LPF)


# 5. counters
def counters(e, bad):
    b = np.zeros(2, np.uint32)
    bad.download(b, stream=e.stream)
    e.sync()
    return b.tolist()


def test_bad_counters_golden(auto, golden_verify):
    cases = golden_verify["cases"]
    buf, desc = pack_cases(cases)
    bad = cgck.DeviceBuffer(8)
    cgck.load().cgck_memset(bad.ptr, 0, 8, auto.stream)
    _, v, _, kernel = launch(auto, buf, desc, cgck.VERIFY_BSD, want_out=False, bad=bad.ptr)
    b = counters(auto, bad)
    bad.free()
    assert kernel.startswith(LPF), kernel
    assert b[0] == sum(1 - c["bsd_ip"] for c in cases)
    assert b[1] == sum(1 - c["bsd_l4"] for c in cases)
    assert b[0] == int(((v & 1) != 0).sum()) and b[1] == int(((v & 2) != 0).sum())


def test_bad_counters_run_on(auto, port):
    rng = np.random.default_rng(55)
    buf, desc = F.packed(rng, 3000, MIXES["imix"], plain=True)
    port.batch_desc(buf, desc.view(np.uint8), len(desc), cgck.FILL_BOTH)
    hit = F.corrupt(buf, desc, 10)
    _, ever = port.batch_desc(buf.copy(), desc.view(np.uint8), len(desc), cgck.VERIFY_TOY)
    want = [int(((ever & 1) != 0).sum()), int(((ever & 2) != 0).sum())]
    assert want == [0, len(hit)]
    bad = cgck.DeviceBuffer(8)
    try:
        cgck.load().cgck_memset(bad.ptr, 0, 8, auto.stream)
        for rep in (1, 2):   # running counters: never reset by the library
            kernel = check(auto, port, buf, desc, cgck.VERIFY_TOY, bad=bad.ptr)
            assert kernel.startswith(LPF), kernel
            assert counters(auto, bad) == [rep * want[0], rep * want[1]]
        kernel = check(auto, port, buf, desc, cgck.GEN_BOTH, bad=bad.ptr)
        assert kernel.startswith(LPF), kernel
        assert counters(auto, bad) == [2 * want[0], 2 * want[1]]
    finally:
        bad.free()


# 6. the automatic choice
def test_dispatch(auto, port):
    rng = np.random.default_rng(66)
    buf, desc = F.packed(rng, 2000, MIXES["imix"])
    assert check(auto, port, buf, desc, cgck.FILL_BOTH).startswith("lpf_kernel<true")
    bad = cgck.DeviceBuffer(8)
    try:
        cgck.load().cgck_memset(bad.ptr, 0, 8, auto.stream)
        assert check(auto, port, buf, desc, cgck.GEN_BOTH, bad=bad.ptr).startswith("lpf_kernel<true")
    finally:
        bad.free()
    assert check(auto, port, buf, desc, cgck.GEN_BOTH).startswith("lpw_kernel<")
    # the one cell that did not clear its margin: a fill of frames
    # the caller says are packed stays on slot2; counters under that hint do not
    auto.set_desc_layout(cgck.LAYOUT_PACKED)
    assert check(auto, port, buf, desc, cgck.FILL_BOTH).startswith("slot2_kernel<")
    bad = cgck.DeviceBuffer(8)
    try:
        cgck.load().cgck_memset(bad.ptr, 0, 8, auto.stream)
        assert check(auto, port, buf, desc, cgck.VERIFY_TOY, bad=bad.ptr).startswith("lpf_kernel<true")
    finally:
        bad.free()
    auto.set_desc_layout(cgck.LAYOUT_ANY)
    # descriptors that cannot travel by DMA (not 16-byte aligned)
    k = check(auto, port, buf, desc, cgck.FILL_BOTH, desc_shift=4)
    assert not k.startswith((LPF, "lpw_kernel")), k
    for hint in (200, 1500):
        auto.set_desc_len_hint(hint)
        k = check(auto, port, buf, desc, cgck.FILL_BOTH)
        assert not k.startswith(LPF), (hint, k)
    auto.set_desc_len_hint(HINT)
    # strided, back to back
    n, ln = 1500, 576
    sb = rng.integers(0, 256, n * ln + 64, dtype=np.uint8)
    sb[0:n * ln:ln] = 0x45
    sb[9:n * ln:ln] = np.resize([6, 17, 1], n)
    ref = sb.copy()
    exp, ever = port.batch_strided(ref, n, ln, 0, ln, cgck.FILL_BOTH)
    got = sb.copy()
    out, ver = auto.run_host_strided(got, n, ln, 0, ln, cgck.FILL_BOTH)
    assert auto.last_kernel.startswith("lpf_kernel<false"), auto.last_kernel
    assert np.array_equal(out, exp) and np.array_equal(ver, ever) and np.array_equal(got, ref)


# 7. the host path
@pytest.mark.parametrize("how", ["staged", "registered", "registered_over_server_caps"])
def test_desc_host_fill(auto, port, how):
    rng = np.random.default_rng(77)
    buf, desc = F.packed(rng, 300, MIXES["imix"])
    ref = buf.copy()
    exp, ever = port.batch_desc(ref, desc.view(np.uint8), len(desc), cgck.FILL_BOTH)
    L = cgck.load()
    ring = None
    if how != "staged":
        raw, ring = page_ring(len(buf))
        ring[:len(buf)] = buf
        assert L.cgck_host_register(ring.ctypes.data, ring.nbytes) == 0
    if how == "registered_over_server_caps":
        auto.burst_open(max_pkts=64, max_bytes=1 << 20)   # 300 frames exceed it: the launch path
    try:
        got = buf.copy() if ring is None else ring[:len(buf)]
        out = np.zeros(len(desc), np.uint32)
        ver = np.zeros(len(desc), np.uint8)
        auto.desc_host(got, desc, cgck.FILL_BOTH, out, ver)
        kernel = auto.last_kernel
        assert np.array_equal(out, exp) and np.array_equal(ver, ever)
        assert np.array_equal(got, ref)
        assert kernel.startswith(LPF), kernel
    finally:
        if how == "registered_over_server_caps":
            auto.burst_close()
        if ring is not None:
            assert L.cgck_host_unregister(ring.ctypes.data) == 0


# 8. generate -> fill -> verify on the device
@pytest.mark.parametrize("slot,l3", [(0, 0), (2048, 14)])
def test_generate_fill_verify(auto, port, slot, l3):
    n, seed = 1000, 0xC0C4
    ref, rdesc = F.synth_imix_ref(port, n, seed, slot, l3)
    port.batch_desc(ref, rdesc.view(np.uint8), n, cgck.FILL_BOTH)
    nbytes = ref.nbytes
    buf, desc, ver, bad = (cgck.DeviceBuffer(nbytes), cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(n),
                           cgck.DeviceBuffer(8))
    try:
        if slot:
            auto.synth_imix_ring(buf.ptr, desc.ptr, n, slot, l3, seed)
        else:
            auto.synth_imix(buf.ptr, desc.ptr, n, seed)
        auto.desc(buf.ptr, desc.ptr, n, cgck.FILL_BOTH)
        k_fill = auto.last_kernel
        cgck.load().cgck_memset(bad.ptr, 0, 8, auto.stream)
        auto.desc(buf.ptr, desc.ptr, n, cgck.VERIFY_TOY, None, ver.ptr, bad.ptr)
        k_ver = auto.last_kernel
        got = np.zeros(nbytes, np.uint8)
        v = np.zeros(n, np.uint8)
        d = np.zeros(n, cgck.DESC_DTYPE)
        buf.download(got, stream=auto.stream)
        ver.download(v, stream=auto.stream)
        desc.download(d, stream=auto.stream)
        b = counters(auto, bad)
    finally:
        for x in (buf, desc, ver, bad):
            x.free()
    assert k_fill.startswith(LPF) and k_ver.startswith(LPF), (k_fill, k_ver)
    assert np.array_equal(d, rdesc)
    s = F.starts(rdesc)
    for k in range(n):
        a, z = int(s[k]), int(s[k]) + int(rdesc["ip_len"][k])
        assert np.array_equal(got[a:z], ref[a:z]), f"frame {k}"
    assert not v.any() and b == [0, 0]
