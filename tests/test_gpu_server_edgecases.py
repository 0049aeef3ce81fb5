"""The edge-class corpus of edgecases.py through every body of the resident
burst server (burst_server_kernel, cgck_group.hip) and both host routes into
it: cgck_desc_host (staged, or in place on registered memory) and
cgck_burst_request.  A cell opens a server, sends its batch in the requests of
its plan and holds the outputs, the verdicts and the whole buffer after the
calls bit-exact against the oracle.  Before each request the library itself
names the route (cgck_test_burst_route, validated on the CPU by
test_server_routes_cpu.py) and the cell asserts it is the family's; that the
server, not a launch, served a cgck_desc_host call shows in
cgck_ctx_last_kernel, which a server request leaves at the sentinel a one-record
Toeplitz launch put there.  A mismatch names the class labels, the request, its
route and q = start & 15 of the first wrong frames.

test_server_slice_passes runs the second pass of a slice; the drop-in symbols
and the TX window go over zero-sum frames with this thread's server open and
closed, and the RX window replays the stacks over the corpus at three
alignments: the only ways into the bodies compiled for CGCK_RAW, CGCK_L4 |
kFlagNoLenCheck, kTxFlags, kTxFlags | kFlagL4Auto and kRxFlags."""
import fnmatch

import numpy as np
import pytest

import cgck
import edgecases as E
import rxcorpus
import test_gpu_windows as W   # replay_pair, replay_posted, tx_calls, expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sentinel(engine):
    """Sets cgck_ctx_last_kernel to a name no checksum launch produces."""
    data, out = cgck.DeviceBuffer(64), cgck.DeviceBuffer(64)
    key = np.arange(40, dtype=np.uint8)

    def mark():
        engine.toeplitz(data.ptr, 1, 12, 12, key, out.ptr)
        name = engine.last_kernel
        assert name.startswith("toeplitz"), name
        return name
    yield mark
    engine.sync()
    data.free()
    out.free()


def serve(engine, sentinel, b, flags, mem, max_pkts, max_bytes, windows, want):
    """Send frames [lo, hi) of b as one request per window; returns (out,
    verdict, the buffer after the calls, [(lo, hi, route)])."""
    L = cgck.load()
    out = np.full(b.n, 0xA5A5A5A5, np.uint32)
    ver = np.full(b.n, 0xA5, np.uint8)
    owner = ring = None
    if mem == E.PAGEABLE:
        got = b.buf.copy()
    else:
        owner, ring, size = rxcorpus.registered_copy(b.buf)
        got = ring[:len(b.buf)]
        assert L.cgck_host_register(ring.ctypes.data, size) == 0, cgck.last_error()
    routes = []
    engine.burst_open(max_pkts=max_pkts, max_bytes=max_bytes)
    try:
        dev = cgck.host_device_ptr(ring) if mem == E.REQUEST else None
        for lo, hi in windows:
            route = E.route_of(b, lo, hi, flags, mem, max_pkts, max_bytes)
            assert fnmatch.fnmatchcase(route, want), f"request {lo, hi} takes {route}, not {want}"
            routes.append((lo, hi, route))
            desc = np.ascontiguousarray(b.desc[lo:hi])
            if mem == E.REQUEST:
                rc = engine.burst_request(dev, len(b.buf), desc, flags, out[lo:hi], ver[lo:hi])
                assert rc == 0, f"request {lo, hi} ({route}): {rc} {cgck.last_error()}"
            else:
                mark = sentinel()
                engine.desc_host(got, desc, flags, out[lo:hi], ver[lo:hi])
                assert engine.last_kernel == mark, f"request {lo, hi} ({route}) was launched: {engine.last_kernel}"
        got = got.copy()
    finally:
        engine.burst_close()
        if ring is not None:
            assert L.cgck_host_unregister(ring.ctypes.data) == 0
    return out, ver, got, routes


def compare(what, b, routes, out, ver, got, exp, ever, after):
    def where(idx):
        idx = [int(i) for i in idx[:8]]
        req = {next((lo, hi, r) for lo, hi, r in routes if lo <= i < hi) for i in idx}
        return f"{b.labels(idx)} q {[int(b.starts[i]) & 15 for i in idx]} in requests {sorted(req)}"
    wrong = np.nonzero(out != exp)[0]
    assert len(wrong) == 0, (f"{what}: {len(wrong)} outputs differ: {where(wrong)} got {[hex(x) for x in out[wrong[:8]]]} "
                             f"want {[hex(x) for x in exp[wrong[:8]]]}")
    wrong = np.nonzero(ver != ever)[0]
    assert len(wrong) == 0, f"{what}: {len(wrong)} verdicts differ: {where(wrong)} got {ver[wrong[:8]]} want {ever[wrong[:8]]}"
    diff = np.nonzero(got != after)[0]
    if len(diff):
        hit = [i for i in range(b.n) if ((diff >= b.starts[i]) & (diff < b.starts[i] + len(b.frames[i].data))).any()][:8] \
            if b.n <= E.MAX_FRAMES else []
        assert False, f"{what}: {len(diff)} bytes differ after the calls, first at {diff[:8]}: {where(np.asarray(hit))}"


def run_cell(engine, sentinel, port, family, cell):
    flags = cell[1]
    b = E.cell_batch(port, cell)
    k, max_pkts, want = E.plan(cell)
    exp, ever, after = E.expect(port, b, flags)
    out, ver, got, routes = serve(engine, sentinel, b, flags, E.SERVER[family], max_pkts, E.SERVER_BYTES,
                                  E.requests(b, k), want)
    compare(f"{family} {E.cell_id(cell)} {want}", b, routes, out, ver, got, exp, ever, after)


def family_cells(family):
    return pytest.mark.parametrize("cell", E.cells(family), ids=E.cell_id)


@family_cells("srv_ldsp4")
def test_srv_ldsp4(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_ldsp4", cell)


@family_cells("srv_ldsp16")
def test_srv_ldsp16(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_ldsp16", cell)


@family_cells("srv_scratch")
def test_srv_scratch(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_scratch", cell)


@family_cells("srv_sys4")
def test_srv_sys4(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_sys4", cell)


@family_cells("srv_sys16")
def test_srv_sys16(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_sys16", cell)


@family_cells("srv_inplace")
def test_srv_inplace(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_inplace", cell)


@family_cells("srv_wide_staged")
def test_srv_wide_staged(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_wide_staged", cell)


@family_cells("srv_wide_inplace")
def test_srv_wide_inplace(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_wide_inplace", cell)


@family_cells("srv_store_host")
def test_srv_store_host(engine, sentinel, port, cell):
    run_cell(engine, sentinel, port, "srv_store_host", cell)


PASS_RUNS = [(mix, mem, flags) for mix, (_, flag_sets) in E.PASS_CELLS.items() for flags in flag_sets
             for mem in ((E.REQUEST,) if flags & cgck.STORE else (E.REQUEST, E.PAGEABLE))]


@pytest.mark.parametrize("mix,mem,flags", PASS_RUNS, ids=lambda v: v if isinstance(v, str) else f"{v:#x}")
def test_server_slice_passes(engine, sentinel, port, mix, mem, flags):
    """One request of PASS_N = 32 * 1024 + 71 frames to a server opened for as
    many (max_bytes 8 MiB: the mid mix staged is 6.4 MB): 32 workgroups, each a
    full pass of 1024 descriptors and a pass of 2 or 3.  Frame k of the request is
    frame (k + rot) % m of a small-mix or mid-mix corpus, overlapping in the one
    buffer, or (CGCK_FILL_BOTH) in copy k // m of it; test_server_routes_cpu.py
    holds that every class falls in a second pass."""
    where = "inplace" if mem == E.REQUEST else "staged"
    want = f"wide32/slice/{where}/{'g4' if mix == 'small' else 'g16'}u4+u1/rt/2passes"
    b = E.pass_batch(E.cell_batch(port, (E.PASS_CELLS[mix][0], flags)), want, tiled=bool(flags & cgck.STORE))
    exp, ever, after = E.expect(port, b, flags)
    out, ver, got, routes = serve(engine, sentinel, b, flags, mem, E.PASS_N, E.PASS_BYTES, [(0, E.PASS_N)], want)
    compare(f"passes {mix} {want} {flags:#x}", b, routes, out, ver, got, exp, ever, after)
    late = E.second_pass(want)
    assert np.array_equal(out[late], exp[late]) and np.array_equal(ver[late], ever[late])


DROPIN_LENS = (20, 41, 64, 99, 576, 1500)


@pytest.mark.parametrize("server", [True, False], ids=["server", "launch"])
def test_dropins_on_zero_sums(port, server):
    """in_cksum / ip_cksum / udp_cksum on every zero_* and fill frame of six
    lengths at buffer offsets 0 and 1, with this thread's burst server open (the
    LDS-resident bodies compiled for CGCK_RAW and CGCK_L4 | kFlagNoLenCheck) and
    closed (a launch a call), against the oracle; the crafted halves are 0xFFFF."""
    if server:
        cgck.burst_open(max_pkts=512, max_bytes=1 << 20)
    try:
        crafted = [0, 0, 0]
        for ln in DROPIN_LENS:
            rng = np.random.default_rng(0xD0 + ln)
            raw = [f for f in E.frames4(port, rng, ln, cgck.RAW) if f.cls != "hl_sweep"]
            gen = [f for f in E.frames4(port, rng, ln, E.G) if f.cls != "hl_sweep"]
            for off in (0, 1):
                for is_raw, f in [(True, f) for f in raw] + [(False, f) for f in gen]:
                    buf = np.concatenate([np.full(off, 0x5A, np.uint8), f.data, np.full(16, 0x5A, np.uint8)])
                    what = f"{f.label}({ln}) at {off}"
                    got = cgck.in_cksum(buf, off, ln)
                    assert got == port.in_cksum(buf, off, ln), what
                    if is_raw and f.lo_ffff:
                        assert got == 0xFFFF, what
                        crafted[0] += 1
                    hl = (int(f.data[0]) & 15) * 4
                    if is_raw or hl < 20 or hl > ln:
                        continue
                    got = cgck.ip_cksum(buf, off)
                    assert got == port.in_cksum(buf, off, hl), what
                    if f.lo_ffff:
                        assert got == 0xFFFF, what
                        crafted[1] += 1
                    got = cgck.udp_cksum(buf, off, ln - hl)
                    assert got == port.udp_cksum(buf, off, ln - hl), what
                    if f.hi_ffff:
                        assert got == 0xFFFF, what
                        crafted[2] += 1
        assert min(crafted) >= 2 * 3 * len(DROPIN_LENS), crafted
    finally:
        if server:
            cgck.burst_close()


TX_FIELD = {6: 16, 17: 6, 1: 2}


@pytest.mark.parametrize("mode", ["flush", "post"])
@pytest.mark.parametrize("server", [True, False], ids=["server", "launch"])
@pytest.mark.parametrize("protos,lens", [((6, 17), (64, 1500)), ((6, 17, 1), (64, 1500)), ((6, 17, 1), (64,))],
                         ids=["tcp_udp", "icmp", "small"])
def test_tx_window_zero_sums(port, server, mode, protos, lens):
    """A TX fill of zero_both frames (ip_hl 5; both sums multiples of 65535 with
    the fields read as zero, the ICMP message's without the pseudo-header) queued
    from a registered pool in the stack's call order: every field comes out FF FF
    and the pool equals the oracle's fill byte for byte, through cgck_tx_flush and
    cgck_tx_post / cgck_tx_complete, with this thread's server open (the bodies
    compiled for kTxFlags, and for kTxFlags | kFlagL4Auto when the fill holds
    ICMP) and closed."""
    rng = np.random.default_rng(0x7E + len(protos) + len(lens))
    pkts = []
    for rep in range(2):
        for ln in lens:
            for p in protos:
                flags = E.GZ | (cgck.L4_NOPSEUDO if p == 1 else 0)
                pkts.append((p, ln, E.zero_frame(port, rng, ln, 5, p, flags, 3)))
    raw, ring, size = rxcorpus.registered_copy(np.zeros(len(pkts) * 2048, np.uint8))
    slots = ring[:len(pkts) * 2048].reshape(len(pkts), 2048)
    before = np.zeros_like(slots)
    L = cgck.load()
    assert L.cgck_host_register(ring.ctypes.data, size) == 0
    if server:
        cgck.burst_open(max_pkts=512, max_bytes=1 << 20)
    try:
        cgck.tx_begin()
        for i, (p, ln, pkt) in enumerate(pkts):
            slots[i, 14:14 + ln] = pkt
            before[i, 14:14 + ln] = W.expected(port, pkt, TX_FIELD[p], icmp=p == 1)
            W.tx_calls(slots[i], ln, TX_FIELD[p], icmp=p == 1)
        if mode == "flush":
            assert cgck.tx_flush() == 2 * len(pkts)
        else:
            assert cgck.tx_post() == 2 * len(pkts)
            assert cgck.tx_complete() == 2 * len(pkts)
        for i, (p, ln, pkt) in enumerate(pkts):
            fo = 14 + 20 + TX_FIELD[p]
            assert slots[i, 14 + 10:14 + 12].tolist() == [0xFF, 0xFF], (i, p, ln, "ip_sum")
            assert slots[i, fo:fo + 2].tolist() == [0xFF, 0xFF], (i, p, ln, "L4 field")
        diff = np.nonzero(slots != before)
        assert len(diff[0]) == 0, f"pool differs from the oracle's fill in slots {sorted(set(diff[0].tolist()))[:8]}"
    finally:
        if server:
            cgck.burst_close()
        L.cgck_host_unregister(ring.ctypes.data)


RX_CELLS = [(0, 1, 1), (1, 1, 1), (0, 1, 2), (1, 2, 2), (0, 2, 2), (1, 1, 2)]   # stack, ip_in, tcp_in


@pytest.mark.parametrize("mode", ["sync", "posted"])
@pytest.mark.parametrize("l2", E.RX_L2)
def test_rx_window_edge_classes(port, l2, mode):
    """The RX window over the zero-sum, planted-field, 0xFF-payload and ip_hl
    sweep frames (E.rx_bursts: sane headers, so the stacks reach their verdicts;
    test_server_routes_cpu.py holds that the planted fields decide them), with
    this thread's server open, on a registered ring, the IPv4 header at l2 = 14,
    16 or 21 (q even, zero, odd): bursts of 16 mixed frames, of 64 frames of 64
    bytes and of 282, opened at once (cgck_rx_begin) or posted (cgck_rx_post /
    cgck_rx_begin_posted, read in place).  Outcomes, counters and ring bytes
    equal the reference replay; every checksum call the stack makes is answered
    from the window (served == d[0], served + d[1] == calls, d[1] == 0)."""
    R = W.referee(port)
    L = cgck.load()
    bursts = E.rx_bursts(port)
    raw, ring, size = rxcorpus.registered_copy(np.zeros(300 * rxcorpus.SLOT + 64, np.uint8))
    assert L.cgck_host_register(ring.ctypes.data, size) == 0
    cgck.burst_open(max_pkts=4096, max_bytes=8 << 20)
    try:
        for i, (name, frames) in enumerate(bursts):
            buf, desc = rxcorpus.ring([f.data for f in frames], l2)
            for cell in (RX_CELLS[i % 6], RX_CELLS[(i + 3) % 6]):
                what = (name, l2, mode, cell)
                if mode == "sync":
                    (a, ref), (b, got), m, served, d = W.replay_pair(port, buf, desc, *cell, ring)
                    assert np.array_equal(a[0], b[0]), (what, [frames[k].label for k in np.nonzero(a[0] != b[0])[0][:8]])
                    assert np.array_equal(a[1], b[1]), (what, a[1], b[1])
                    assert np.array_equal(ref, got), what
                    calls = int(b[1][4] + b[1][5])
                else:
                    got = ring[:len(buf)]
                    got[:] = buf
                    assert cgck.rx_post(got, desc) == len(desc)
                    served, d, calls = W.replay_posted(port, R, buf, desc, got, cell)
                assert served == d[0] and served + d[1] == calls, (what, served, d, calls)
                assert d[1] == 0 and calls > 0, (what, served, d, calls)
    finally:
        cgck.burst_close()
        L.cgck_host_unregister(ring.ctypes.data)
