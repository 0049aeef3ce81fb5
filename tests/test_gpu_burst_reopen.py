"""Reopening the burst server with another capacity on the same context.
cgck_burst_open builds the server's state (cgck::BurstServer, cgck_burst.h)
and assigns it at once, cgck_burst_close resets it whole: a field a reopen
left over from the server before it (the workgroup count, the slot size, the
seqs, the device-memory doorbell) would serve the next server's requests
wrong.  So: a one-workgroup server, a five-workgroup one, a one-workgroup one
again, every request exact against the port; a second open is refused and
leaves the server serving, a second close is a no-op."""
import errno

import numpy as np
import pytest

import cgck
from test_gpu_parity import check_burst, page_ring, random_batch

pytestmark = pytest.mark.gpu

SMALL = dict(max_pkts=16, max_bytes=4096)         # burst_wgs(16): one workgroup
LARGE = dict(max_pkts=2048, max_bytes=1 << 20)    # up to 32 workgroups of kBurstPerWG = 64 packets


def batch(seed, npk, max_len, fixed=False):
    """random_batch; fixed: every packet max_len (<= 64) bytes (its frames
    start at least 64 bytes apart)."""
    buf, desc = random_batch(np.random.default_rng(seed), npk, max_len)
    if fixed:
        assert max_len <= 64
        at = desc["frame_off"].astype(np.int64) + desc["l3_off"]
        desc["ip_len"] = max_len
        buf[at + 2], buf[at + 3] = max_len >> 8, max_len & 0xFF
    return buf, desc


def serve(eng, port, caps, buf, desc, what, route, ring=None):
    """One cgck_desc_host request (CGCK_GEN_BOTH) that the server opened with
    `caps` takes by `route`, exact against the port."""
    name = cgck.burst_route(caps["max_pkts"], caps["max_bytes"],
                            cgck.ROUTE_PAGEABLE if ring is None else cgck.ROUTE_REGISTERED,
                            desc["ip_len"], cgck.GEN_BOTH)
    assert name.startswith(route), (what, name)
    ref = buf.copy()
    exp, ever = port.batch_desc(ref, desc.view(np.uint8), len(desc), cgck.GEN_BOTH)
    if ring is None:
        got = buf.copy()
    else:
        ring[:len(buf)] = buf
        got = ring[:len(buf)]
    out = np.full(len(desc), 0xDEADBEEF, np.uint32)
    ver = np.full(len(desc), 0xEE, np.uint8)
    eng.desc_host(got, desc, cgck.GEN_BOTH, out, ver)
    check_burst(out, exp, ver, ever, got, ref, what, caps["max_pkts"], ring, desc)


def test_reopen_with_other_capacity(engine, port):
    L = cgck.load()
    raw, ring = page_ring(1 << 20)
    assert L.cgck_host_register(ring.ctypes.data, ring.nbytes) == 0
    try:
        engine.burst_open(**SMALL)
        assert L.cgck_burst_open(engine.ctx, 2048, 1 << 20, 0) == -errno.EBUSY
        assert "already open" in cgck.last_error()
        serve(engine, port, SMALL, *batch(7301, 3, 64, fixed=True), "small server, 3 x 64 B pageable", "one/")
        engine.burst_close()

        engine.burst_open(**LARGE)
        buf, desc = batch(7302, 300, 300)
        assert len(buf) <= ring.nbytes
        serve(engine, port, LARGE, buf, desc, "large server, 300 packets in the ring", "wide5/", ring)
        serve(engine, port, LARGE, *batch(7303, 1, 300), "large server, 1 packet in the ring", "one/", ring)
        engine.burst_close()

        engine.burst_open(**SMALL)
        serve(engine, port, SMALL, *batch(7304, 1, 300), "small server again, 1 staged packet", "one/")
        engine.burst_close()
        assert L.cgck_burst_close(engine.ctx) == 0
    finally:
        engine.burst_close()
        assert L.cgck_host_unregister(ring.ctypes.data) == 0
