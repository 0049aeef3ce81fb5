"""Header, zero-sum and stored-field edge classes through every kernel family's
own finishing code.  Each cell sends one batch of edgecases.py (hl_sweep, fill,
zero_ip / zero_l4 / zero_both, stored; validated on the CPU by
test_edgecases_cpu.py) through one pinned family and holds the outputs, the
verdicts, the whole buffer after the call and the `bad` counters bit-exact
against the oracle, and the kernel that ran against the family's own name: a
fallback to another kernel cannot make a cell pass.  A mismatch names the
class labels of the frames it hit."""
import numpy as np
import pytest

import cgck
import edgecases as E

pytestmark = pytest.mark.gpu

PINS = {"lpd": "lpd", "lpa": "lpa", "dstr": "dstr", "lpw": "lpw", "slot2": "slot2", "lpp": "lpp", "group": "group"}
KERNEL = {"lpd": "lpd_kernel<", "lpa": "lpa_kernel<", "dstr": "dstr_kernel<", "lpw": "lpw_kernel<",
          "lpf": "lpf_kernel<", "lpf_bad": "lpf_kernel<", "slot2": "slot2_kernel<", "lpp": "lpp_kernel<",
          "group": "cksum_kernel<", "lpd6": "lpd6_kernel<", "lpa6": "lpa6_kernel<", "dstr6": "dstr6_kernel<",
          "lpw6": "lpw6_kernel<", "group6": "cksum6_kernel<"}
PIN_OF = {"lpf": "lpw", "lpf_bad": "lpw", "lpd6": "lpd", "lpa6": "lpa", "dstr6": "dstr", "lpw6": "lpw", "group6": "group"}


@pytest.fixture(scope="module")
def engines():
    es = {f: cgck.Engine(0, kernel=k) for f, k in PINS.items()}
    yield es
    for e in es.values():
        e.close()


def launch(e, b, flags, want_ver, want_bad):
    """Upload, cgck_strided or cgck_desc, download: (out, verdict | None, the
    buffer after the call, the bad counters | None, kernel)."""
    n = b.n
    bufs = [cgck.DeviceBuffer(b.buf.nbytes), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n), cgck.DeviceBuffer(8),
            cgck.DeviceBuffer(12 * n + 64)]
    d, o, v, c, dd = bufs
    try:
        d.upload(b.buf, stream=e.stream)
        L = cgck.load()
        L.cgck_memset(o.ptr, 0xA5, 4 * n, e.stream)
        L.cgck_memset(v.ptr, 0xA5, n, e.stream)
        L.cgck_memset(c.ptr, 0, 8, e.stream)
        vp, cp = v.ptr if want_ver else None, c.ptr if want_bad else None
        if b.desc is None:
            e.strided(d.ptr, n, b.stride, b.l3_off, b.ip_len, flags, o.ptr, vp, cp)
        else:
            dd.upload(b.desc, stream=e.stream)
            e.desc(d.ptr, dd.ptr, n, flags, o.ptr, vp, cp)
        kernel = e.last_kernel
        out, ver, got, bad = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.empty_like(b.buf), np.zeros(2, np.uint32)
        o.download(out, stream=e.stream)
        v.download(ver, stream=e.stream)
        d.download(got, stream=e.stream)
        c.download(bad, stream=e.stream)
        e.sync()
    finally:
        for x in bufs:
            x.free()
    return out, ver if want_ver else None, got, bad if want_bad else None, kernel


def run_cell(engines, port, family, cell, want_ver=True, want_bad=False):
    flags = cell[1]
    b = E.cell_batch(port, cell)
    exp, ever, after = E.expect(port, b, flags)
    out, ver, got, bad, kernel = launch(engines[PIN_OF.get(family, family)], b, flags, want_ver, want_bad)
    # (CGCK_RAW | CGCK_IP6 is CGCK_RAW: the family's IPv4 kernel runs it)
    own = KERNEL[family].replace("6_kernel", "_kernel") if flags & cgck.RAW else KERNEL[family]
    assert kernel.startswith(own), f"{family}: ran {kernel}"
    wrong = np.nonzero(out != exp)[0]
    assert len(wrong) == 0, (f"{family} {kernel}: {len(wrong)} outputs differ: {b.labels(wrong[:8])} "
                             f"got {[hex(x) for x in out[wrong[:8]]]} want {[hex(x) for x in exp[wrong[:8]]]}")
    if want_ver:
        wrong = np.nonzero(ver != ever)[0]
        assert len(wrong) == 0, (f"{family} {kernel}: {len(wrong)} verdicts differ: {b.labels(wrong[:8])} "
                                 f"got {ver[wrong[:8]]} want {ever[wrong[:8]]}")
    diff = np.nonzero(got != after)[0]
    assert len(diff) == 0, (f"{family} {kernel}: {len(diff)} bytes differ after the call, first at {diff[:8]}: "
                            f"{b.labels(b.at_byte(diff)[:8])}")
    if want_bad:
        want = [int(((ever & cgck.BAD_IP) != 0).sum()), int(((ever & cgck.BAD_L4) != 0).sum())]
        assert bad.tolist() == want and min(want) > 0, f"{family} {kernel}: bad counters {bad.tolist()} want {want}"


def family_cells(family):
    return pytest.mark.parametrize("cell", E.cells(family), ids=E.cell_id)


@family_cells("lpd")
def test_lpd(engines, port, cell):
    run_cell(engines, port, "lpd", cell, want_ver=False)   # lpd takes no verdict array


@family_cells("lpa")
def test_lpa(engines, port, cell):
    run_cell(engines, port, "lpa", cell)


@family_cells("dstr")
def test_dstr(engines, port, cell):
    run_cell(engines, port, "dstr", cell)


@family_cells("lpw")
def test_lpw(engines, port, cell):
    run_cell(engines, port, "lpw", cell)


@family_cells("lpf")
def test_lpf_stores(engines, port, cell):
    run_cell(engines, port, "lpf", cell)


@family_cells("lpf_bad")
def test_lpf_bad_counters(engines, port, cell):
    run_cell(engines, port, "lpf_bad", cell, want_bad=True)


@family_cells("slot2")
def test_slot2(engines, port, cell):
    run_cell(engines, port, "slot2", cell)


@family_cells("lpp")
def test_lpp(engines, port, cell):
    run_cell(engines, port, "lpp", cell)


@family_cells("group")
def test_group(engines, port, cell):
    run_cell(engines, port, "group", cell)


@family_cells("lpd6")
def test_lpd6(engines, port, cell):
    run_cell(engines, port, "lpd6", cell, want_ver=False)


@family_cells("lpa6")
def test_lpa6(engines, port, cell):
    run_cell(engines, port, "lpa6", cell)


@family_cells("dstr6")
def test_dstr6(engines, port, cell):
    run_cell(engines, port, "dstr6", cell)


@family_cells("lpw6")
def test_lpw6(engines, port, cell):
    run_cell(engines, port, "lpw6", cell)


@family_cells("group6")
def test_cksum6(engines, port, cell):
    run_cell(engines, port, "group6", cell)
