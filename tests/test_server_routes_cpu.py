"""The burst server's routes (burst_route(), con-gen_amd/csrc/cgck_route.cpp,
through cgck_test_burst_route) against the server cells of edgecases.py, on
the CPU: every request of every cell's plan takes the route its family names,
every kind of body a product request can reach is reached by a cell, and the
whole table is the recorded one (tests/golden/server_routes.txt), so a constant
that moves shows as a diff there, not as a cell quietly served by another body.
No GPU, no context."""
import fnmatch
import os
from collections import Counter

import numpy as np
import pytest

import cgck
import edgecases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "server_routes.txt")
FAMILIES = sorted(E.SERVER)


def cell_routes(port, family, cell):
    b = E.cell_batch(port, cell)
    k, max_pkts, _ = E.plan(cell)
    return [E.route_of(b, lo, hi, cell[1], E.SERVER[family], max_pkts) for lo, hi in E.requests(b, k)]


def pass_routes(port):
    """{(mix, staged or in place, flags): the route of the PASS_N-frame request}"""
    out = {}
    for mix, (shape, flag_sets) in E.PASS_CELLS.items():
        for flags in flag_sets:
            b = E.cell_batch(port, (shape, flags))
            for mem in (E.REQUEST,) if flags & cgck.STORE else (E.REQUEST, E.PAGEABLE):
                lens = b.lens[np.arange(E.PASS_N) % b.n]   # (a rotation moves no length out of the request)
                out[mix, mem, flags] = cgck.burst_route(E.PASS_N, E.PASS_BYTES, mem, lens, flags)
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_every_request_takes_the_familys_route(port, family):
    for cell in E.cells(family):
        b = E.cell_batch(port, cell)
        k, max_pkts, want = E.plan(cell)
        windows = E.requests(b, k)
        assert windows[0][0] == 0 and windows[-1][1] == b.n and len(windows) <= 72
        assert all(a[1] == c[0] and 0 < a[1] - a[0] <= k for a, c in zip(windows, windows[1:] + [(b.n, 0)]))
        for (lo, hi), got in zip(windows, cell_routes(port, family, cell)):
            assert fnmatch.fnmatchcase(got, want), f"{family} {E.cell_id(cell)} request {lo, hi}: {got}, not {want}"
    if E.SERVER[family] == E.PAGEABLE:   # by design: a pageable batch that stores is launched
        cell = E.cells(family)[0]
        b = E.cell_batch(port, cell)
        assert E.route_of(b, 0, 8, cgck.FILL_BOTH, E.PAGEABLE, 4096) == "launch"


def test_plans_cover_both_unrolls_and_every_alignment(port):
    """What the issue's table asks of the plans beyond the route: srv_scratch and
    srv_inplace at n <= 16 and above, the wide families on servers of 128 and
    4096 frames, and the in-place layouts together every q = start & 15."""
    for fam, ns in (("srv_scratch", (16, 48)), ("srv_inplace", (16, 48))):
        assert {dict(s[2])["plan_k"] for s in E.CELLS[fam][0]} == set(ns)
    for fam in ("srv_wide_staged", "srv_wide_inplace"):
        assert {dict(s[2])["plan_max_pkts"] for s in E.CELLS[fam][0]} == {128, 4096}
    for fam in ("srv_sys4", "srv_sys16", "srv_inplace"):
        qs = set()
        for cell in E.cells(fam):
            if cell[1] == E.G:
                qs |= set((E.cell_batch(port, cell).starts & 15).tolist())
        assert qs == set(range(16)), (fam, sorted(qs))
    long_ = E.cell_batch(port, (E.CELLS["srv_inplace"][0][2], E.G))
    assert int(long_.lens.min()) > 1536


def test_second_pass_holds_every_class(port):
    """test_server_slice_passes' condition: the hook reports two passes on 32
    workgroups, and among the frames that fall in second passes every class the
    corpus holds occurs, all six where the flags read the fields.  (A corpus whose
    flags read no field, CGCK_GEN_BOTH's, holds no `stored` frame, so for it the
    condition is the other five: narrower than "every class" in every run.)  The
    wide g4u4 and g16u1 kinds are reached by these requests alone: no srv_wide_*
    cell has a slice pass of more than 64 or fewer than 17 frames."""
    seen = set()
    for (mix, mem, flags), route in pass_routes(port).items():
        where = "inplace" if mem == E.REQUEST else "staged"
        g = "g4" if mix == "small" else "g16"
        assert route == f"wide32/slice/{where}/{g}u4+u1/rt/2passes", (mix, mem, flags, route)
        late = E.second_pass(route)
        assert len(late) == 71 and len(set(late)) == 71
        b = E.cell_batch(port, (E.PASS_CELLS[mix][0], flags))
        pb = E.pass_batch(b, route, tiled=bool(flags & cgck.STORE))
        assert pb.n == E.PASS_N
        got = Counter(pb.frames[k].cls for k in late)
        want = set(E.PASS_CLASSES) if E.reads_fields(flags) else set(E.PASS_CLASSES) - {"stored"}
        assert set(got) >= want, (mix, flags, got)
        if flags & cgck.STORE:
            assert E.disjoint(pb)
        seen |= set(got)
    assert seen >= set(E.PASS_CLASSES)


def table(port):
    """The route table: per family and cell the distinct routes of its requests
    with their counts, then the slice-pass requests, then the kinds."""
    lines = []
    for family in FAMILIES:
        for cell in E.cells(family):
            c = Counter(cell_routes(port, family, cell))
            lines.append(f"{family} {E.cell_id(cell)} " + " ".join(f"{r} x{c[r]}" for r in sorted(c)))
    for (mix, mem, flags), route in sorted(pass_routes(port).items()):
        lines.append(f"passes {mix} mem{mem} {flags:#x} {route}")
    for kind, product in cgck.burst_route_kinds().items():
        lines.append(f"kind {kind} {'product' if product else 'lab'}")
    return lines


def test_route_table_matches_recorded(port):
    got = table(port)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [f"{a!r} -> {b!r}" for a, b in zip(want, got) if a != b]
    assert not diff and len(got) == len(want), "routes differ from tests/golden/server_routes.txt:\n" + "\n".join(diff[:20])


def test_every_product_route_is_reached_by_a_cell(port):
    kinds = cgck.burst_route_kinds()
    reached = set()
    for family in FAMILIES:
        for cell in E.cells(family):
            for r in set(cell_routes(port, family, cell)):
                reached |= E.route_kinds(r)
    for route in pass_routes(port).values():
        reached |= E.route_kinds(route)
    assert reached <= set(kinds), sorted(reached - set(kinds))     # a name the library does not list
    product = {k for k, p in kinds.items() if p}
    assert product - reached == set(), f"no cell reaches {sorted(product - reached)}"
    assert not reached - product, f"cells reach lab-only bodies {sorted(reached - product)}"


def test_route_names():
    """Spot values of the hook itself, the two names the header quotes among them."""
    r = cgck.burst_route
    assert r(4096, 4 << 20, E.REQUEST, [1500] * 16, cgck.VERIFY_BSD) == "one/lds/sys/g16u1/fl"
    assert r(E.PASS_N, 8 << 20, E.REQUEST, [64] * E.PASS_N, E.G) == "wide32/slice/inplace/g4u4+u1/rt/2passes"
    assert r(4096, 4 << 20, E.PAGEABLE, [1500] * 5000, E.G) == "launch"             # above max_pkts
    assert r(4096, 1 << 16, E.PAGEABLE, [1500] * 64, E.G) == "launch"               # above max_bytes
    assert r(4096, 4 << 20, E.REQUEST, [1500] * 5000, E.G) == "refused"
    assert r(4096, 4 << 20, E.REQUEST, [64] * 4, E.G | cgck.IP6) == "refused"
    assert r(4096, 4 << 20, E.PAGEABLE, [64] * 4, E.G | cgck.IP6) == "launch"
    # registered memory is copied up to 32 KiB of block, read in place above or when posted
    assert r(4096, 4 << 20, E.REGISTERED, [1500] * 16, E.G) == "one/scratch/staged/g16u1/rt"
    assert r(4096, 4 << 20, E.REGISTERED, [1500] * 16, E.G, posted=True) == "one/lds/sys/g16u1/rt"
    assert r(4096, 4 << 20, E.REGISTERED, [1500] * 32, E.G) == "one/lds/inplace/g16u4/rt"
    assert r(4096, 4 << 20, E.PAGEABLE, [1] * 1, cgck.RAW) == "one/lds/ldsp/g4u1/fl"
    assert r(4096, 4 << 20, E.PAGEABLE, [64] * 40, cgck.VERIFY_BSD, n1=20) == "one/lds/ldsp/g4u1/rt"   # two parts


def test_rx_corpus_decides_outcomes(port):
    """test_rx_window_edge_classes' frames through the reference's own functions
    (oracle.reference(), the restatement where that build is absent): the planted
    fields of the `stored` frames decide accepted and dropped outcomes, on the IP
    header's sum and on the L4 sum, and both stacks make L4 calls."""
    import oracle
    import rxcorpus
    R = oracle.reference() or port
    name, frames = E.rx_bursts(port)[-1]
    assert name == "300" and len(frames) > 64
    assert {f.cls for f in frames} == {"zero_ip", "zero_l4", "zero_both", "stored", "fill", "hl_sweep"}
    assert all(20 <= f.hl * 4 <= len(f.data) for f in frames if f.cls == "hl_sweep")
    for l2 in E.RX_L2:
        buf, desc = rxcorpus.ring([f.data for f in frames], l2)
        assert set((desc["frame_off"] + desc["l3_off"]) & 15) == {l2 & 15}
        for stack, want in ((0, {0, 2, 3}), (1, {0, 2, 3})):
            res, ctr = port.replay_rx(*R.fn_pointers(), buf.copy(), desc.view(np.uint8), len(desc), stack, 2, 2)
            stored = {int(res[i]) for i, f in enumerate(frames) if f.cls == "stored"}
            assert stored >= want, (l2, stack, stored)       # accepted, dropped on the IP sum, on the L4 sum
            assert ctr[4] >= len(frames) - 10 and ctr[5] > 0, ctr
    sizes = Counter(len(fr) for _, fr in E.rx_bursts(port))
    assert sizes[16] >= 10 and sizes[64] >= 1 and max(sizes) > 64
    assert all(len(f.data) == 64 for n_, fr in E.rx_bursts(port) if len(fr) == 64 for f in fr)


def test_every_name_the_route_function_produces_is_listed():
    """A grid of arguments through the hook, the windows' internal flag sets and
    two-part requests included: every name it produces stands for listed kinds,
    product ones only (no lab option is set), and the grid reaches each of them,
    so the list's product / lab split is held by the function itself."""
    L = cgck.load()
    kinds = cgck.burst_route_kinds()
    product = {k for k, p in kinds.items() if p}
    rx, tx = cgck.IP | cgck.L4 | cgck.ZERO_FIELDS | 1 << 14 | 1 << 13, cgck.IP | cgck.L4 | cgck.ZERO_FIELDS
    name = __import__("ctypes").create_string_buffer(64)
    seen, other = set(), set()
    for max_pkts in (1, 64, 65, 128, 4096, E.PASS_N):
        for max_bytes in (4096, 4 << 20, 64 << 20):
            for mem in (E.PAGEABLE, E.REGISTERED, E.REQUEST):
                for posted in (0, 1):
                    for n in (1, 16, 17, 64, 65, 128, 1025, 2049, E.PASS_N):
                        for ln in (20, 80, 81, 1520, 1521, 4000):
                            for flags in (cgck.RAW, E.G, cgck.VERIFY_BSD, cgck.FILL_BOTH, rx, tx, tx | 1 << 14,
                                          cgck.L4 | 1 << 15, E.G | cgck.IP6):
                                for n1 in (0, 5, 40):
                                    assert L.cgck_test_burst_route(max_pkts, max_bytes, mem, posted, n, ln,
                                                                   n * ((ln + 15) & ~15), flags, n1, name, 64) == 0
                                    r = name.value.decode()
                                    (seen if "/" in r else other).add(r)
    assert other == {"launch", "refused"}
    reached = set().union(*(E.route_kinds(r) for r in seen))
    assert reached == product, (sorted(reached - product), sorted(product - reached))
