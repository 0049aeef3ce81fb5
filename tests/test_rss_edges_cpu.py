"""The conditions under which the edge tests of cgck_toeplitz and cgck_dst_cache
(tests/test_gpu_rss.py) mean something, proven on the CPU: the case lists of
tests/toepbatches.py reach every kernel under every mask, the caps they take
from the referee lie on the tile edges they claim, and the recovery of a tuple's
loop index agrees with the referee's order.  No device."""
import time

import numpy as np
import pytest

import toepbatches as TB
from conftest import load_golden


@pytest.fixture(scope="module")
def key():
    return np.frombuffer(bytes.fromhex(load_golden("rss.json")["keys"]["freebsd"]), np.uint8).copy()


@pytest.fixture(scope="module")
def full(port, key):
    """{name: the referee's whole enumeration} of the tile-edge configurations."""
    return {c["name"]: TB.referee(port, c, key) for c in TB.EDGE_CONFIGS}


def test_expected_kernel_rule():
    """The rule on the shapes the issue names one by one."""
    ek = TB.expected_kernel
    assert ek(0, 12, 12) is None
    for ds, os in ((d, o) for d in (0, 4, 8, 12, 1) for o in (0, 4, 8, 12)):
        want = TB.X4 if (ds, os) == (0, 0) else TB.B_LDS if ds == 1 else TB.W3
        assert ek(TB.ALIGN_N, 12, 12, ds, os) == want, (ds, os)
    for n in TB.X4_SIZES:
        assert ek(n, 12, 12) == (TB.W3 if n < 4 else TB.X4), n
    want = {(12, 16): TB.W3, (12, 4): TB.W3, (36, 36): TB.W9, (36, 40): TB.W9, (36, 4): TB.W9, (36, 37): TB.B_LDS,
            (35, 36): TB.B_LDS, (37, 40): TB.B_GLB, (11, 12): TB.B_LDS, (13, 16): TB.B_LDS, (1, 1): TB.B_LDS,
            (0, 8): TB.B_LDS, (12, 0): TB.W3, (40, 1): TB.B_GLB}
    assert set(want) == set(TB.GRID)
    for (cnt, stride), k in want.items():
        assert ek(TB.GRID_N, stride, cnt) == k, (cnt, stride)
    assert ek(3, 1, TB.MAX_CNT) == TB.B_GLB
    assert [ek(TB.pass_n(1 << 19), s, c) for s, c in TB.PASS_SHAPES] == [TB.W3, TB.W9, TB.B_LDS, TB.B_GLB]


def test_every_kernel_under_every_mask():
    by_mask = TB.cases_by_mask()
    assert set(by_mask) == set(TB.MASKS)
    for m, cases in by_mask.items():
        names = {TB.expected_kernel(*c) for c in cases}
        assert names == set(TB.KERNELS), (hex(m), names)
    assert [TB.expected_kernel(*c) for c in TB.MASK_CASES] == list(TB.KERNELS)


def test_x4_sizes_reach_the_group_edges():
    """ng = n / 4 in {255, 256, 257} with every n % 4, and the batches below two groups."""
    big = [n for n in TB.X4_SIZES if n >= 1000]
    assert {n // 4 for n in big} == {254, 255, 256, 257}
    for ng in (255, 256, 257):
        assert {n % 4 for n in big if n // 4 == ng} >= ({0, 1, 3} if ng != 257 else {0, 1}), ng
    assert {n % 4 for n in big} == {0, 1, 3} and 1023 in big       # 1023: ng 255 with the longest tail
    assert set(range(1, 6)) <= set(TB.X4_SIZES)
    assert TB.ALIGN_N == 4 * 256 + 4 * 37 + 3


def test_records_end_the_allocation():
    for n, stride, cnt, _, _ in TB.ALIGN_CASES + TB.X4_CASES + TB.GRID_CASES:
        d = TB.records(n, stride, cnt, 1)
        assert d.nbytes == (n - 1) * stride + cnt == TB.data_bytes(n, stride, cnt)


def test_overlapping_records(port, key):
    """toeplitz_batch with stride < cnt is toeplitz_hash on the overlapping slices."""
    for stride, cnt in ((1, 12), (4, 36), (1, 37), (0, 12)):
        n = 300
        d = TB.records(n, stride, cnt, 5)
        got = port.toeplitz_batch(d, n, stride, cnt, key)
        want = [port.toeplitz_hash(d[k * stride:k * stride + cnt].copy(), key) for k in range(n)]
        assert got.tolist() == want, (stride, cnt)
        if stride:
            assert len(set(want)) > n - 3, "the records of an overlapping batch differ"


def test_second_pass_records_differ(port, key):
    """The second-pass shapes at a small n: (nearly) every record hashes differently,
    so a record written by the wrong lane or pass shows."""
    for stride, cnt in TB.PASS_SHAPES:
        n = 5000
        h = port.toeplitz_batch(TB.records(n, stride, cnt, 9), n, stride, cnt, key)
        assert len(np.unique(h)) > n - 5, (stride, cnt)


@pytest.mark.parametrize("c", TB.EDGE_CONFIGS, ids=lambda c: c["name"])
def test_edge_caps(full, c):
    e = full[c["name"]]
    total = len(e)
    assert total > 0, "the enumeration is empty"
    l0, f0, nf = c["laddr"][0], c["faddr"][0], c["nf"]
    i = TB.tuple_index(e, l0, f0, nf)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < TB.tuples(c), "tuple_index does not follow the referee's order"
    if c["queue_num"] <= 1:
        assert np.array_equal(i, np.arange(total)), "without the filter every tuple is an entry"
    ck = TB.edge_counts(e, l0, f0, nf)
    assert all(a < b for a, b in zip(ck, ck[1:])) and 0 < ck[0] and ck[-1] < total, ck
    caps = TB.edge_caps(e, l0, f0, nf)
    assert caps == sorted(set(caps)) and caps[0] == 1 and caps[-1] == total + 1
    assert all(1 <= cap <= total + 1 for cap in caps)
    for x in ck + [total]:
        assert {x - 1, x, x + 1} <= set(caps) | {0}
    # the entry at a tile edge's count is the first one of the next tile
    for k, x in zip((1, 2, 16), ck):
        assert i[x - 1] < TB.TILE_EDGE * k <= i[x]


@pytest.mark.parametrize("c", TB.NF_CONFIGS + TB.LARGE_CONFIGS, ids=lambda c: c["name"])
def test_capped_configs(port, key, c):
    n = c["nl"] * c["nf"] * TB.NEPH
    assert n < 2 ** 32 and TB.tuples(c) == n, "the tuple count wraps"
    t0 = time.perf_counter()
    e = TB.referee(port, c, key, c["cap"])
    took = time.perf_counter() - t0
    assert len(e) == c["cap"], "the enumeration ends before cap: no early stop"
    assert took < 1.0, f"the referee took {took:.2f} s"
    i = TB.tuple_index(e, c["laddr"][0], c["faddr"][0], c["nf"])
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < n


def test_large_configs_are_large():
    for c in TB.LARGE_CONFIGS:
        assert c["nf"] == 70000 and TB.tuples(c) == 4237520000
        assert TB.tuples(c) // TB.TILE_EDGE > 500000      # half a million tiles


@pytest.mark.parametrize("c", TB.EMPTY_CONFIGS, ids=lambda c: c["name"])
def test_empty_configs(port, key, c):
    assert TB.tuples(c) == 0 and 0 in (c["nl"], c["nf"])
    assert len(TB.referee(port, c, key, c["cap"])) == 0
