"""cgck_steer without a device: the referee (tests/steerref.py) against a naive
bucket loop, the plan (cgck_test_steer_plan, csrc/cgck_steer_plan.cpp) over a
sweep of (n, queue_num), and the header's prototypes."""
import ctypes
import os
import re

import numpy as np
import pytest

import cgck
import steerref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a tile is a multiple of the workgroup's four 64-frame wave-steps,
# and tiles x (queue_num + 1) stays within 64 scan passes of 4096 words.
STEP = 256
BASE_TILE = 4096
BUDGET = 64 * 4096
EINVAL = -22

NS = sorted({0, 1, 2 ** 32 - 1} | {2 ** e + d for e in range(1, 32) for d in (-1, 0, 1)} | {2 ** 32 - 2})
QUEUES = (1, 2, 7, 128)


def test_referee_is_a_stable_bucket_loop():
    rng = np.random.default_rng(11)
    for case in range(300):
        n = int(rng.integers(0, 400))
        qn = int(rng.choice((1, 2, 3, 7, 8, 127, 128)))
        pool = np.concatenate((np.arange(min(qn, 12)), [qn - 1, qn % 256, 200, 255])).astype(np.uint8)
        queue = rng.integers(0, 256, n, dtype=np.uint8) if case % 3 == 0 else rng.choice(pool, n)
        qoff, perm, slot, desc = steerref.expect(queue, qn, np.arange(n) * 7)
        loop = steerref.bucket_loop(queue, qn)
        assert qoff.tolist() == loop[0] and perm.tolist() == loop[1] and slot.tolist() == loop[2]
        assert desc.tolist() == [7 * k for k in loop[1]]
        assert qoff.dtype == perm.dtype == slot.dtype == np.uint32


def test_referee_edges():
    qoff, perm, slot, _ = steerref.expect(np.zeros(0, np.uint8), 8)
    assert qoff.tolist() == [0] * 10 and len(perm) == 0 and len(slot) == 0
    qoff, perm, slot, _ = steerref.expect(np.array([0xFF, 1, 8, 1, 0, 200], np.uint8), 8)
    assert qoff.tolist() == [0, 1, 3, 3, 3, 3, 3, 3, 3, 6]
    assert perm.tolist() == [4, 1, 3, 0, 2, 5] and slot.tolist() == [3, 1, 4, 2, 0, 5]


@pytest.mark.parametrize("qn", QUEUES)
def test_plan_sweep(qn):
    L = cgck.load()
    last = 0
    for n in NS:
        tile, tiles, work = cgck.steer_plan(n, qn)
        what = f"n {n} queue_num {qn}: tile {tile} tiles {tiles} work {work}"
        assert tiles == -(-n // tile), what
        assert tile % STEP == 0 and tile >= BASE_TILE, what
        assert tile & (tile - 1) == 0, what                       # doubling from the base tile
        assert tiles * (qn + 1) <= BUDGET, what
        assert tile == BASE_TILE or -(-n // (tile // 2)) * (qn + 1) > BUDGET, what   # no larger than needed
        assert (work == 0) == (tiles <= 1), what
        # the histogram fits; past the base tile the whole budget is asked for
        assert work == (0 if tiles <= 1 else 4 * tiles * (qn + 1) if tile == BASE_TILE else 4 * BUDGET), what
        assert work >= last, what
        last = work
        assert L.cgck_steer_work_bytes(n, qn) == work, what
        assert cgck.steer_work_bytes(n, qn) == work, what


def test_plan_one_tile_is_every_burst():
    for qn in (1, 8, 128):
        for n in (1, 64, 256, 1024, 4096):
            assert cgck.steer_plan(n, qn) == (BASE_TILE, 1, 0)
        assert cgck.steer_plan(0, qn) == (BASE_TILE, 0, 0)
        assert cgck.steer_plan(4097, qn) == (BASE_TILE, 2, 8 * (qn + 1))


def test_plan_arguments():
    L = cgck.load()
    t, m, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t()
    by = ctypes.byref
    for n, qn in ((10, 0), (10, 129), (2 ** 32, 8)):
        assert L.cgck_test_steer_plan(n, qn, by(t), by(m), by(w)) == EINVAL
        assert L.cgck_steer_work_bytes(n, qn) == 0
    assert L.cgck_test_steer_plan(10 ** 6, 8, None, None, None) == 0
    assert L.cgck_test_steer_plan(10 ** 6, 8, None, by(m), None) == 0 and m.value == 245


def test_header_prototypes():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for proto in (
            "size_t cgck_steer_work_bytes(uint64_t n, uint32_t queue_num);",
            "int cgck_steer(cgck_ctx_t *ctx, const uint8_t *queue, uint64_t n, uint32_t queue_num, "
            "const cgck_desc_t *desc_in, const cgck_steer_res_t *res, void *work, void *stream);",
            "int cgck_rss_steer_desc(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *desc, uint64_t n, "
            "const cgck_rss_spec_t *spec, const cgck_rss_res_t *rss, const cgck_steer_res_t *res, "
            "void *work, void *stream);",
            "int cgck_test_steer_plan(uint64_t n, uint32_t queue_num, uint32_t *tile, uint32_t *tiles, "
            "size_t *work_bytes);"):
        assert proto in flat, proto
    m = re.search(r"typedef struct cgck_steer_res \{(.*?)\} cgck_steer_res_t;", hdr, re.S)
    assert m, "struct cgck_steer_res"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "uint32_t *qoff; uint32_t *perm; uint32_t *slot; cgck_desc_t *desc_out;"
    assert ctypes.sizeof(cgck.SteerRes) == 32
    assert [f[0] for f in cgck.SteerRes._fields_] == ["qoff", "perm", "slot", "desc_out"]
    assert cgck.load().cgck_abi_version() == 2
