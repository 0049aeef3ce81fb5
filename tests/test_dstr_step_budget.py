"""The steady loop of dstr_kernel<3, 16, true, 0> computes no per-step geometry
(cgck_dense_kernel.inc: a step's geometry is the same for every step and is
hoisted in front of the loops).  clang emits the device assembly for gfx950
here (no GPU); the test takes the loops that hold the counted wait
`s_waitcnt vmcnt(12)` and issue a full step's whole KiBs unconditionally
from the scalar base (the `global_load_lds_dwordx4 vN, s[a:b]` form: one such
loop per number of whole KiBs), and counts their instructions over all their
blocks, rare paths included.

The bound is "strictly below the loop of the commit before the hoisting",
whose counts, taken the same way from a compile of that commit, are PARENT
below (its one loop held the general issue(): a 64-bit multiply chain and two
64-bit compares and branches per DMA)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_guard  # noqa: E402

SRC = os.path.join(ROOT, "con-gen_amd", "csrc", "cgck_dense.hip")
KERNEL = "dstr_kernelILi3ELi16ELb1ELi0E"
# the parent's loop around vmcnt(12): 856 instructions in 89 blocks
PARENT = {"v_mul_lo_u32": 2, "v_cmp_u64": 28, "s_cbranch": 43, "instructions": 856}
SCALAR_BASE_DMA = re.compile(r"global_load_lds_dwordx4 v\d+, s\[\d+:\d+\]")


def loop_counts(ins):
    ops = [i["op"] for i in ins]
    return {"v_mul_lo_u32": sum(o.startswith("v_mul_lo_u32") for o in ops),
            "v_cmp_u64": sum(bool(re.match(r"v_cmpx?_\w+_u64", o)) for o in ops),
            "s_cbranch": sum(o.startswith("s_cbranch") for o in ops),
            "instructions": len(ops)}


@pytest.fixture(scope="module")
def wait_loops(tmp_path_factory):
    """[(instructions of the innermost loop, it issues scalar-base DMAs)] for
    every counted vmcnt(12) of the kernel."""
    out = str(tmp_path_factory.mktemp("isa") / "cgck_dense.s")
    text = isa_guard.device_asm(SRC, out, include_dirs=(os.path.join(ROOT, "include"),))
    _, body, _ = isa_guard.kernel_text(text, KERNEL)
    blocks = isa_guard.blocks_of(body)
    lp = isa_guard.loops(blocks)
    res = []
    for bi, b in enumerate(blocks):
        for ins in b["ins"]:
            if ins["op"] == "s_waitcnt" and ins["asm"] and isa_guard.vmcnt_of(ins["text"]) == 12:
                inner = min((x for x in lp.values() if bi in x), key=len)
                all_ins = [i for j in sorted(inner) for i in blocks[j]["ins"]]
                res.append((all_ins, any(SCALAR_BASE_DMA.match(i["text"]) for i in all_ins)))
    return res


def test_steady_loops_exist(wait_loops):
    """One loop per number of whole KiBs of a full step (0..5), and the loop
    of the general issue() for a wave's last steps."""
    hot = [l for l, fast in wait_loops if fast]
    rest = [l for l, fast in wait_loops if not fast]
    assert len(hot) == 6 and len(rest) == 1, (len(hot), len(rest))


def test_steady_loops_are_below_the_parent(wait_loops):
    hot = [l for l, fast in wait_loops if fast]
    assert hot
    for ins in hot:
        c = loop_counts(ins)
        print(c)
        assert c["v_mul_lo_u32"] == 0, c
        assert c["v_cmp_u64"] < PARENT["v_cmp_u64"], c
        assert c["s_cbranch"] < PARENT["s_cbranch"], c
        assert c["instructions"] < PARENT["instructions"], c
        # every DMA of the loop sits in the one statement of a full step
        dma = [i for i in ins if i["op"].startswith("global_load_lds")]
        assert len(dma) == 6 and all(i["asm"] for i in dma), len(dma)
