"""The kernel choice (choose(), con-gen_amd/csrc/cgck_choose.cpp) against its
recorded decision table, on the CPU: tools/dispatch_table (the product build)
and tools/dispatch_table_lab (-DCGCK_LAB=1) replay every batch and (pin, bits)
column of tests/golden/dispatch.txt / dispatch_lab.txt through choose() and
report what differs.  The fixtures were recorded from launch_cksum as it was
before choose() existed, its launchers stubbed, so they say what the dispatcher
did, not what choose() does.  No GPU, no libcgck, no HIP.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
PRODUCT = ["group", "lpp", "slot2", "lpa", "lpd", "lpw", "lpw6", "lpf", "dstr"]
LAB = PRODUCT + ["slot", "lppp", "lpp0", "lpp1", "lpp3", "span", "slotd", "stream"]


@pytest.fixture(scope="module")
def binaries():
    subprocess.run(["make", "-s", "-C", TOOLS, "dispatch_table", "dispatch_table_lab"], check=True)


@pytest.mark.parametrize("binary,fixture,kernels", [
    ("dispatch_table", "dispatch.txt", PRODUCT),
    ("dispatch_table_lab", "dispatch_lab.txt", LAB),
])
def test_choice_matches_recorded_table(binaries, binary, fixture, kernels):
    r = subprocess.run([os.path.join(TOOLS, binary), os.path.join(ROOT, "tests", "golden", fixture)],
                       capture_output=True, text=True)
    lines = r.stdout.splitlines()
    mismatches = [ln for ln in lines if "->" in ln]
    assert not mismatches, "%d decisions differ from the recorded table:\n%s" % (
        len(mismatches), "\n".join(mismatches[:40]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    totals = [ln.split() for ln in lines if ln.startswith("cases ")]
    assert len(totals) == 1 and int(totals[0][1]) > 100000 and int(totals[0][3]) == 0, totals
    reached = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("reached ")}
    # the binary lists every Kernel value of its build; the fixture reaches each
    assert sorted(reached) == sorted(kernels)
    assert all(reached[k] > 0 for k in kernels), reached
