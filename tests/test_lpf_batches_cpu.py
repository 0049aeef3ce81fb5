"""The inputs of the fill / counter GPU tests (tests/fillbatches.py), validated
with the oracle alone: the builders' frames are pairwise disjoint (a CGCK_STORE
batch must not overlap), a filled batch verifies clean, and planted corruption
is counted exactly.  No GPU."""
import numpy as np
import pytest

import cgck
import fillbatches as F
from batches import MIXES
from test_gpu_parity import random_batch

BAD = cgck.BAD_IP | 2   # BAD_IP | BAD_L4


def n_of(mix):
    return 40 if mix == "jumbo" else 3000


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_builders_disjoint(mix):
    rng = np.random.default_rng(3)
    for first_off in (0, 7):
        _, desc = F.packed(rng, n_of(mix), MIXES[mix], first_off)
        assert F.disjoint(desc), mix
    if max(MIXES[mix]) <= 2048 - 14:
        _, desc = F.ring(rng, 300, MIXES[mix])
        assert F.disjoint(desc)
        assert np.all(F.starts(desc) == 2048 * np.arange(300) + 14)
    _, desc = random_batch(rng, 700, 300)
    assert F.disjoint(desc)
    over = desc.copy()
    over[1] = over[0]
    assert not F.disjoint(over)


@pytest.mark.parametrize("mix", ["imix", "mtu", "wide", "jumbo"])
def test_fill_then_verify_is_clean(port, mix):
    rng = np.random.default_rng(5)
    for build in (F.packed, F.ring):
        if build is F.ring and max(MIXES[mix]) > 2048 - 14:
            continue
        buf, desc = build(rng, n_of(mix), MIXES[mix])
        before = buf.copy()
        port.batch_desc(buf, desc.view(np.uint8), len(desc), cgck.FILL_BOTH)
        assert not np.array_equal(buf, before)
        again = buf.copy()
        port.batch_desc(again, desc.view(np.uint8), len(desc), cgck.FILL_BOTH)
        assert np.array_equal(again, buf), "the fill is idempotent"
        _, ver = port.batch_desc(buf, desc.view(np.uint8), len(desc), cgck.VERIFY_TOY)
        # no bad bit on any frame, but for the few whose two fields are the same
        # two bytes (fields_coincide): the L4 sum was stored over the IP sum
        same = F.fields_coincide(buf, desc)
        assert not (ver[~same] & BAD).any(), (mix, np.nonzero(ver & BAD)[0][:8])
        assert not (ver[same] & 2).any() and same.sum() <= len(desc) // 50


def test_corrupt_counts(port):
    rng = np.random.default_rng(8)
    buf, desc = F.packed(rng, 3000, MIXES["imix"], plain=True)
    port.batch_desc(buf, desc.view(np.uint8), len(desc), cgck.FILL_BOTH)
    hit = F.corrupt(buf, desc, 10)
    assert len(hit) == 300
    _, ver = port.batch_desc(buf, desc.view(np.uint8), len(desc), cgck.VERIFY_TOY)
    assert np.array_equal(np.nonzero(ver & BAD)[0], hit)
    assert int(((ver & 2) != 0).sum()) == len(hit) and not (ver & cgck.BAD_IP).any()


def test_synth_reference_matches_oracle_imix(port):
    """synth_imix_ref's frames are the ones check_synth_imix / check_synth_ring
    compute on: their GEN_BOTH results pass those checks."""
    n = 100
    for slot, l3 in ((0, 0), (2048, 14)):
        buf, desc = F.synth_imix_ref(port, n, 0xC0C3, slot, l3)
        assert F.disjoint(desc)
        out, _ = port.batch_desc(buf, desc.view(np.uint8), n, cgck.GEN_BOTH)
        bad, chk = (port.check_synth_ring(n, slot, l3, 0xC0C3, cgck.GEN_BOTH, out) if slot
                    else port.check_synth_imix(n, 0xC0C3, cgck.GEN_BOTH, out))
        assert bad == 0 and chk == n
