"""The IPv6 IMIX generator's host side: the two calls are declared, exported and
wrapped, and the Python restatement the GPU tests compare them with
(tests/ip6batches.py: imix6) yields well-formed IPv6 frames at the oracle's
IMIX offsets.  No GPU."""
import numpy as np

import cgck
import ip6batches as B
import ip6ref

NAMES = ("cgck_synth_imix_ip6", "cgck_synth_imix_ring_ip6")


def test_exports():
    L = cgck.load()
    for name in NAMES:
        assert name in cgck.EXPORTS
        assert hasattr(L, name), name
    assert callable(cgck.Engine.synth_imix_ip6) and callable(cgck.Engine.synth_imix_ring_ip6)
    assert L.cgck_abi_version() == 2


def test_restatement(port):
    n = 100
    for stride, l3 in ((0, 0), (2048, 14)):
        for nh in (6, 17, 58, 59):
            buf, desc, offs, lens = B.imix6(port, n, nh, 0xBEEF, stride, l3)
            plain = port.stream_bytes(0, buf.nbytes, 0xBEEF)
            touched = np.zeros(buf.nbytes, bool)
            for k in range(n):
                off, ln = port.imix_desc(k)
                assert ln == B.IMIX_CYCLE[k % 12] and lens[k] == ln
                assert offs[k] == (k * stride + l3 if stride else off)
                assert desc["frame_off"][k] + desc["l3_off"][k] == offs[k] and desc["ip_len"][k] == ln
                p = buf[offs[k]:offs[k] + ln]
                assert ip6ref.walk(p, ln) == (40, nh, ip6ref.OK)
                assert bytes(p[:7]) == bytes((0x60, 0, 0, 0, (ln - 40) >> 8, (ln - 40) & 255, nh))
                touched[offs[k]:offs[k] + 7] = True
                if nh in ip6ref.FIELD:
                    f = offs[k] + 40 + ip6ref.FIELD[nh]
                    assert not p[40 + ip6ref.FIELD[nh]:42 + ip6ref.FIELD[nh]].any()
                    touched[f:f + 2] = True
            assert np.array_equal(buf[~touched], plain[~touched])       # the stream's bytes everywhere else
            if not stride:
                assert np.all(offs[1:] == offs[:-1] + lens[:-1])        # back to back
