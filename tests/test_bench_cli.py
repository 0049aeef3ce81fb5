"""bench.py's command line: a plain run times the headline workload alone,
--full brings the other legs back, --dump-outputs writes what the last timed
step computed."""
import json
import subprocess
import sys

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_splits_the_halves(tmp_path):
    o = np.arange(70001, dtype=np.uint32) * np.uint32(2654435761)
    bench.dump_outputs(str(tmp_path / "d"), {"1500": {"out": o}})
    ip = np.load(tmp_path / "d" / "ip_cksum_1500.npy")
    tcp = np.load(tmp_path / "d" / "tcp_cksum_1500.npy")
    assert ip.dtype == tcp.dtype == np.float32
    assert np.array_equal(ip.astype(np.uint32) | (tcp.astype(np.uint32) << 16), o)


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """Above DUMP_PACKETS the same distinct packets, in ascending order, every run."""
    monkeypatch.setattr(bench, "DUMP_PACKETS", 1000)
    o = np.arange(70001, dtype=np.uint32)     # low half = the packet's index mod 65536
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"64": {"out": o}})
        ip = np.load(tmp_path / d / "ip_cksum_64.npy")
        tcp = np.load(tmp_path / d / "tcp_cksum_64.npy")
        got.append(ip.astype(np.int64) + (tcp.astype(np.int64) << 16))
    assert np.array_equal(got[0], got[1])
    assert len(got[0]) == 1000 and np.all(np.diff(got[0]) > 0) and got[0][-1] <= 70000


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, port):
    """One small plain run: the line carries ms_per_step and none of the
    --full legs, and the dumped arrays are the batch's checksums (oracle)."""
    import cgck
    n = 70001     # odd, several blocks
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--packets", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "Gpkt/s" and d["dtype"] == "u16"
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3) / 1e9)
    for k in ("parity", "cpu_baseline", "value_64B", "value_imix", "extra"):
        assert k not in d
    ip = np.load(tmp_path / "ip_cksum_1500.npy")
    tcp = np.load(tmp_path / "tcp_cksum_1500.npy")
    assert ip.dtype == tcp.dtype == np.float32 and len(ip) == len(tcp) == n
    o = ip.astype(np.uint32) | (tcp.astype(np.uint32) << 16)
    bad, chk = port.check_synth_strided(n, 1500, 1500, bench.SEED, cgck.GEN_BOTH, o)
    assert (bad, chk) == (0, n)
