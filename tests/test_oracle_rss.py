"""The Toeplitz RSS restatement (oracle/rss_oracle.c) against the fixtures made
from the reference's own toeplitz_hash / rss_hash4 (tests/golden/rss.json),
the published Microsoft RSS verification vectors, and — where the reference
build is present — randomized differential cases.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    with open(os.path.join(GOLDEN, "rss.json")) as f:
        return json.load(f)


def hexa(s):
    return np.frombuffer(bytes.fromhex(s), np.uint8).copy()


def test_ms_vectors(port, g):
    key = hexa(g["freebsd_rss_key"])
    for v in g["ms_vectors"]:
        d = hexa(v["data_hex"])
        assert port.toeplitz_hash(d, key) == v["ipv4_tcp"]
        assert port.toeplitz_hash(d[:8], key) == v["ipv4"]
        assert port.rss_hash4(v["laddr"], v["faddr"], v["lport"], v["fport"], key) == v["rss_hash4"]
        assert v["rss_hash4"] == v["ipv4_tcp"] & 0x7F


def test_toeplitz_grid(port, g):
    t = g["toeplitz_grid"]
    buf, key = hexa(t["data_hex"]), hexa(t["key_hex"])
    for ks, row in zip(t["key_sizes"], t["hash"]):
        got = [port.toeplitz_hash(buf, key, c, ks) for c in t["cnts"]]
        assert got == row, f"key_size {ks}"


def test_tuples12(port, g):
    key = hexa(g["freebsd_rss_key"])
    d = hexa(g["tuples12"]["data_hex"])
    out = port.toeplitz_batch(d, 4096, 12, 12, key)
    assert out.tolist() == g["tuples12"]["hash"]
    out7 = port.toeplitz_batch(d, 4096, 12, 12, key, mask=0x7F)
    assert np.array_equal(out7, out & 0x7F)


def dst_run(port, g, s, **kw):
    key = hexa(g["keys"][s["key"]])
    return port.dst_cache(s["laddr"][0], s["laddr"][1], s["faddr"][0], s["faddr"][1], s["fport"],
                          s["queue_num"], s["queue_id"], key, s["cap"], **kw)


def test_dst_sets(port, g):
    """The restated loop with the restated hash reproduces every set."""
    for s in g["dst_sets"]:
        if s["count"] > 400000:
            continue   # the large sets run on the GPU side; keep the CPU suite fast
        e = dst_run(port, g, s)
        assert len(e) == s["count"], s["name"]
        assert hashlib.sha256(e.tobytes()).hexdigest() == s["sha256"], s["name"]
        if len(e):
            assert e[:32].tobytes().hex() == s["head"]
            assert e[-32:].tobytes().hex() == s["tail"]


def test_dst_semantics(port, g):
    """Spot semantics of con-gen.c:291-360 on the default set."""
    s = g["dst_sets"][0]
    key = hexa(g["keys"]["freebsd"])
    e = dst_run(port, g, s)
    # every entry passes the filter, ports are ephemeral, SO_HASH as subr.h:179
    for x in e[:500]:
        h = port.rss_hash4(int(x["laddr"]), int(x["faddr"]), int(x["lport"]), int(x["fport"]), key)
        assert h % s["queue_num"] == s["queue_id"]
        lp = int.from_bytes(int(x["lport"]).to_bytes(2, "little"), "big")
        assert 5000 <= lp <= 65535
        fa, lpt, fpt = int(x["faddr"]), int(x["lport"]), int(x["fport"])
        so = fa ^ (fa >> 16) ^ int.from_bytes(((lpt ^ fpt) & 0xFFFF).to_bytes(2, "little"), "big")
        assert int(x["hash"]) == so


def test_differential_vs_reference(port, g):
    """Random cases against the values recorded from the reference build
    (tests/golden/differential.json) and, where it is present, side by side."""
    import refcases
    d = refcases.golden()["rss_random"]
    key = hexa(g["freebsd_rss_key"])
    t, r = refcases.rss_random(port, key)
    assert (len(t), len(r)) == (3000, 2000)
    assert t == d["toeplitz_hash"] and r == d["rss_hash4"]
    R = oracle.reference_rss()
    if R is not None:
        assert np.array_equal(R.key, key)
        assert refcases.rss_random(R, R.key) == (t, r)


def test_dst_loop_with_reference_hash(port, g):
    """The restated loop around the reference's rss_hash4: the entries the
    fixture recorded from exactly that pair (make_golden.py rss_main), and
    the live pair where the reference build is present."""
    s = g["dst_sets"][1]
    a = dst_run(port, g, s)
    assert len(a) == s["count"] and hashlib.sha256(a.tobytes()).hexdigest() == s["sha256"]
    R = oracle.reference_rss()
    if R is not None:
        b = dst_run(port, g, s, hash_fn=R.fn_rss_hash4())
        assert np.array_equal(a, b)
