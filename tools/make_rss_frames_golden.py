#!/usr/bin/env python3
"""Generate tests/golden/rss_frames.json: expected per-frame RSS hashes
(cgck_rss_strided / cgck_rss_desc / cgck_rss_desc_host) recorded with the
REFERENCE's own compiled toeplitz_hash and freebsd_rss_key
(oracle/_ref/libref_rss.so, built by oracle/build_ref.sh) over the tuples
tests/rssref.py finds.  Runs in the build container only:

    make -C oracle && python tools/make_rss_frames_golden.py

The file holds bytes and results only:
  "ms": Microsoft's published IPv4 and IPv6 verification tuples wrapped as minimal
        TCP frames, with the hash with ports ("tcp") and of the addresses alone
        ("ip"); the tool stops if the reference does not reproduce the published
        values.
  "frames": about 200 class frames (tests/rssbatches.py; none longer than 256
        bytes) as hex, and "sets": their hash and kind under hf = 0, TCP and
        TCP | UDP.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import oracle  # noqa: E402
import rssbatches as RB  # noqa: E402
import rssref  # noqa: E402

SETS = {"none": 0, "tcp": rssref.RSS_TCP, "tcp_udp": rssref.RSS_TCP | rssref.RSS_UDP}


def one(R, frame, hf):
    h, kind, _ = rssref.expect(R, frame, [0], [len(frame)], R.key, hf)
    return int(h[0]), int(kind[0])


def main():
    R = oracle.reference_rss()
    if R is None:
        sys.exit("make_rss_frames_golden: oracle/_ref/libref_rss.so missing (run make -C oracle)")
    with open(os.path.join(ROOT, "tests", "golden", "rss.json")) as f:
        old = json.load(f)
    assert bytes(R.key).hex() == old["freebsd_rss_key"]
    ms = []
    for v in old["ms_vectors"]:            # the published IPv4 tuples, as that fixture records them
        fr = RB.ms_frame4(np.frombuffer(bytes.fromhex(v["data_hex"]), np.uint8))
        tcp, ip = one(R, fr, rssref.RSS_TCP)[0], one(R, fr, 0)[0]
        assert (tcp, ip) == (v["ipv4_tcp"], v["ipv4"]), v
        ms.append({"frame": bytes(fr).hex(), "tcp": tcp, "ip": ip})
    for src, dst, sp, dp, want_tcp, want_ip in RB.MS_IP6:
        fr = RB.ms_frame6(src, dst, sp, dp)
        tcp, ip = one(R, fr, rssref.RSS_TCP)[0], one(R, fr, 0)[0]
        assert (tcp, ip) == (want_tcp, want_ip), (src, hex(tcp), hex(ip))
        ms.append({"frame": bytes(fr).hex(), "tcp": tcp, "ip": ip})

    rng = np.random.default_rng(0x5253)
    seen, frames = set(), []
    for f in RB.all_classes(rng):
        t = frozenset(RB.tags(f))
        if len(f) > 256 or (t in seen and len(frames) >= 150):
            continue
        seen.add(t)
        frames.append(f)
    frames = frames[:200]
    buf, _, offs, lens = RB.packed(rng, frames, 0)
    sets = {}
    for name, hf in SETS.items():
        h, kind, _ = rssref.expect(R, buf, offs, lens, R.key, hf)
        sets[name] = {"hf": hf, "hash": h.tolist(), "kind": kind.tolist()}
    have = set().union(*(RB.tags(f) for f in frames))
    short = {t for t in RB.REQUIRED if not any(t.endswith(f"len{n}") for n in (575, 576, 577, 1279, 1280, 1499, 1500, 1514))}
    assert short <= have, sorted(short - have)
    path = os.path.join(ROOT, "tests", "golden", "rss_frames.json")
    with open(path, "w") as f:
        json.dump({"note": "made by tools/make_rss_frames_golden.py with the reference's compiled toeplitz_hash "
                           "and freebsd_rss_key",
                   "key": bytes(R.key).hex(), "ms": ms, "frames": [bytes(f).hex() for f in frames], "sets": sets},
                  f, indent=0)
    print(f"{path}: {len(ms)} published tuples, {len(frames)} frames, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
