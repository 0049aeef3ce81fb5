#!/usr/bin/env python3
"""Generate tests/golden/mixed.json: a CGCK_MIXED batch of about 200 packets of
every class the mixed tests name (tests/mixedbatches.py: IPv4 lengths, header
lengths, protocols, stored zero sums and the BAD_LEN lengths; IPv6 lengths, next
headers, extension chains and their failures; frames of neither family), with
the expected `out` and `verdict` of four flag sets computed by the REFERENCE's
own compiled in_cksum / udp_cksum (oracle/_ref/libref_cksum.so, built by
oracle/build_ref.sh) through tests/mixedref.expect_pure.  Runs in the build
container only:

    make -C oracle && python tools/make_mixed_golden.py

The file holds bytes and results only: {"note", "packets": [hex, ...], "sets":
{name: {"flags", "out": [...], "verdict": [...]}}}.  Half the packets carry
valid checksum fields (as a sender stores them), so the verify sets hold good
and bad verdicts of both families.  Long frames are left out to keep the file
small: the lengths 576 and 1500 appear once per family.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import ip6ref  # noqa: E402
import mixedbatches as MB  # noqa: E402
import mixedref as MR  # noqa: E402
import oracle  # noqa: E402

GEN_BOTH = MR.IP | MR.L4
SETS = {
    "gen_both": GEN_BOTH,
    "gen_both_zero_fields": GEN_BOTH | MR.ZERO_FIELDS,
    "verify_toy": GEN_BOTH | MR.VERIFY,
    "verify_bsd": GEN_BOTH | MR.VERIFY | MR.V_IP_ZERO_IS_FFFF | MR.V_UDP_ZERO_SKIP,
}


def main():
    R = oracle.reference()
    if R is None:
        sys.exit("make_mixed_golden: oracle/_ref/libref_cksum.so missing (run make -C oracle)")
    rng = np.random.default_rng(0x4D58)
    frames = MB.all_classes(rng)
    # one long frame of each length per family is enough here
    seen, keep = set(), []
    for f in frames:
        key = (int(f[0]) >> 4 if len(f) else -1, len(f))
        if len(f) >= 575 and key in seen:
            continue
        seen.add(key)
        keep.append(f)
    frames = keep
    # and random short packets of either family up to about 200
    for k in range(200 - len(frames)):
        ln = int(rng.integers(1, 140))
        if k % 9 == 8:
            frames.append(MB.other(rng, ln, int(rng.choice(MB.OTHER_V + (1, 7, 12)))))
        elif k % 2:
            ch = tuple((int(rng.choice((0, 43, 60, 51))), 8 * int(rng.integers(1, 3))) for _ in range(int(rng.integers(0, 3))))
            frames.append(ip6ref.packet(rng, ln, int(rng.choice((6, 17, 58, 59, 132))), ch))
        else:
            frames.append(MB.v4(rng, ln, int(rng.choice((1, 6, 17, 47, 132))), int(rng.choice((5, 5, 5, 6, 8, 15)))))
    buf, desc, offs, lens = MB.packed(rng, frames, 0)
    # valid fields in every second packet, by the reference's own functions
    out, _ = MR.expect_pure(R, buf, offs, lens, GEN_BOTH | MR.ZERO_FIELDS)
    for i in range(0, len(frames), 2):
        o, p = int(offs[i]), buf[int(offs[i]):int(offs[i]) + int(lens[i])]
        at = MB.l4_field_at(p)
        keep_udp0 = "v4_udpsum0" in MB.tags(p) or "v6_udpsum0" in MB.tags(p)
        if at is not None and not keep_udp0:
            buf[o + at], buf[o + at + 1] = (int(out[i]) >> 16) & 255, int(out[i]) >> 24
        if len(p) >= 20 and int(p[0]) >> 4 == 4 and len(p) >= 4 * (int(p[0]) & 15) and "v4_ipsum0" not in MB.tags(p):
            buf[o + 10], buf[o + 11] = int(out[i]) & 255, (int(out[i]) >> 8) & 255
    sets = {}
    for name, flags in SETS.items():
        o, v = MR.expect_pure(R, buf, offs, lens, flags)
        sets[name] = {"flags": flags | MR.MIXED, "out": o.tolist(), "verdict": v.tolist()}
    have = set().union(*(MB.tags(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)))
    assert MB.REQUIRED <= have, sorted(MB.REQUIRED - have)
    vt = np.array(sets["verify_toy"]["verdict"])
    assert all(np.count_nonzero(vt & b) for b in (MR.BAD_IP, MR.BAD_L4, MR.BAD_LEN, MR.NOT_IP)) and np.count_nonzero(vt == 0)
    packets = [bytes(buf[int(o):int(o) + int(ln)]).hex() for o, ln in zip(offs, lens)]
    path = os.path.join(ROOT, "tests", "golden", "mixed.json")
    with open(path, "w") as f:
        json.dump({"note": "made by tools/make_mixed_golden.py with the reference's compiled in_cksum / udp_cksum",
                   "packets": packets, "sets": sets}, f, indent=0)
    print(f"{path}: {len(packets)} packets, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
