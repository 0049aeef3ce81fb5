#!/usr/bin/env python3
"""Transmit fills and receive verifies with counters on the mixed-length set,
within one build: what lpf_kernel gains over the path
such batches took before it (slot2_kernel), and what the stores and counters
cost against lpw's plain generate.

One process, HIP events, 5 warm-ups and the median of 20 launches per leg, the
legs run a b c d e twice, and the whole repeated on a second allocation made
while the first is held.  16M-packet IMIX set, packed and again in 2048 B ring
slots at +14, at the 354 B descriptor length hint:
  a  GEN_BOTH, auto                               lpw_kernel (the yardstick)
  b  FILL_BOTH, auto                              the shipped choice
  c  FILL_BOTH, pinned "slot2"                    slot2_kernel (the path before lpf)
  d  VERIFY_TOY + verdicts + bad counters, auto   the shipped choice
  e  as d, pinned "slot2"                         slot2_kernel
The buffer is filled once before the first leg (FILL_BOTH is idempotent under
ZERO_FIELDS, so every later fill writes the same bytes and every verify sees
good sums).  After every leg 64 sampled packets are checked against the oracle
(outputs, for d / e verdicts and counters too); after b and c the sampled
frames' bytes as well.

    python tools/fill_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table.  Algorithmic bytes: cgck_imix_bytes(n) +
16 n, as tools/ab_inproc.py counts them (the 2-4 written bytes per packet are
not added).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "con-gen_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cgck  # noqa: E402
import oracle  # noqa: E402

SEED = 0xF11
HBM_PEAK = 8.0e12
IMIX = (64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576)
HINT = sum(IMIX) // 12   # 354

LEGS = (("a_gen", cgck.GEN_BOTH, "auto", False), ("b_fill", cgck.FILL_BOTH, "auto", False),
        ("c_fill_slot2", cgck.FILL_BOTH, "slot2", False), ("d_verify_bad", cgck.VERIFY_TOY, "auto", True),
        ("e_verify_bad_slot2", cgck.VERIFY_TOY, "slot2", True))


def time_desc(eng, buf, desc, out, ver, bad, n, flags, warm=5, reps=20):
    a, b = cgck.Event(), cgck.Event()
    v, c = (ver.ptr, bad.ptr) if ver else (None, None)
    for _ in range(warm):
        eng.desc(buf.ptr, desc.ptr, n, flags, out.ptr, v, c)
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.record(a)
        eng.desc(buf.ptr, desc.ptr, n, flags, out.ptr, v, c)
        eng.record(b)
        eng.sync()
        ms.append(eng.elapsed_ms(a, b))
    return statistics.median(ms), min(ms), max(ms), eng.last_kernel


def check(eng, P, buf, out, ver, n, stride, l3, flags, frames):
    """64 packets spread over the batch against the oracle: the generator's
    frame restated (stream bytes, IMIX offsets, the IPv4 stamp), filled, then
    run with the leg's flags.  frames: compare the device frame's bytes too."""
    got, gv = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    out.download(got, stream=eng.stream)
    if ver:
        ver.download(gv, stream=eng.stream)
    eng.sync()
    bad = 0
    d1 = np.zeros(1, cgck.DESC_DTYPE)
    for k in np.linspace(0, n - 1, 64).astype(np.int64):
        off, ln = P.imix_desc(int(k))
        if stride:
            off = int(k) * stride + l3
        p = P.stream_bytes(off, ln, SEED)
        P.stamp_header(p, 0, ln)
        d1[0] = (0, 0, ln)
        P.batch_desc(p, d1.view(np.uint8), 1, cgck.FILL_BOTH)        # the state every leg runs on
        eo, ev = P.batch_desc(p, d1.view(np.uint8), 1, flags)
        bad += int(got[k]) != int(eo[0]) or (ver is not None and int(gv[k]) != int(ev[0]))
        if frames:
            dev = np.zeros(ln, np.uint8)
            buf.download(dev, off=off, stream=eng.stream)
            eng.sync()
            bad += not np.array_equal(dev, p)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    P = oracle.port()
    eng = cgck.Engine(0)
    eng.set_desc_len_hint(HINT)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    layouts = (("packed", 0, 0), ("ring", 2048, 14))
    algo = cgck.load().cgck_imix_bytes(n) + 16 * n
    rows, held = [], []
    for alloc in (0, 1):
        for name, stride, l3 in layouts:
            buf = cgck.DeviceBuffer(n * stride if stride else cgck.load().cgck_imix_bytes(n))
            desc, out, ver, cnt = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n),
                                   cgck.DeviceBuffer(8))
            held += [buf, desc, out, ver, cnt]   # the second allocation is made while the first is held
            (eng.synth_imix_ring(buf.ptr, desc.ptr, n, stride, l3, SEED) if stride else
             eng.synth_imix(buf.ptr, desc.ptr, n, SEED))
            eng.set_kernel("slot2")
            eng.desc(buf.ptr, desc.ptr, n, cgck.FILL_BOTH)   # good sums for every leg
            eng.set_kernel("auto")
            for rnd in (0, 1):
                for leg, flags, family, counted in LEGS:
                    cgck.load().cgck_memset(cnt.ptr, 0, 8, eng.stream)
                    eng.set_kernel(family)
                    med, lo, hi, kern = time_desc(eng, buf, desc, out, ver if counted else None, cnt, n, flags)
                    eng.set_kernel("auto")
                    bad = check(eng, P, buf, out, ver if counted else None, n, stride, l3, flags,
                                bool(flags & cgck.STORE))
                    c = np.zeros(2, np.uint32)
                    cnt.download(c, stream=eng.stream)
                    eng.sync()
                    r = {"alloc": alloc, "layout": name, "leg": leg, "round": rnd, "packets": n,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "pct_hbm_peak": round(100 * algo / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                         "oracle_mismatches_of_64": bad, "bad_counters": c.tolist()}
                    rows.append(r)
                    emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()

    def med_of(name, leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["layout"] == name and r["leg"] == leg
                                 and alloc in (None, r["alloc"]))

    def spread(name, leg):
        a0, a1 = med_of(name, leg, 0), med_of(name, leg, 1)
        return 100 * abs(a0 - a1) / min(a0, a1)

    emit("")
    emit(f"{'layout':7} {'leg':19} {'kernel':30} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  % peak  vs a")
    for name, _, _ in layouts:
        for leg, _, _, _ in LEGS:
            sel = [r for r in rows if r["layout"] == name and r["leg"] == leg]
            med = med_of(name, leg)
            emit(f"{name:7} {leg:19} {sel[0]['kernel']:30} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {100 * algo / (med * 1e-3) / HBM_PEAK:5.1f}  {med / med_of(name, 'a_gen'):6.3f}")
        for new, old, what in (("b_fill", "c_fill_slot2", "fill"), ("d_verify_bad", "e_verify_bad_slot2", "verify + counters")):
            x, y = med_of(name, new), med_of(name, old)
            emit(f"{name:7} {what}: auto / slot2 = {x / y:.3f} ({100 * (y - x) / y:+.2f} % of slot2's time saved); "
                 f"margin (slot2's spread between the two allocations) {spread(name, old):.2f} %")
    emit(f"oracle mismatches over all legs: {sum(r['oracle_mismatches_of_64'] for r in rows)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
