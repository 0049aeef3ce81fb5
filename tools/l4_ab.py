#!/usr/bin/env python3
"""cgck_l4_desc (l4d_kernel) beside the per-frame hash of the same burst, in one
process.

The method is tools/l2_ab.py's: HIP events through the binding's Event, 5 warm-ups
and the median of 20 calls per leg, the legs interleaved twice (a b c d a b c d),
the whole repeated on a second allocation made while the first is still held, and
64 sampled frames of every leg checked against the referee (tests/l4ref.py; for d
tests/rssref.py over the oracle's port).  The set is 16M frames:
cgck_synth_imix_dual in 2048-byte slots at l3_off 18, read through the set's own
descriptors.  Its TCP header bytes are random, so th_off is uniform and the option
areas are noise: a worst case for the walk, not typical traffic.  Legs:
  a  cgck_l4_desc, seg + cls + hash + count        l4d_kernel<true, true>
  b  cgck_l4_desc, seg only                        l4d_kernel<true, false>
  c  cgck_l4_desc, cls + count                     l4d_kernel<false, true>
  d  cgck_rss_desc (hash only), same descriptors   rssf_kernel<true, false>: the yardstick

    python tools/l4_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table with a / d, b / d and c / d, each leg's spread
between the two allocations as its margin.  Bytes are counted from the shapes: the
128-byte line that holds the chunks a lane loads in the first round (six from the
IP header's granule for a, b and c, four for d: one line per frame in this
layout), plus descriptors and outputs; the second load round is not counted.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("con-gen_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import cgck  # noqa: E402
import l4ref  # noqa: E402
import mixedbatches as MB  # noqa: E402
import oracle  # noqa: E402
import rssref  # noqa: E402

SEED = 0xAB7
HBM_PEAK = 8.0e12
STRIDE, L3 = 2048, 18
LEGS = ("a_all", "b_seg_only", "c_cls_count", "d_rss_desc")
HF = cgck.RSS_TCP | cgck.RSS_UDP


def timed(eng, launch, warm=5, reps=20):
    a, b = cgck.Event(), cgck.Event()
    for _ in range(warm):
        launch()
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.record(a)
        launch()
        eng.record(b)
        eng.sync()
        ms.append(eng.elapsed_ms(a, b))
    return statistics.median(ms), min(ms), max(ms)


def sample(n):
    """64 frames spread over the set, restated from the oracle's stream bytes and the
    stamp: (indices, expected records, classes, hashes, the frames)."""
    P = oracle.port()
    # (n - 1) / 63 is a multiple of 5 at 16M frames: shift the grid so both families are drawn
    ks = np.unique(np.minimum(np.linspace(0, n - 1, 64).astype(np.int64) + np.arange(64) % 5, n - 1))
    seg, cls, hsh, frames = np.zeros(len(ks), l4ref.SEG_DTYPE), [], [], []
    for i, k in enumerate(ks):
        k = int(k)
        ln = P.imix_desc(k)[1]
        slot = P.stream_bytes(k * STRIDE, STRIDE, SEED)
        MB.stamp_dual(slot[L3:L3 + ln], ln, k)
        f = slot[L3:L3 + ln].copy()
        c, r, h = l4ref.one(f)
        seg[i] = tuple(r[x] for x in l4ref.FIELDS)
        cls.append(c)
        hsh.append(h)
        frames.append(f)
    return ks, seg, np.array(cls, np.uint8), np.array(hsh, np.uint32), frames


def fetch(eng, dev, ks, dtype):
    """Elements ks of a device array."""
    got = np.zeros(len(ks), dtype)
    for i, k in enumerate(ks):
        dev.download(got[i:i + 1], off=got.itemsize * int(k), stream=eng.stream)
    eng.sync()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    P = oracle.port()
    with open(os.path.join(ROOT, "tests", "golden", "rss.json")) as f:
        key = np.frombuffer(bytes.fromhex(json.load(f)["freebsd_rss_key"]), np.uint8).copy()
    eng = cgck.Engine(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    ks, want_s, want_c, want_h, frames = sample(n)
    lens = np.array([len(f) for f in frames], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    want_r = rssref.expect(P, np.concatenate(frames), offs, lens, key, HF)[0]
    emit("sampled classes: " + json.dumps({l4ref.NAMES[c]: int(np.count_nonzero(want_c & 15 == c))
                                           for c in range(l4ref.NCLASS) if np.any(want_c & 15 == c)}))
    spec = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, 0)
    moved = {"a_all": (128 + 12 + 32 + 1 + 4) * n, "b_seg_only": (128 + 12 + 32) * n,
             "c_cls_count": (128 + 12 + 1) * n, "d_rss_desc": (128 + 12 + 4) * n}
    rows, held = [], []
    for alloc in (0, 1):
        buf = cgck.DeviceBuffer(n * STRIDE)
        desc, seg, cls, hsh, cnt, out = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(n),
                                         cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(4 * l4ref.NCOUNT),
                                         cgck.DeviceBuffer(4 * n))
        held += [buf, desc, seg, cls, hsh, cnt, out]       # the second allocation is made while the first is held
        eng.synth_imix_dual(buf.ptr, desc.ptr, n, SEED, STRIDE, L3)
        eng.sync()

        def leg_a():
            eng.l4_desc(buf.ptr, desc.ptr, n, seg=seg.ptr, cls=cls.ptr, hash=hsh.ptr, count=cnt.ptr)

        def leg_b():
            eng.l4_desc(buf.ptr, desc.ptr, n, seg=seg.ptr)

        def leg_c():
            eng.l4_desc(buf.ptr, desc.ptr, n, cls=cls.ptr, count=cnt.ptr)

        def leg_d():
            eng.rss_desc(buf.ptr, desc.ptr, n, spec, hash=out.ptr)

        for rnd in (0, 1):
            for leg, fn in zip(LEGS, (leg_a, leg_b, leg_c, leg_d)):
                for k in ks:                                # the sampled outputs are written anew by this leg
                    if leg in ("a_all", "b_seg_only"):
                        seg.upload(np.full(32, 0xEE, np.uint8), off=32 * int(k), stream=eng.stream)
                    if leg in ("a_all", "c_cls_count"):
                        cls.upload(np.full(1, 0xEE, np.uint8), off=int(k), stream=eng.stream)
                    if leg == "a_all":
                        hsh.upload(np.full(4, 0xEE, np.uint8), off=4 * int(k), stream=eng.stream)
                    if leg == "d_rss_desc":
                        out.upload(np.full(4, 0xEE, np.uint8), off=4 * int(k), stream=eng.stream)
                cnt.upload(np.zeros(l4ref.NCOUNT, np.uint32), stream=eng.stream)
                med, lo, hi = timed(eng, fn)
                kern = eng.last_kernel
                miss = 0
                if leg in ("a_all", "b_seg_only"):
                    miss += int(np.count_nonzero(fetch(eng, seg, ks, l4ref.SEG_DTYPE) != want_s))
                if leg in ("a_all", "c_cls_count"):
                    gn = np.zeros(l4ref.NCOUNT, np.uint32)
                    cnt.download(gn, stream=eng.stream)
                    eng.sync()
                    miss += int(np.count_nonzero(fetch(eng, cls, ks, np.uint8) != want_c))
                    # 25 calls (5 warm-ups, 20 timed); two frames in five are IPv6
                    miss += int(int(gn[:l4ref.NCLASS].sum()) != 25 * n)
                    miss += int(int(gn[11]) != 25 * sum((n - r + 4) // 5 for r in (0, 1)))
                if leg == "a_all":
                    miss += int(np.count_nonzero(fetch(eng, hsh, ks, np.uint32) != want_h))
                if leg == "d_rss_desc":
                    miss += int(np.count_nonzero(fetch(eng, out, ks, np.uint32) != want_r))
                r = {"alloc": alloc, "leg": leg, "round": rnd, "packets": n, "ms_median": round(med, 4),
                     "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes_counted": moved[leg],
                     "pct_hbm_peak": round(100 * moved[leg] / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                     "referee_mismatches": miss, "sampled": len(ks)}
                if leg == "a_all":
                    r["classes_per_call"] = {l4ref.NAMES[c]: int(gn[c]) // 25 for c in range(l4ref.NCLASS)}
                rows.append(r)
                emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()

    def med_of(leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["leg"] == leg and alloc in (None, r["alloc"]))

    emit("")
    emit(f"{'leg':12} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  margin %   MB counted  % of 8 TB/s  kernel")
    for leg in LEGS:
        sel = [r for r in rows if r["leg"] == leg]
        med, m0, m1 = med_of(leg), med_of(leg, 0), med_of(leg, 1)
        emit(f"{leg:12} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
             + f"  {med:7.4f}  {100 * abs(m0 - m1) / min(m0, m1):8.2f}  {moved[leg] / 1e6:10.1f}"
             + f"  {100 * moved[leg] / (med * 1e-3) / HBM_PEAK:11.1f}  {sel[0]['kernel']}")
    a, b, c, d = (med_of(leg) for leg in LEGS)
    emit(f"a / d = {a / d:.3f}, b / d = {b / d:.3f}, c / d = {c / d:.3f}; each leg's margin is its spread between the "
         f"two allocations")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    emit("not measured: bursts of a few hundred frames (launch-bound), typical traffic (option areas of real segments), "
         "the host route (header lines to the host, a parse there)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
