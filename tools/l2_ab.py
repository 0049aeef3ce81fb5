#!/usr/bin/env python3
"""cgck_l2_desc (l2d_kernel) beside the per-frame hash that follows it on the same
burst, in one process.

The method is tools/rssf_ab.py's: HIP events through the binding's Event, 5
warm-ups and the median of 20 calls per leg, the legs interleaved twice
(a b c a b c), the whole repeated on a second allocation made while the first is
still held, and 64 sampled frames of every leg checked against the referee
(tests/l2ref.py; for c tests/rssref.py over the oracle's port).  The set is 16M
frames: cgck_synth_imix_dual in 2048-byte slots at l3_off 18, then cgck_synth_eth
with vlan_every 8 (every eighth frame tagged; no frame of this set is short
enough to be padded).  Legs:
  a  cgck_l2_desc, desc_out + cls + count          l2d_kernel<true, true>
  b  cgck_l2_desc, desc_out only                   l2d_kernel<true, false>
  c  cgck_rss_desc (hash only) over a's desc_out   rssf_kernel<true, false>: the yardstick

    python tools/l2_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table with a / c and b / c, each leg's spread
between the two allocations as its margin.  Bytes are counted from the shapes: the
128-byte lines that hold a byte of the chunks a lane loads (three from the
Ethernet header's granule for a and b, four from the IP header's for c: one line
per frame in this layout), plus descriptors and outputs.  The host route (the
frames' first bytes down, a loop, the descriptors up) is not timed here.
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
import l2batches as LB  # noqa: E402
import l2ref  # noqa: E402
import mixedbatches as MB  # noqa: E402
import oracle  # noqa: E402
import rssref  # noqa: E402

SEED, ESEED = 0xAB7, 0xE7
HBM_PEAK = 8.0e12
STRIDE, L3, VLAN_EVERY = 2048, 18, 8
LEGS = ("a_desc_cls_count", "b_desc_only", "c_rss_desc")
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
    """64 frames spread over the set, restated from the oracle's stream bytes and
    the two stamps: (indices, expected desc_out rows, expected cls, slots)."""
    P = oracle.port()
    ks = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))
    want_d, want_c, slots = [], [], []
    for k in ks:
        k = int(k)
        ln = P.imix_desc(k)[1]
        slot = P.stream_bytes(k * STRIDE, STRIDE, SEED)
        MB.stamp_dual(slot[L3:L3 + ln], ln, k)
        _, e_off, L = LB.synth_eth_one(slot, k, 0, L3, ln, VLAN_EVERY, ESEED)
        c, flags, off, ip_len = l2ref.one(slot[e_off:e_off + L], L, e_off)
        want_d.append((k * STRIDE, e_off if c == l2ref.RUNT else e_off + off, ip_len))
        want_c.append(c | flags)
        slots.append(slot)
    return ks, np.array(want_d, l2ref.DESC_DTYPE), np.array(want_c, np.uint8), slots


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

    ks, want_d, want_c, slots = sample(n)
    assert np.all(want_c & 15 <= l2ref.IP6) and np.array_equal(want_d["l3_off"], np.full(len(ks), L3))
    soffs = np.arange(len(ks), dtype=np.int64) * STRIDE + L3
    want_h = rssref.expect(P, np.concatenate(slots), soffs, want_d["ip_len"].astype(np.int64), key, HF)[0]
    spec = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, 0)
    moved = {"a_desc_cls_count": (128 + 12 + 12 + 1) * n, "b_desc_only": (128 + 12 + 12) * n,
             "c_rss_desc": (128 + 12 + 4) * n}
    rows, held = [], []
    for alloc in (0, 1):
        buf = cgck.DeviceBuffer(n * STRIDE)
        desc, raw, dout, cls, cnt, out = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(12 * n),
                                          cgck.DeviceBuffer(n), cgck.DeviceBuffer(4 * l2ref.NCOUNT),
                                          cgck.DeviceBuffer(4 * n))
        held += [buf, desc, raw, dout, cls, cnt, out]      # the second allocation is made while the first is held
        eng.synth_imix_dual(buf.ptr, desc.ptr, n, SEED, STRIDE, L3)
        eng.synth_eth(buf.ptr, desc.ptr, raw.ptr, n, VLAN_EVERY, ESEED)
        eng.sync()

        def leg_a():
            eng.l2_desc(buf.ptr, raw.ptr, n, desc_out=dout.ptr, cls=cls.ptr, count=cnt.ptr)

        def leg_b():
            eng.l2_desc(buf.ptr, raw.ptr, n, desc_out=dout.ptr)

        def leg_c():
            eng.rss_desc(buf.ptr, dout.ptr, n, spec, hash=out.ptr)

        for rnd in (0, 1):
            for leg, fn in zip(LEGS, (leg_a, leg_b, leg_c)):
                if leg != "c_rss_desc":                    # the sampled descriptors are written anew by this leg
                    for k in ks:
                        dout.upload(np.zeros(12, np.uint8), off=12 * int(k), stream=eng.stream)
                if leg == "a_desc_cls_count":
                    cnt.upload(np.zeros(l2ref.NCOUNT, np.uint32), stream=eng.stream)
                med, lo, hi = timed(eng, fn)
                kern = eng.last_kernel
                if leg == "c_rss_desc":
                    miss = int(np.count_nonzero(fetch(eng, out, ks, np.uint32) != want_h))
                else:
                    miss = int(np.count_nonzero(fetch(eng, dout, ks, l2ref.DESC_DTYPE) != want_d))
                    if leg == "a_desc_cls_count":
                        gn = np.zeros(l2ref.NCOUNT, np.uint32)
                        cnt.download(gn, stream=eng.stream)
                        eng.sync()
                        miss += int(np.count_nonzero(fetch(eng, cls, ks, np.uint8) != want_c))
                        # 25 calls (5 warm-ups, 20 timed) over frames that are all IPv4 or IPv6
                        miss += int(int(gn[:2].sum()) != 25 * n or int(gn[11]) != 25 * ((n + VLAN_EVERY - 1) // VLAN_EVERY))
                r = {"alloc": alloc, "leg": leg, "round": rnd, "packets": n, "ms_median": round(med, 4),
                     "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes_counted": moved[leg],
                     "pct_hbm_peak": round(100 * moved[leg] / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                     "referee_mismatches": miss, "sampled": len(ks)}
                rows.append(r)
                emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()

    def med_of(leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["leg"] == leg and alloc in (None, r["alloc"]))

    emit("")
    emit(f"{'leg':18} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  margin %   MB counted  % of 8 TB/s  kernel")
    for leg in LEGS:
        sel = [r for r in rows if r["leg"] == leg]
        med, m0, m1 = med_of(leg), med_of(leg, 0), med_of(leg, 1)
        emit(f"{leg:18} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
             + f"  {med:7.4f}  {100 * abs(m0 - m1) / min(m0, m1):8.2f}  {moved[leg] / 1e6:10.1f}"
             + f"  {100 * moved[leg] / (med * 1e-3) / HBM_PEAK:11.1f}  {sel[0]['kernel']}")
    a, b, c = (med_of(leg) for leg in LEGS)
    emit(f"a / c = {a / c:.3f}, b / c = {b / c:.3f}, a / b = {a / b:.3f}; each leg's margin is its spread between the "
         f"two allocations")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    emit("not measured: the host route (frame heads to the host, a loop there, descriptors back up)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
