#!/usr/bin/env python3
"""The per-frame RSS hash (cgck_rss_desc, rssf_kernel) beside the pass that
reads every byte of the same burst and beside the hash alone, in one process
(DESIGN.md section 5.9).

The method is tools/mixed_ab.py's: HIP events through the binding's Event, 5
warm-ups and the median of 20 launches per leg, the legs interleaved twice
(a b c d a b c d), the whole repeated on a second allocation made while the first
is still held, and 64 sampled frames of every leg checked against the referee
(tests/rssref.py, tests/mixedref.py and the oracle's port).  The set is
cgck_synth_imix_dual's: 16M IMIX frames, two in five IPv6, TCP / UDP / ICMP by
k % 7, packed and again in 2048 B ring slots at +14.  Its IPv4 frames carry
random flags / fragment-offset bytes, so nearly all of them count as fragments
and hash their 8 address bytes; its IPv6 frames have no extension header and
hash 36 bytes (TCP, UDP) or 32 (ICMPv6).  No frame of it needs the kernel's second
load round.  Legs:
  a  cgck_rss_desc, hash only                                        rssf_kernel<true, false>
  b  cgck_rss_desc, hash + kind + queue + qcount at queue_num 8      rssf_kernel<true, true>
  c  GEN_BOTH | CGCK_MIXED over the same descriptors: every byte read  lpwx_kernel
  d  cgck_toeplitz over 16M pre-cut 12-byte tuples: the hash with no gather

    python tools/rssf_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table with a / c and a / d and the margin: c's own
spread between the two allocations.  Bytes are counted from the shapes: for a
and b the distinct 128-byte lines that hold a byte of the four 16-byte chunks a
lane loads (its frame's first granules), plus descriptors and outputs; for c
every frame byte; for d 12 + 4 bytes a tuple.
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
import mixedbatches as MB  # noqa: E402
import mixedref as MR  # noqa: E402
import oracle  # noqa: E402
import rssref  # noqa: E402

SEED = 0xAB7
HBM_PEAK = 8.0e12
IMIX_BYTES = 7 * 64 + 4 * 576 + 1500
CYCLE = (64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576)
LEGS = ("a_hash", "b_hash_kind_queue", "c_mixed_cksum", "d_toeplitz12")
HF = cgck.RSS_TCP | cgck.RSS_UDP
QN = 8


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


def sample(n, stride, l3):
    """tools/mixed_ab.py's: 64 frames spread over the set, restated from the
    oracle's stream bytes, laid back to back: (indices, buf, offs, lens)."""
    P = oracle.port()
    ks = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))
    frames = []
    for k in ks:
        off, ln = P.imix_desc(int(k))
        if stride:
            off = int(k) * stride + l3
        p = P.stream_bytes(off, ln, SEED)
        MB.stamp_dual(p, ln, int(k))
        frames.append(p)
    lens = np.array([len(f) for f in frames], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    return ks, np.concatenate(frames), offs, lens


def lines_touched(n, stride, l3):
    """Distinct 128-byte lines holding a byte of the chunks rssf_kernel's first
    round loads, over n frames (counted over one period of the layout and scaled)."""
    if stride:
        per = len({(l3 // 16 * 16 + 16 * i) // 128 for i in range(4)})     # every slot alike
        return n * per
    period = 12 * 32                       # 32 cycles of 4252 bytes = 1063 lines
    seen, off = set(), 0
    for k in range(period):
        ln = CYCLE[k % 12]
        a, nch = off // 16 * 16, (off % 16 + ln + 15) // 16
        seen |= {(a + 16 * min(i, nch - 1)) // 128 for i in range(4)}
        off += ln
    return n * len(seen) // period


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
    eng.set_desc_len_hint(IMIX_BYTES // 12)      # 354
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    frame_bytes = n // 12 * IMIX_BYTES + sum(CYCLE[:n % 12])
    layouts = (("packed", 0, 0), ("ring", 2048, 14))
    spec_a = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, 0)
    spec_b = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, QN)
    tup = np.random.default_rng(SEED).integers(0, 256, 12 * n, dtype=np.uint8)
    tks = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))
    want_t = np.array([P.toeplitz_hash(tup[12 * k:12 * k + 12], key) for k in tks], np.uint32)
    rows, held = [], []
    for alloc in (0, 1):
        for name, stride, l3 in layouts:
            buf = cgck.DeviceBuffer(n * stride if stride else cgck.load().cgck_imix_bytes(n))
            desc, out, kind, queue, qc = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n),
                                          cgck.DeviceBuffer(n), cgck.DeviceBuffer(4 * 128))
            dt = cgck.DeviceBuffer(12 * n)
            held += [buf, desc, out, kind, queue, qc, dt]   # the second allocation is made while the first is held
            eng.synth_imix_dual(buf.ptr, desc.ptr, n, SEED, stride, l3)
            dt.upload(tup, stream=eng.stream)
            qc.upload(np.zeros(128, np.uint32), stream=eng.stream)
            eng.sync()
            ks, sbuf, soffs, slens = sample(n, stride, l3)
            want_h, want_k, want_q = rssref.expect(P, sbuf, soffs, slens, key, HF, queue_num=QN)
            want_c = MR.expect(P, sbuf, soffs, slens, cgck.GEN_BOTH)[0]
            nb_lines = 128 * lines_touched(n, stride, l3)
            moved = {"a_hash": nb_lines + 16 * n, "b_hash_kind_queue": nb_lines + 18 * n,
                     "c_mixed_cksum": frame_bytes + 16 * n, "d_toeplitz12": 16 * n}

            def leg_a():
                eng.rss_desc(buf.ptr, desc.ptr, n, spec_a, hash=out.ptr)

            def leg_b():
                eng.rss_desc(buf.ptr, desc.ptr, n, spec_b, hash=out.ptr, kind=kind.ptr, queue=queue.ptr, qcount=qc.ptr)

            def leg_c():
                eng.desc(buf.ptr, desc.ptr, n, cgck.GEN_BOTH | cgck.MIXED, out.ptr)

            def leg_d():
                eng.toeplitz(dt.ptr, n, 12, 12, key, out.ptr)

            for rnd in (0, 1):
                for leg, fn in zip(LEGS, (leg_a, leg_b, leg_c, leg_d)):
                    med, lo, hi = timed(eng, fn)
                    kern = eng.last_kernel
                    got = np.zeros(n, np.uint32)
                    out.download(got, stream=eng.stream)
                    eng.sync()
                    if leg == "a_hash":
                        miss = int(np.count_nonzero(got[ks] != want_h))
                    elif leg == "b_hash_kind_queue":
                        gk, gq = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
                        kind.download(gk, stream=eng.stream)
                        queue.download(gq, stream=eng.stream)
                        eng.sync()
                        miss = int(np.count_nonzero((got[ks] != want_h) | (gk[ks] != want_k) | (gq[ks] != want_q)))
                    elif leg == "c_mixed_cksum":
                        miss = int(np.count_nonzero(got[ks] != want_c))
                    else:
                        miss = int(np.count_nonzero(got[tks] != want_t))
                    r = {"alloc": alloc, "layout": name, "leg": leg, "round": rnd, "packets": n,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "bytes_counted": moved[leg],
                         "pct_hbm_peak": round(100 * moved[leg] / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                         "referee_mismatches": miss, "sampled": len(ks)}
                    rows.append(r)
                    emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()

    def med_of(name, leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["layout"] == name and r["leg"] == leg
                                 and alloc in (None, r["alloc"]))

    emit("")
    emit(f"{'layout':7} {'leg':18} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median   MB counted  % of 8 TB/s  kernel")
    for name, _, _ in layouts:
        for leg in LEGS:
            sel = [r for r in rows if r["layout"] == name and r["leg"] == leg]
            med = med_of(name, leg)
            emit(f"{name:7} {leg:18} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {sel[0]['bytes_counted'] / 1e6:10.1f}  {100 * sel[0]['bytes_counted'] / (med * 1e-3) / HBM_PEAK:11.1f}"
                 + f"  {sel[0]['kernel']}")
        a, b, c, d = (med_of(name, leg) for leg in LEGS)
        c0, c1 = med_of(name, "c_mixed_cksum", 0), med_of(name, "c_mixed_cksum", 1)
        emit(f"{name:7} a / c = {a / c:.3f}, b / a = {b / a:.3f}, a / d = {a / d:.3f}; margin (c's spread between the "
             f"two allocations) {100 * abs(c0 - c1) / min(c0, c1):.2f} %")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
