#!/usr/bin/env python3
"""The partition by queue id (cgck_steer, cgck_steer.hip) beside the host pass it
replaces and beside the hash that feeds it, in one process.

The method is tools/rssf_ab.py's: HIP events through the binding's Event, 5
warm-ups and the median of 20 calls per leg, the legs interleaved twice
(a b c d a b c d), the whole repeated on a second allocation made while the first
is still held, and 64 sampled slots of every leg checked against the referee
(tests/steerref.py over the queue ids the device wrote, which tools/rssf_ab.py
checks against tests/rssref.py).  The set is cgck_synth_imix_dual's 16M packed
IMIX frames after one cgck_rss_desc, with 8 queues and again with 128.  Legs:
  a  cgck_steer, qoff + perm + slot + desc_out       count, scan, steer_scatter_kernel<true, true, true>
  b  cgck_steer, perm only                           count, scan, steer_scatter_kernel<true, false, false>
  c  the route without cgck_steer: queue[] copied to the host, a stable bucket
     there (numpy: argsort(kind="stable") of the uint8 bins, a radix sort, then a
     fancy-index gather of the descriptors the host already holds), the gathered
     descriptors uploaded; timed end to end, copies included
  d  cgck_rss_desc, hash + kind + queue + qcount (tools/rssf_ab.py's leg b), for scale

    python tools/steer_ab.py [--packets N] [--out FILE]
    python tools/steer_ab.py --launches [--out FILE]

One JSON line per leg, then a table with a / c and the margin: d's own spread
between the two allocations.  Bytes are counted from the shapes: a reads n x (2 x
1 + 12) (queue[] twice, the descriptors) and writes n x (4 + 4 + 12), plus the
workspace written, scanned and read (4 x 4 bytes a word); b reads 2 n and writes
4 n.

--launches times the one-launch kernel against the three launches at n = 256 and
n = the tile, all four outputs, 8 queues.  It needs the lab build (make -C tools
lab), whose CGCK_STEER_THREE knob sends a one-tile call that brings a workspace
through count, scan and scatter: the same process runs both, with and without
`work`.  Each figure is the median of 20 single calls between two events, and of
20 trains of 50 calls divided by 50.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--launches" in sys.argv:        # before the binding reads them
    os.environ["CGCK_LIB"] = os.path.join(ROOT, "con-gen_amd", "libcgck_lab.so")
    os.environ["CGCK_STEER_THREE"] = "1"
for d in ("con-gen_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import cgck  # noqa: E402
import steerref  # noqa: E402

SEED = 0xAB7
HBM_PEAK = 8.0e12
LEGS = ("a_steer_all", "b_steer_perm", "c_host_bucket", "d_rss_desc")
HF = cgck.RSS_TCP | cgck.RSS_UDP


def timed(eng, launch, warm=5, reps=20, train=1):
    a, b = cgck.Event(), cgck.Event()
    for _ in range(warm):
        launch()
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.record(a)
        for _ in range(train):
            launch()
        eng.record(b)
        eng.sync()
        ms.append(eng.elapsed_ms(a, b) / train)
    return statistics.median(ms), min(ms), max(ms)


def fetch(eng, buf, n, dtype):
    out = np.zeros(n, dtype)
    buf.download(out, stream=eng.stream)
    eng.sync()
    return out


def bursts(eng, emit):
    """steer_one_kernel against count + scan + scatter on one-tile bursts."""
    qn = 8
    T = cgck.steer_plan(1, qn)[0]
    rng = np.random.default_rng(SEED)
    rows = []
    for n in (256, T):
        queue = rng.choice(np.concatenate((np.arange(qn), [0xFF])).astype(np.uint8), n)
        desc = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint32)
        want = steerref.expect(queue, qn, desc)
        dq, di = cgck.DeviceBuffer(n), cgck.DeviceBuffer(12 * n)
        qoff, perm, slot, dout = (cgck.DeviceBuffer(4 * (qn + 2)), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(4 * n),
                                  cgck.DeviceBuffer(12 * n))
        work = cgck.DeviceBuffer(4 * (qn + 1))
        dq.upload(queue, stream=eng.stream)
        di.upload(desc, stream=eng.stream)
        eng.sync()
        for rnd in (0, 1):
            for leg, w in (("one_launch", None), ("three_launches", work.ptr)):
                def call():
                    eng.steer(dq.ptr, n, qn, di.ptr, qoff.ptr, perm.ptr, slot.ptr, dout.ptr, work=w)
                for x in (qoff, perm, slot, dout):
                    cgck.load().cgck_memset(x.ptr, 0xEE, x.nbytes, eng.stream)
                single = timed(eng, call)
                train = timed(eng, call, train=50)
                kern = eng.last_kernel
                got = (fetch(eng, qoff, qn + 2, np.uint32), fetch(eng, perm, n, np.uint32),
                       fetch(eng, slot, n, np.uint32), fetch(eng, dout, 3 * n, np.uint32).reshape(n, 3))
                miss = sum(int(np.count_nonzero(g != w_)) for g, w_ in zip(got, want))
                r = {"n": n, "queue_num": qn, "leg": leg, "round": rnd, "us_single_median": round(1e3 * single[0], 2),
                     "us_single_min": round(1e3 * single[1], 2), "us_train50_median": round(1e3 * train[0], 2),
                     "us_train50_min": round(1e3 * train[1], 2), "kernel": kern, "referee_mismatches": miss}
                rows.append(r)
                emit(json.dumps(r))
        for x in (dq, di, qoff, perm, slot, dout, work):
            x.free()
    emit("")
    for n in (256, T):
        def med(leg, k):
            return statistics.median(r[k] for r in rows if r["n"] == n and r["leg"] == leg)
        emit(f"n {n:5}: one launch {med('one_launch', 'us_single_median'):7.2f} us single, "
             f"{med('one_launch', 'us_train50_median'):7.2f} us in a train; three launches "
             f"{med('three_launches', 'us_single_median'):7.2f} us single, "
             f"{med('three_launches', 'us_train50_median'):7.2f} us in a train")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--launches", action="store_true", help="one launch against three on one-tile bursts (lab build)")
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    with open(os.path.join(ROOT, "tests", "golden", "rss.json")) as f:
        key = np.frombuffer(bytes.fromhex(json.load(f)["freebsd_rss_key"]), np.uint8).copy()
    eng = cgck.Engine(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        eng.close()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.launches:
        bursts(eng, emit)
        return finish()

    emit(f"numpy {np.__version__} does leg c's bucketing: argsort(kind='stable') of uint8 bins, then desc[perm]")
    ss = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))       # the sampled slots
    rows, held = [], []
    for alloc in (0, 1):
        buf = cgck.DeviceBuffer(cgck.load().cgck_imix_bytes(n))
        desc, out, kind, queue, qc = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n),
                                      cgck.DeviceBuffer(n), cgck.DeviceBuffer(4 * 128))
        perm, slot, dout, qoff = (cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(12 * n),
                                  cgck.DeviceBuffer(4 * 130))
        held += [buf, desc, out, kind, queue, qc, perm, slot, dout, qoff]   # the second allocation is made while the first is held
        eng.synth_imix_dual(buf.ptr, desc.ptr, n, SEED)
        qc.upload(np.zeros(128, np.uint32), stream=eng.stream)
        hdesc = fetch(eng, desc, 3 * n, np.uint32).reshape(n, 3)
        for qn in (8, 128):
            spec = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, qn)
            eng.rss_desc(buf.ptr, desc.ptr, n, spec, hash=out.ptr, kind=kind.ptr, queue=queue.ptr, qcount=qc.ptr)
            hq = fetch(eng, queue, n, np.uint8)
            want = steerref.expect(hq, qn, hdesc)
            T, tiles, wb = cgck.steer_plan(n, qn)
            work = cgck.DeviceBuffer(max(wb, 4))
            held.append(work)
            hist = 4 * tiles * (qn + 1)
            moved = {"a_steer_all": n * (2 + 12) + n * (4 + 4 + 12) + 4 * hist, "b_steer_perm": 2 * n + 4 * n + 4 * hist,
                     "c_host_bucket": n + 12 * n, "d_rss_desc": 0}
            hq2 = np.zeros(n, np.uint8)

            def leg_a():
                eng.steer(queue.ptr, n, qn, desc.ptr, qoff.ptr, perm.ptr, slot.ptr, dout.ptr, work=work.ptr)

            def leg_b():
                eng.steer(queue.ptr, n, qn, perm=perm.ptr, work=work.ptr)

            def leg_c():
                queue.download(hq2, stream=eng.stream)
                eng.sync()
                order = np.argsort(np.minimum(hq2, qn).astype(np.uint8), kind="stable")
                dout.upload(hdesc[order], stream=eng.stream)

            def leg_d():
                eng.rss_desc(buf.ptr, desc.ptr, n, spec, hash=out.ptr, kind=kind.ptr, queue=queue.ptr, qcount=qc.ptr)

            for rnd in (0, 1):
                for leg, fn in zip(LEGS, (leg_a, leg_b, leg_c, leg_d)):
                    for x in (perm, slot, dout, qoff):
                        cgck.load().cgck_memset(x.ptr, 0xEE, x.nbytes, eng.stream)
                    med, lo, hi = timed(eng, fn)
                    kern = eng.last_kernel if leg != "c_host_bucket" else "(host)"
                    miss = 0
                    if leg in ("a_steer_all", "b_steer_perm"):
                        miss += int(np.count_nonzero(fetch(eng, perm, n, np.uint32)[ss] != want[1][ss]))
                    if leg in ("a_steer_all", "c_host_bucket"):
                        miss += int(np.count_nonzero(fetch(eng, dout, 3 * n, np.uint32).reshape(n, 3)[ss] != want[3][ss]))
                    if leg == "a_steer_all":
                        miss += int(np.count_nonzero(fetch(eng, slot, n, np.uint32)[ss] != want[2][ss]))
                        miss += int(np.count_nonzero(fetch(eng, qoff, qn + 2, np.uint32) != want[0]))
                    if leg == "d_rss_desc":
                        miss += int(np.count_nonzero(fetch(eng, queue, n, np.uint8) != hq))
                    r = {"alloc": alloc, "queue_num": qn, "leg": leg, "round": rnd, "packets": n, "tile": T, "tiles": tiles,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "bytes_counted": moved[leg],
                         "pct_hbm_peak": round(100 * moved[leg] / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                         "referee_mismatches": miss, "sampled": len(ss)}
                    rows.append(r)
                    emit(json.dumps(r))
    for b in held:
        b.free()

    def med_of(qn, leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["queue_num"] == qn and r["leg"] == leg
                                 and alloc in (None, r["alloc"]))

    emit("")
    emit(f"{'queues':6} {'leg':14} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "    median   MB counted  % of 8 TB/s  kernel")
    for qn in (8, 128):
        for leg in LEGS:
            sel = [r for r in rows if r["queue_num"] == qn and r["leg"] == leg]
            med = med_of(qn, leg)
            emit(f"{qn:6} {leg:14} " + " ".join(f"{r['ms_median']:8.3f}" for r in sel)
                 + f"  {med:8.3f}  {sel[0]['bytes_counted'] / 1e6:10.1f}  {100 * sel[0]['bytes_counted'] / (med * 1e-3) / HBM_PEAK:11.1f}"
                 + f"  {sel[0]['kernel']}")
        a, b, c, d = (med_of(qn, leg) for leg in LEGS)
        d0, d1 = med_of(qn, "d_rss_desc", 0), med_of(qn, "d_rss_desc", 1)
        emit(f"{qn:6} c / a = {c / a:.1f}, a / b = {a / b:.2f}, a / d = {a / d:.2f}; margin (d's spread between the two "
             f"allocations) {100 * abs(d0 - d1) / min(d0, d1):.2f} %")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    finish()


if __name__ == "__main__":
    main()
