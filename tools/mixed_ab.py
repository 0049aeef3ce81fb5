#!/usr/bin/env python3
"""One CGCK_MIXED call against the two calls a caller makes without the flag,
in one process and on the same bytes.

The method is tools/ipv6_ab.py --imix's: HIP events through the binding's
Event, 5 warm-ups and the median of 20 launches per leg, the legs interleaved
twice (a b c d a b c d), the whole repeated on a second allocation made while
the first is still held, and 64 sampled packets of every leg checked against
the referee (tests/mixedref.py, tests/ip6ref.py and the oracle's port).  The
set is cgck_synth_imix_dual's: 16M IMIX frames, two in five IPv6, TCP / UDP /
ICMP by k % 7, packed and again in 2048 B ring slots at +14, at the 354 B
descriptor length hint.  Legs:
  a  GEN_BOTH | MIXED, one call                               lpwx_kernel
  b  the yardstick: GEN_BOTH over the IPv4 descriptors (lpw_kernel) and
     GEN_BOTH | IP6 over the IPv6 ones (lpw6_kernel), the same buffer, the two
     launches between one pair of events.  The split descriptor arrays are built
     once, on the host, outside the timed region.  The ICMP frames ride in the
     IPv4 call under the wrong L4 rule (the pseudo-header): a third call for them
     would only flatter a.
  c  VERIFY_TOY | MIXED with a verdict array and `bad` counters  lpwx_kernel
  d  GEN_BOTH over every descriptor, the bytes read as all-IPv4  lpw_kernel
     (what lpwx's second finish costs; the IPv6 frames' results mean nothing)

    python tools/mixed_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table with a / b, c / b and a / d and the
margin: b's own spread between the two allocations.
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
import ip6ref  # noqa: E402
import mixedbatches as MB  # noqa: E402
import mixedref as MR  # noqa: E402
import oracle  # noqa: E402

SEED = 0xAB7
HBM_PEAK = 8.0e12
IMIX_BYTES = 7 * 64 + 4 * 576 + 1500
CYCLE = (64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576)
LEGS = ("a_mixed", "b_two_calls", "c_mixed_verify", "d_all_ip4")


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
    """64 packets spread over the set, restated from the oracle's stream bytes:
    (indices, buf, offs, lens) with the packets laid back to back in buf."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    P = oracle.port()
    eng = cgck.Engine(0)
    eng.set_desc_len_hint(IMIX_BYTES // 12)      # 354
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    GEN, TOY = cgck.GEN_BOTH, cgck.VERIFY_TOY
    six = np.arange(n) % 5 < 2
    i4, i6 = np.nonzero(~six)[0], np.nonzero(six)[0]
    n4, n6 = len(i4), len(i6)
    read = n // 12 * IMIX_BYTES + sum(CYCLE[:n % 12])
    layouts = (("packed", 0, 0), ("ring", 2048, 14))
    rows, held = [], []
    for alloc in (0, 1):
        for name, stride, l3 in layouts:
            buf = cgck.DeviceBuffer(n * stride if stride else cgck.load().cgck_imix_bytes(n))
            desc, out, ver, bad = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n),
                                   cgck.DeviceBuffer(8))
            d4, d6, out4 = cgck.DeviceBuffer(12 * n4), cgck.DeviceBuffer(12 * n6), cgck.DeviceBuffer(4 * n4)
            held += [buf, desc, out, ver, bad, d4, d6, out4]   # the second allocation is made while the first is held
            eng.synth_imix_dual(buf.ptr, desc.ptr, n, SEED, stride, l3)
            hd = np.zeros(n, cgck.DESC_DTYPE)
            desc.download(hd, stream=eng.stream)
            eng.sync()
            d4.upload(hd[i4], stream=eng.stream)          # the host-side sort by family, not timed
            d6.upload(hd[i6], stream=eng.stream)
            bad.upload(np.zeros(2, np.uint32), stream=eng.stream)
            eng.sync()
            ks, sbuf, soffs, slens = sample(n, stride, l3)
            sdesc = np.zeros(len(ks), cgck.DESC_DTYPE)
            sdesc["frame_off"], sdesc["ip_len"] = soffs, slens
            want_mixed = {f: MR.expect(P, sbuf, soffs, slens, f) for f in (GEN, TOY)}
            want_ip4 = P.batch_desc(sbuf.copy(), sdesc.view(np.uint8), len(ks), GEN)[0]
            want_ip6 = ip6ref.expect(P, sbuf, soffs, slens, GEN | cgck.IP6)[0]

            def leg_a():
                eng.desc(buf.ptr, desc.ptr, n, GEN | cgck.MIXED, out.ptr)

            def leg_b():
                eng.desc(buf.ptr, d4.ptr, n4, GEN, out4.ptr)
                k4 = eng.last_kernel
                eng.desc(buf.ptr, d6.ptr, n6, GEN | cgck.IP6, out.ptr)
                leg_b.kernels = k4 + " + " + eng.last_kernel

            def leg_c():
                eng.desc(buf.ptr, desc.ptr, n, TOY | cgck.MIXED, out.ptr, ver.ptr, bad.ptr)

            def leg_d():
                eng.desc(buf.ptr, desc.ptr, n, GEN, out.ptr)

            for rnd in (0, 1):
                for leg, fn in zip(LEGS, (leg_a, leg_b, leg_c, leg_d)):
                    med, lo, hi = timed(eng, fn)
                    kern = leg_b.kernels if leg == "b_two_calls" else eng.last_kernel
                    got, gv = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
                    out.download(got, stream=eng.stream)
                    ver.download(gv, stream=eng.stream)
                    eng.sync()
                    if leg == "a_mixed":
                        miss = int(np.count_nonzero(got[ks] != want_mixed[GEN][0]))
                    elif leg == "c_mixed_verify":
                        miss = int(np.count_nonzero((got[ks] != want_mixed[TOY][0]) | (gv[ks] != want_mixed[TOY][1])))
                    elif leg == "d_all_ip4":
                        miss = int(np.count_nonzero(got[ks] != want_ip4))
                    else:       # b: the IPv6 results in out, the IPv4 ones in out4, each by rank in its family
                        g4 = np.zeros(n4, np.uint32)
                        out4.download(g4, stream=eng.stream)
                        eng.sync()
                        s6 = six[ks]
                        miss = int(np.count_nonzero(got[np.searchsorted(i6, ks[s6])] != want_ip6[s6]) +
                                   np.count_nonzero(g4[np.searchsorted(i4, ks[~s6])] != want_ip4[~s6]))
                    r = {"alloc": alloc, "layout": name, "leg": leg, "round": rnd, "packets": n,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "pct_hbm_peak": round(100 * read / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
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
    emit(f"{'layout':7} {'leg':15} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1)) + "   median  % peak  kernel")
    for name, _, _ in layouts:
        for leg in LEGS:
            sel = [r for r in rows if r["layout"] == name and r["leg"] == leg]
            med = med_of(name, leg)
            emit(f"{name:7} {leg:15} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {100 * read / (med * 1e-3) / HBM_PEAK:5.1f}  {sel[0]['kernel']}")
        a, b, c, d = (med_of(name, leg) for leg in LEGS)
        b0, b1 = med_of(name, "b_two_calls", 0), med_of(name, "b_two_calls", 1)
        emit(f"{name:7} a / b = {a / b:.3f}, c / b = {c / b:.3f}, a / d = {a / d:.3f}; margin (b's spread between the "
             f"two allocations) {100 * abs(b0 - b1) / min(b0, b1):.2f} %")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
