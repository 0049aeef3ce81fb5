#!/usr/bin/env python3
"""IPv4 against IPv6 (CGCK_IP6) on the same kernel family, in one process and
on the same allocation.

Per allocation and shape: the buffer is filled and stamped as IPv4
(cgck_synth_strided) and CGCK_GEN_BOTH is timed, then the same buffer is
stamped as IPv6 (cgck_synth_strided_ip6, the same byte stream) and
CGCK_GEN_BOTH | CGCK_IP6 is timed; both legs twice (A B A B), each 5 warm-ups
and the median of 20 launches, timed with HIP events through the binding's
Event.  The whole is repeated on a second, fresh allocation made while the
first is still held.  Shapes: 16M x 1500 B (dstr / dstr6) and 16M x 64 B
stride (lpd / lpd6; IPv4 ip_len 64, IPv6 ip_len 60, and IPv6 ip_len 64 as the
same-bytes row).  64 sampled packets of every IPv6 leg are checked against
the oracle (in_cksum over pseudo-header || segment).

    python tools/ipv6_ab.py [--packets N] [--out FILE]

--imix: the mixed-length legs instead, built the same way (one process, the
same allocation restamped, A B A B, two allocations, 64 sampled packets of every
IPv6 leg against the oracle), on the 16M-packet IMIX set packed and again in
2048 B ring slots at +14, all at the 354 B descriptor length hint:
  a  IPv4 GEN_BOTH, auto                      lpw_kernel
  b  IPv6 GEN_BOTH | IP6, auto                lpw6_kernel
  c  as b, pinned "group"                     cksum6_kernel (the path before lpw6)
  d  IPv6 VERIFY_TOY | IP6, verdict array     lpw6_kernel

One JSON line per leg, then a table.
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

SEED = 0xAB6
HBM_PEAK = 8.0e12   # bytes/s, the figure the project's other tables use


def time_leg(eng, buf, out, n, stride, ip_len, flags, warm=5, reps=20):
    a, b = cgck.Event(), cgck.Event()
    for _ in range(warm):
        eng.strided(buf.ptr, n, stride, 0, ip_len, flags, out.ptr)
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.record(a)
        eng.strided(buf.ptr, n, stride, 0, ip_len, flags, out.ptr)
        eng.record(b)
        eng.sync()
        ms.append(eng.elapsed_ms(a, b))
    return statistics.median(ms), min(ms), max(ms), eng.last_kernel


def check_ip6(eng, out, n, stride, ip_len, nh):
    """64 packets spread over the batch against the oracle."""
    P = oracle.port()
    got = np.zeros(n, np.uint32)
    out.download(got, stream=eng.stream)
    eng.sync()
    bad = 0
    for k in np.linspace(0, n - 1, 64).astype(np.int64):
        p = P.stream_bytes(int(k) * stride, ip_len, SEED)
        p[0:4] = (0x60, 0, 0, 0)
        p[4], p[5], p[6] = (ip_len - 40) >> 8, (ip_len - 40) & 255, nh
        fo = {6: 16, 17: 6, 58: 2}.get(nh)
        if fo is not None and 40 + fo + 2 <= ip_len:
            p[40 + fo:40 + fo + 2] = 0
        m = ip_len - 40
        ph = np.array([m >> 24, (m >> 16) & 255, (m >> 8) & 255, m & 255, 0, 0, 0, nh], np.uint8)
        z = np.ascontiguousarray(np.concatenate((p[8:40], ph, p[40:])))
        bad += int(got[k]) != P.in_cksum(z, 0, len(z)) << 16
    return bad


IMIX_BYTES = 7 * 64 + 4 * 576 + 1500     # one 12-frame cycle


def time_desc(eng, buf, desc, out, ver, n, flags, warm=5, reps=20):
    a, b = cgck.Event(), cgck.Event()
    for _ in range(warm):
        eng.desc(buf.ptr, desc.ptr, n, flags, out.ptr, ver.ptr if ver else None)
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.record(a)
        eng.desc(buf.ptr, desc.ptr, n, flags, out.ptr, ver.ptr if ver else None)
        eng.record(b)
        eng.sync()
        ms.append(eng.elapsed_ms(a, b))
    return statistics.median(ms), min(ms), max(ms), eng.last_kernel


def check_imix6(eng, out, ver, n, stride, l3, nh, flags):
    """64 packets spread over the batch against the oracle (the generator's
    frames restated: stream bytes, the IMIX offsets, the IPv6 stamp)."""
    P = oracle.port()
    got, gv = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    out.download(got, stream=eng.stream)
    if ver:
        ver.download(gv, stream=eng.stream)
    eng.sync()
    bad = 0
    for k in np.linspace(0, n - 1, 64).astype(np.int64):
        off, ln = P.imix_desc(int(k))
        if stride:
            off = int(k) * stride + l3
        p = P.stream_bytes(off, ln, SEED)
        p[0:4] = (0x60, 0, 0, 0)
        p[4], p[5], p[6] = (ln - 40) >> 8, (ln - 40) & 255, nh
        fo = {6: 16, 17: 6, 58: 2}.get(nh)
        if fo is not None and 40 + fo + 2 <= ln:
            p[40 + fo:40 + fo + 2] = 0
        m = ln - 40
        ph = np.array([m >> 24, (m >> 16) & 255, (m >> 8) & 255, m & 255, 0, 0, 0, nh], np.uint8)
        z = np.ascontiguousarray(np.concatenate((p[8:40], ph, p[40:])))
        hi = P.in_cksum(z, 0, len(z))
        wantv = cgck.BAD_L4 if flags & cgck.VERIFY and fo is not None and hi != 0 else 0   # the stored field is 0
        bad += int(got[k]) != hi << 16 or (ver is not None and int(gv[k]) != wantv)
    return bad


def imix_main(args):
    n = args.packets
    eng = cgck.Engine(0)
    eng.set_desc_len_hint(IMIX_BYTES // 12)      # 354
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    G6, T6 = cgck.GEN_BOTH | cgck.IP6, cgck.VERIFY_TOY | cgck.IP6
    legs = (("a_ip4", cgck.GEN_BOTH, "auto", False), ("b_ip6", G6, "auto", False),
            ("c_ip6_group", G6, "group", False), ("d_ip6_verify", T6, "auto", True))
    if args.reverse:
        legs = legs[::-1]
        emit("legs in reverse order")
    layouts = (("packed", 0, 0), ("ring", 2048, 14))
    read = n // 12 * IMIX_BYTES + sum((64, 576, 64, 64, 576, 64, 1500, 64, 576, 64, 64, 576)[:n % 12])
    rows, held = [], []
    for alloc in (0, 1):
        for name, stride, l3 in layouts:
            buf = cgck.DeviceBuffer(n * stride if stride else cgck.load().cgck_imix_bytes(n))
            desc, out, ver = cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n)
            held += [buf, desc, out, ver]       # the second allocation is made while the first is held
            for rnd in (0, 1):
                for leg, flags, family, wantv in legs:
                    if not flags & cgck.IP6:
                        (eng.synth_imix_ring(buf.ptr, desc.ptr, n, stride, l3, SEED) if stride else
                         eng.synth_imix(buf.ptr, desc.ptr, n, SEED))
                    elif stride:
                        eng.synth_imix_ring_ip6(buf.ptr, desc.ptr, n, stride, l3, 6, SEED)
                    else:
                        eng.synth_imix_ip6(buf.ptr, desc.ptr, n, 6, SEED)
                    eng.set_kernel(family)
                    med, lo, hi, kern = time_desc(eng, buf, desc, out, ver if wantv else None, n, flags)
                    eng.set_kernel("auto")
                    bad = (check_imix6(eng, out, ver if wantv else None, n, stride, l3, 6, flags)
                           if flags & cgck.IP6 else None)
                    r = {"alloc": alloc, "layout": name, "leg": leg, "round": rnd, "packets": n,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "tb_s": round(read / med / 1e9, 3), "pct_hbm_peak": round(100 * read / (med * 1e-3) / HBM_PEAK, 1),
                         "kernel": kern, "oracle_mismatches_of_64": bad}
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
    emit(f"{'layout':7} {'leg':13} {'kernel':30} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  % peak  vs a")
    for name, _, _ in layouts:
        for leg, _, _, _ in sorted(legs):
            sel = [r for r in rows if r["layout"] == name and r["leg"] == leg]
            med = med_of(name, leg)
            emit(f"{name:7} {leg:13} {sel[0]['kernel']:30} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {100 * read / (med * 1e-3) / HBM_PEAK:5.1f}  {med / med_of(name, 'a_ip4'):6.3f}")
        b, c = med_of(name, "b_ip6"), med_of(name, "c_ip6_group")
        emit(f"{name:7} b against c (the group path): {100 * (c - b) / c:+.2f} % of c's time saved; "
             f"c's spread between the two allocations {spread(name, 'c_ip6_group'):.2f} %")
        emit(f"{name:7} b / a = {b / med_of(name, 'a_ip4'):.3f}; a's spread between the two allocations "
             f"{spread(name, 'a_ip4'):.2f} %")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    ap.add_argument("--reverse", action="store_true",
                    help="time each shape's legs in the opposite order (is a difference the leg's or its place's?)")
    ap.add_argument("--imix", action="store_true", help="the mixed-length legs (lpw / lpw6 / cksum6), packed and ring")
    args = ap.parse_args()
    if args.imix:
        return imix_main(args)
    n = args.packets
    eng = cgck.Engine(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    shapes = [("1500", 1500, (("ip4", 1500, cgck.GEN_BOTH), ("ip6", 1500, cgck.GEN_BOTH | cgck.IP6))),
              ("64", 64, (("ip4", 64, cgck.GEN_BOTH), ("ip6", 60, cgck.GEN_BOTH | cgck.IP6),
                          ("ip6_len64", 64, cgck.GEN_BOTH | cgck.IP6)))]
    if args.reverse:
        shapes = [(name, stride, legs[::-1]) for name, stride, legs in shapes]
        emit("legs in reverse order")
    rows = []
    held = []
    for alloc in (0, 1):
        for name, stride, legs in shapes:
            buf = cgck.DeviceBuffer(n * stride)
            out = cgck.DeviceBuffer(4 * n)
            held += [buf, out]          # the second allocation is made while the first is held
            for rnd in (0, 1):
                for leg, ip_len, flags in legs:
                    if flags & cgck.IP6:
                        eng.synth_strided_ip6(buf.ptr, n, stride, ip_len, 6, SEED)
                    else:
                        eng.synth_strided(buf.ptr, n, stride, ip_len, SEED)
                    med, lo, hi, kern = time_leg(eng, buf, out, n, stride, ip_len, flags)
                    bad = check_ip6(eng, out, n, stride, ip_len, 6) if flags & cgck.IP6 else None
                    # bytes the kernel must read: the packets (at 64 B stride whole slots are read)
                    read = n * (stride if stride <= 64 else ip_len)
                    r = {"alloc": alloc, "shape": name, "leg": leg, "round": rnd, "ip_len": ip_len, "packets": n,
                         "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                         "tb_s": round(read / med / 1e9, 3), "pct_hbm_peak": round(100 * read / (med * 1e-3) / HBM_PEAK, 1),
                         "kernel": kern, "oracle_mismatches_of_64": bad}
                    rows.append(r)
                    emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()
    emit("")
    emit(f"{'shape':6} {'leg':10} {'kernel':28} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  vs ip4")
    for name, _, legs in shapes:
        base = statistics.median(r["ms_median"] for r in rows if r["shape"] == name and r["leg"] == "ip4")
        for leg, _, _ in legs:
            sel = [r for r in rows if r["shape"] == name and r["leg"] == leg]
            med = statistics.median(r["ms_median"] for r in sel)
            emit(f"{name:6} {leg:10} {sel[0]['kernel']:28} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {med / base:6.3f}")
        ip4 = [r["ms_median"] for r in rows if r["shape"] == name and r["leg"] == "ip4"]
        a0, a1 = statistics.median(ip4[:2]), statistics.median(ip4[2:])
        emit(f"{name:6} ip4 spread between the two allocations: {100 * abs(a0 - a1) / min(a0, a1):.2f} %")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
