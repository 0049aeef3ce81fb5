#!/usr/bin/env python3
"""cgck_pcb_lookup and cgck_pcb_build (pcbl_kernel, pcbb_kernel) under both table
shapes, beside cgck_l4_desc and cgck_rss_desc over the same descriptors, in one
process.

The method is tools/l4b_ab.py's: HIP events through the binding's Event, 5 warm-ups
and the median of 20 calls per leg, the legs interleaved twice, the whole repeated
on a second allocation made while the first is still held, each leg's spread between
the two allocations as its margin, and 64 sampled frames of every lookup leg checked
against the referee (tests/pcbref.py).  The set is section 5.14's: 16M header-only
frames in 2048-byte slots with the IP header at byte 18, written here by
cgck_l4_build from the peers' flows and read back by cgck_l4_desc, so the lookup's
inputs are the receive pipeline's own.  The table is dst-cache-shaped: connection i
is {flow i, lport 5000 + i % 60000, fport 80, TCP}, two flows in five IPv6, a local
address per connection; nconn is 4096 and 4M.  Frame k belongs to connection
(k * 2654435761) % nconn; every fourth frame carries source port 81 and misses.
Legs, per nconn:
  la   cgck_pcb_lookup, idx + fidx + kind + count, 8-byte slots   pcbl_kernel<true, true, true>
  li   cgck_pcb_lookup, idx alone, 8-byte slots                   pcbl_kernel<true, false, true>
  ua   as la with 4-byte slots (cgck_test_pcb_mode 2)             pcbl_kernel<true, true, false>
  ui   as li with 4-byte slots                                    pcbl_kernel<true, false, false>
  c    cgck_l4_desc, seg only                                     l4d_kernel: the yardstick
  d    cgck_rss_desc, hash only                                   rssf_kernel: the other yardstick
  bt   cgck_pcb_build, 8-byte slots (the memset included)         pcbb_kernel<true>
  bu   cgck_pcb_build, 4-byte slots                               pcbb_kernel<false>

    python tools/pcb_ab.py [--packets N] [--small] [--out FILE]

One JSON line per leg, then a table with the ratios to c and d.  --small adds the
microseconds per call of la, c and d at 256 and 4096 frames.  The sample's
expectation: with nconn 4096 the referee's dict over the whole table; with 4M (four
million dict inserts a run) the referee's key compare of the reported connection
(pcbref.true_hit) and the index the generator chose, which is the only one with
that key.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("con-gen_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import cgck  # noqa: E402
import l4bref  # noqa: E402
import pcbref  # noqa: E402

STRIDE, CHUNK = 2048, 1 << 20
LOOKUPS = ("la_lookup_all", "li_lookup_idx", "ua_lookup_all_4B", "ui_lookup_idx_4B")
LEGS = LOOKUPS + ("c_l4_desc_seg", "d_rss_desc", "bt_build", "bu_build_4B")
HF = cgck.RSS_TCP | cgck.RSS_UDP


def be16(v):
    v = np.asarray(v, np.uint32)
    return (((v & 255) << 8) | (v >> 8)).astype(np.uint16)


def table(nconn):
    """(conn, flow) of the receiver and the peers' flows the frames are built from."""
    i = np.arange(nconn, dtype=np.uint32)
    flow = np.zeros(nconn, l4bref.FLOW_DTYPE)
    flow["flags"] = np.where(i % 5 < 2, l4bref.FLOW_IP6, 0)
    flow["ttl"] = 64
    flow["eth_dst"][:, 5], flow["eth_src"][:, 5] = 1, 2
    flow["laddr"][:, 0], flow["faddr"][:, 0] = 10, 10
    flow["laddr"][:, 1:4] = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=1)
    flow["faddr"][:, 1:4] = (1, 0, 1)
    six = (flow["flags"] & l4bref.FLOW_IP6) != 0
    flow["laddr"][six, 15], flow["faddr"][six, 15] = 0x11, 0x22
    conn = np.zeros(nconn, pcbref.CONN_DTYPE)
    conn["flow"], conn["lport"], conn["fport"], conn["proto"] = i, be16(5000 + i % 60000), be16(80), 6
    peer = flow.copy()
    peer["laddr"], peer["faddr"] = flow["faddr"], flow["laddr"]
    return conn, flow, peer


def records(k, nconn):
    """(slot, seg, fidx, hit) of the frames k as the peers send them."""
    k = np.asarray(k, np.uint64)
    j = ((k * np.uint64(2654435761)) % np.uint64(nconn)).astype(np.uint32)
    hit = k % 4 != 3
    seg = np.zeros(len(k), l4bref.SEG_DTYPE)
    seg["seq"], seg["ack"] = k & np.uint64(0xFFFFFFFF), (k * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    seg["sport"], seg["dport"] = be16(np.where(hit, 80, 81)), be16(5000 + j % 60000)
    seg["win"], seg["th_flags"] = 0xFFFF, 0x10
    slot = np.zeros(len(k), l4bref.DESC_DTYPE)
    slot["frame_off"], slot["l3_off"], slot["ip_len"] = k * np.uint64(STRIDE), 4, STRIDE - 4
    return slot, seg, j, hit


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


def fetch(eng, dev, ks, dtype, unit=None):
    got = np.zeros(len(ks), dtype)
    step = got.itemsize if unit is None else unit
    for i, k in enumerate(ks):
        dev.download(got[i:i + 1], off=step * int(k), stream=eng.stream)
    eng.sync()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--nconn", type=int, nargs="*", default=[4096, 4 << 20])
    ap.add_argument("--small", action="store_true", help="also time bursts of 256 and 4096 frames")
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    with open(os.path.join(ROOT, "tests", "golden", "rss.json")) as f:
        key = np.frombuffer(bytes.fromhex(json.load(f)["freebsd_rss_key"]), np.uint8).copy()
    eng = cgck.Engine(0)
    spec = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, 0)
    lines, rows, small, held = [], [], [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    ks = np.unique(np.minimum(np.linspace(0, n - 1, 64).astype(np.int64) + np.arange(64) % 41, n - 1))
    for alloc in (0, 1):
        buf = cgck.DeviceBuffer(n * STRIDE)
        slot, seg, fidx, desc = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(4 * n),
                                 cgck.DeviceBuffer(12 * n))
        sg, c4, scratch, hsh = cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(n), cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(4 * n)
        oi, of, ok, cnt, stat = (cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(n),
                                 cgck.DeviceBuffer(4 * pcbref.NCOUNT), cgck.DeviceBuffer(16))
        held += [buf, slot, seg, fidx, desc, sg, c4, scratch, hsh, oi, of, ok, cnt, stat]
        for nconn in args.nconn:
            conn, flow, peer = table(nconn)
            dconn, dflow, dpeer = cgck.DeviceBuffer(12 * nconn), cgck.DeviceBuffer(48 * nconn), cgck.DeviceBuffer(48 * nconn)
            tbytes = cgck.pcb_table_bytes(nconn)
            dtab = cgck.DeviceBuffer(tbytes)
            held += [dconn, dflow, dpeer, dtab]
            for dv, a in ((dconn, conn), (dflow, flow), (dpeer, peer)):
                raw = a.view(np.uint8).reshape(-1)
                for o in range(0, len(raw), 32 << 20):
                    dv.upload(raw[o:o + (32 << 20)], off=o, stream=eng.stream)
                eng.sync()
            for a in range(0, n, CHUNK):
                s_, g_, f_, _ = records(np.arange(a, min(a + CHUNK, n)), nconn)
                slot.upload(s_, off=12 * a, stream=eng.stream)
                seg.upload(g_, off=32 * a, stream=eng.stream)
                fidx.upload(f_, off=4 * a, stream=eng.stream)
                eng.sync()
            # the frames as the peers send them, and the receive pipeline's records of them
            eng.l4_build(buf.ptr, n, slot.ptr, seg.ptr, dpeer.ptr, nconn, fidx=fidx.ptr, ip_id0=1, ip_off=0x4000, desc_out=desc.ptr)
            eng.l4_desc(buf.ptr, desc.ptr, n, seg=sg.ptr, cls=c4.ptr)
            eng.sync()
            pcb = cgck.Pcb(dconn.ptr, nconn, dflow.ptr, nconn, dtab.ptr, tbytes, None)
            _, _, sj, shit = records(ks, nconn)
            want_idx = np.where(shit, sj, pcbref.NOIDX).astype(np.uint32)
            want_kind = np.where(shit, pcbref.HIT, pcbref.MISS).astype(np.uint8)
            sdesc = fetch(eng, desc, ks, l4bref.DESC_DTYPE)
            sseg, scls = fetch(eng, sg, ks, l4bref.SEG_DTYPE), fetch(eng, c4, ks, np.uint8)
            sbuf = fetch(eng, buf, ks, np.dtype((np.uint8, 128)), STRIDE).reshape(-1)
            rd = sdesc.copy()
            rd["frame_off"] = np.arange(len(ks)) * 128
            if nconn <= 1 << 16:
                ri, rf, rk, _ = pcbref.lookup(sbuf, rd, sseg, scls, conn, flow)
                assert np.array_equal(ri, want_idx) and np.array_equal(rk, want_kind) and np.array_equal(rf, want_idx)
            for i in range(len(ks)):                    # the generator's index is the one the referee's key compare accepts
                o = int(rd["frame_off"][i]) + int(rd["l3_off"][i])
                assert pcbref.true_hit(sbuf[o:o + int(rd["ip_len"][i])], scls[i], sseg[i], conn, flow, int(sj[i])) == bool(shit[i])

            def lookup(allout, m=n):
                if allout:
                    eng.pcb_lookup(buf.ptr, desc.ptr, sg.ptr, m, pcb, cls=c4.ptr, idx=oi.ptr, fidx=of.ptr, kind=ok.ptr, count=cnt.ptr)
                else:
                    eng.pcb_lookup(buf.ptr, desc.ptr, sg.ptr, m, pcb, cls=c4.ptr, idx=oi.ptr)

            def moded(mode, fn):
                """(launch, clock): the table rebuilt under `mode` first, the mode pinned around the timing."""
                def clock(eng_, launch):
                    cgck.pcb_mode(mode)
                    try:
                        eng_.pcb_build(pcb, stat.ptr)
                        return timed(eng_, launch)
                    finally:
                        cgck.pcb_mode(0)
                return fn, clock

            legs = (moded(0, lambda m=n: lookup(True, m)), moded(0, lambda m=n: lookup(False, m)),
                    moded(2, lambda m=n: lookup(True, m)), moded(2, lambda m=n: lookup(False, m)),
                    (lambda m=n: eng.l4_desc(buf.ptr, desc.ptr, m, seg=scratch.ptr), timed),
                    (lambda m=n: eng.rss_desc(buf.ptr, desc.ptr, m, spec, hash=hsh.ptr), timed),
                    moded(0, lambda: eng.pcb_build(pcb, stat.ptr)), moded(2, lambda: eng.pcb_build(pcb, stat.ptr)))
            for rnd in (0, 1):
                for leg, (fn, clock) in zip(LEGS, legs):
                    for k in ks:                        # what the leg writes of the sample is written anew
                        oi.upload(np.full(4, 0xEE, np.uint8), off=4 * int(k), stream=eng.stream)
                        of.upload(np.full(4, 0xEE, np.uint8), off=4 * int(k), stream=eng.stream)
                        ok.upload(np.full(1, 0xEE, np.uint8), off=int(k), stream=eng.stream)
                    cnt.upload(np.zeros(pcbref.NCOUNT, np.uint32), stream=eng.stream)
                    med, lo, hi = clock(eng, fn)
                    kern = eng.last_kernel
                    miss = 0
                    if leg in LOOKUPS:
                        miss += int(np.count_nonzero(fetch(eng, oi, ks, np.uint32) != want_idx))
                        if "all" in leg:
                            gn = np.zeros(pcbref.NCOUNT, np.uint32)
                            cnt.download(gn, stream=eng.stream)
                            eng.sync()
                            miss += int(np.count_nonzero(fetch(eng, of, ks, np.uint32) != want_idx))    # flow i of connection i
                            miss += int(np.count_nonzero(fetch(eng, ok, ks, np.uint8) != want_kind))
                            miss += int(int(gn[0]) != 25 * (n - n // 4)) + int(int(gn[2]) != 25 * (n // 4)) + int(gn[1] or gn[3] or gn[4])
                    if leg.startswith("b"):
                        gs = np.zeros(4, np.uint32)
                        stat.download(gs, stream=eng.stream)
                        eng.sync()
                        miss += int(gs.tolist() != [nconn, 0, 0, 0])
                    r = {"alloc": alloc, "nconn": nconn, "leg": leg, "round": rnd, "packets": n, "ms_median": round(med, 4),
                         "ms_min": round(lo, 4), "ms_max": round(hi, 4), "kernel": kern, "referee_mismatches": miss,
                         "sampled": len(ks) if leg in LOOKUPS else 0}
                    rows.append(r)
                    emit(json.dumps(r))
            if args.small and alloc == 0:
                for m in (256, 4096):
                    for leg, (fn, clock) in zip(("la_lookup_all", "c_l4_desc_seg", "d_rss_desc"), (legs[0], legs[4], legs[5])):
                        med, lo, hi = clock(eng, lambda: fn(m))
                        small.append({"nconn": nconn, "leg": leg, "packets": m, "us_median": round(1e3 * med, 2),
                                      "us_min": round(1e3 * lo, 2), "us_max": round(1e3 * hi, 2), "kernel": eng.last_kernel})
                        emit(json.dumps(small[-1]))
    for b in held:
        b.free()
    eng.close()

    def med_of(nconn, leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["leg"] == leg and r["nconn"] == nconn and alloc in (None, r["alloc"]))

    emit("")
    for nconn in args.nconn:
        emit(f"nconn {nconn}, {n} frames, three in four hit")
        emit(f"{'leg':18} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1)) + "   median  margin %   / c     / d    kernel")
        c, d = med_of(nconn, "c_l4_desc_seg"), med_of(nconn, "d_rss_desc")
        for leg in LEGS:
            sel = [r for r in rows if r["leg"] == leg and r["nconn"] == nconn]
            med, m0, m1 = med_of(nconn, leg), med_of(nconn, leg, 0), med_of(nconn, leg, 1)
            emit(f"{leg:18} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
                 + f"  {med:7.4f}  {100 * abs(m0 - m1) / min(m0, m1):8.2f}  {med / c:6.3f}  {med / d:6.3f}  {sel[0]['kernel']}")
        emit(f"ua / la = {med_of(nconn, 'ua_lookup_all_4B') / med_of(nconn, 'la_lookup_all'):.3f}, "
             f"ui / li = {med_of(nconn, 'ui_lookup_idx_4B') / med_of(nconn, 'li_lookup_idx'):.3f}, "
             f"bu / bt = {med_of(nconn, 'bu_build_4B') / med_of(nconn, 'bt_build'):.3f}")
    if small:
        emit("small bursts, microseconds per call (median of 20): "
             + ", ".join(f"{s['leg']} at {s['packets']} (nconn {s['nconn']}): {s['us_median']}" for s in small))
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    emit("not measured: a table with long chains (a load factor above one half is not built), tables of duplicates, bursts "
         "whose frames all miss or all hit one connection, IPv6-only tables, bound[] in use, counters from rocprofv3")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
