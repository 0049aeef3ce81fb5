#!/usr/bin/env python3
"""cgck_l4_reply and cgck_l4_reply_packed (l4r_kernel) beside cgck_l4_desc and
cgck_pcb_lookup over the same descriptors, the whole receive-to-transmit chain in one
timing, and the host route the call replaces, in one process.

The method is tools/pcb_ab.py's: HIP events through the binding's Event, 5 warm-ups
and the median of 20 calls per leg, the legs interleaved twice, the whole repeated on
a second allocation made while the first is still held, each leg's spread between the
two allocations as its margin, and 64 sampled frames of the reply legs checked against
the referee (tests/l4rref.py).  The set is section 5.15's: 16M header-only frames in
2048-byte slots with the IP header at byte 18, written by cgck_l4_build from the
peers' flows and read back by cgck_l4_desc; the table is the dst-cache-shaped one of
4096 connections, two flows in five IPv6.  Every second frame carries source port 81,
finds no connection and draws an RST.
Legs:
  r    cgck_l4_reply, all five outputs, no `at`                  l4r_kernel<true, true, 0>
  rq   cgck_l4_reply, queue alone (the packed form's first step) l4r_kernel<false, true, 0>
  ao   cgck_l4_reply, all outputs, at = the packed order, a lane's own stores   <true, true, 1>
  at   the same, turned through LDS (cgck_test_l4_reply_store 2)                <true, true, 2>
  po   cgck_l4_reply_packed (reply, steer, reply), own stores
  pt   cgck_l4_reply_packed, turned
  c    cgck_l4_desc, seg + cls                                   l4d_kernel: the yardstick
  l    cgck_pcb_lookup, kind alone                               pcbl_kernel: the other yardstick
  ch   cgck_l4_desc, cgck_pcb_lookup, cgck_l4_reply_packed, cgck_l4_build over n: the chain
  h    the host route: kind[] and seg[] down, the records edited and the flows gathered
       in numpy (from the generator's table: no frame byte is read, which favours it),
       the records and flows up; 3 runs, wall clock

    python tools/l4r_ab.py [--packets N] [--out FILE]

One JSON line per leg, then a table with the ratios to c and l.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("con-gen_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, d))
import cgck  # noqa: E402
import l4bref  # noqa: E402
import l4rref  # noqa: E402
import pcb_ab  # noqa: E402

STRIDE, CHUNK, NCONN, TXSLOT = pcb_ab.STRIDE, pcb_ab.CHUNK, 4096, 128
LEGS = ("r_reply_all", "rq_reply_queue", "ao_reply_at_own", "at_reply_at_turned", "po_packed_own", "pt_packed_turned",
        "c_l4_desc", "l_pcb_lookup_kind", "ch_chain", "h_host_route")
CHECKED = ("r_reply_all", "ao_reply_at_own", "at_reply_at_turned", "po_packed_own", "pt_packed_turned")


def records(k):
    """pcb_ab.records with every second frame a miss."""
    slot, seg, j, _ = pcb_ab.records(k, NCONN)
    hit = np.asarray(k, np.uint64) % 2 == 0
    seg["sport"] = pcb_ab.be16(np.where(hit, 80, 81))
    seg["th_flags"] = np.where(np.asarray(k, np.uint64) % 6 < 3, 0x10, 0x02)
    return slot, seg, j, hit


def link_rec():
    f = np.zeros(1, l4bref.FLOW_DTYPE)[0]
    f["eth_dst"], f["eth_src"], f["ttl"] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2), 64
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--out", default=None, help="also write the lines and the table here")
    args = ap.parse_args()
    n = args.packets
    eng = cgck.Engine(0)
    link = link_rec()
    lines, rows, held = [], [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    D = cgck.DeviceBuffer
    ks = np.unique(np.minimum(np.linspace(0, n - 1, 64).astype(np.int64) + np.arange(64) % 41, n - 1))
    conn, flow, peer = pcb_ab.table(NCONN)
    nrst = n // 2                                       # the odd frames
    for alloc in (0, 1):
        buf, tx = D(n * STRIDE), D(n * TXSLOT)
        slot, seg, fidx, desc, txslot = D(12 * n), D(32 * n), D(4 * n), D(12 * n), D(12 * n)
        sg, c4, kind, scr, scls = D(32 * n), D(n), D(n), D(32 * n), D(n)
        rseg, rflow, rcls, rq, cnt = D(32 * n), D(48 * n), D(n), D(n), D(4 * l4rref.NCOUNT)
        pq, pat, qoff, work = D(n), D(4 * n), D(12), D(max(cgck.steer_work_bytes(n, 1), 4))
        dconn, dflow, dpeer, dtab = D(12 * NCONN), D(48 * NCONN), D(48 * NCONN), D(cgck.pcb_table_bytes(NCONN))
        held += [buf, tx, slot, seg, fidx, desc, txslot, sg, c4, kind, scr, scls, rseg, rflow, rcls, rq, cnt, pq, pat, qoff, work,
                 dconn, dflow, dpeer, dtab]
        for dv, a in ((dconn, conn), (dflow, flow), (dpeer, peer)):
            dv.upload(a, stream=eng.stream)
        for a in range(0, n, CHUNK):
            k = np.arange(a, min(a + CHUNK, n))
            s_, g_, f_, _ = records(k)
            slot.upload(s_, off=12 * a, stream=eng.stream)
            seg.upload(g_, off=32 * a, stream=eng.stream)
            fidx.upload(f_, off=4 * a, stream=eng.stream)
            t_ = np.zeros(len(k), l4bref.DESC_DTYPE)
            t_["frame_off"], t_["ip_len"] = k.astype(np.uint64) * TXSLOT, TXSLOT
            txslot.upload(t_, off=12 * a, stream=eng.stream)
            eng.sync()
        eng.l4_build(buf.ptr, n, slot.ptr, seg.ptr, dpeer.ptr, NCONN, fidx=fidx.ptr, ip_id0=1, ip_off=0x4000, desc_out=desc.ptr)
        pcb = cgck.Pcb(dconn.ptr, NCONN, dflow.ptr, NCONN, dtab.ptr, cgck.pcb_table_bytes(NCONN), None)
        eng.pcb_build(pcb)
        eng.l4_desc(buf.ptr, desc.ptr, n, seg=sg.ptr, cls=c4.ptr)
        eng.pcb_lookup(buf.ptr, desc.ptr, sg.ptr, n, pcb, cls=c4.ptr, kind=kind.ptr)
        eng.sync()
        # the sample's expectation: the referee over the sampled frames' own bytes and records
        sdesc = pcb_ab.fetch(eng, desc, ks, l4bref.DESC_DTYPE)
        sseg, sc, sk = pcb_ab.fetch(eng, sg, ks, l4bref.SEG_DTYPE), pcb_ab.fetch(eng, c4, ks, np.uint8), pcb_ab.fetch(eng, kind, ks, np.uint8)
        sbuf = pcb_ab.fetch(eng, buf, ks, np.dtype((np.uint8, 128)), STRIDE).reshape(-1)
        rd = sdesc.copy()
        rd["frame_off"] = np.arange(len(ks)) * 128
        wc, ws, wf = l4rref.per_frame(sbuf, rd, sseg, link, cls=sc, kind=sk)
        assert np.array_equal((wc & 15) == l4rref.RST, ks % 2 == 1)
        want_at = np.where(ks % 2 == 1, ks // 2, nrst + ks // 2)     # the packed order: RSTs first, both in arrival order

        def reply(at=None, allout=True, m=n):
            if allout:
                eng.l4_reply(buf.ptr, m, desc.ptr, sg.ptr, link, cls=c4.ptr, kind=kind.ptr, at=at, seg_out=rseg.ptr, flow_out=rflow.ptr,
                             cls_out=rcls.ptr, queue=rq.ptr, count=cnt.ptr)
            else:
                eng.l4_reply(buf.ptr, m, desc.ptr, sg.ptr, link, cls=c4.ptr, kind=kind.ptr, queue=rq.ptr)

        def packed(m=n):
            eng.l4_reply_packed(buf.ptr, m, desc.ptr, sg.ptr, link, pq.ptr, pat.ptr, qoff.ptr, work=work.ptr, cls=c4.ptr, kind=kind.ptr,
                                seg_out=rseg.ptr, flow_out=rflow.ptr, cls_out=rcls.ptr, count=cnt.ptr)

        def chain():
            eng.l4_desc(buf.ptr, desc.ptr, n, seg=scr.ptr, cls=scls.ptr)
            eng.pcb_lookup(buf.ptr, desc.ptr, scr.ptr, n, pcb, cls=scls.ptr, kind=kind.ptr)
            eng.l4_reply_packed(buf.ptr, n, desc.ptr, scr.ptr, link, pq.ptr, pat.ptr, qoff.ptr, work=work.ptr, cls=scls.ptr, kind=kind.ptr,
                                seg_out=rseg.ptr, flow_out=rflow.ptr, cls_out=rcls.ptr)
            eng.l4_build(tx.ptr, n, txslot.ptr, rseg.ptr, rflow.ptr, n, cls=rcls.ptr, ip_id0=7, ip_off=0x4000)

        def host_route():
            hk, hs = np.zeros(n, np.uint8), np.zeros(n, l4bref.SEG_DTYPE)
            for a in range(0, n, CHUNK):
                kind.download(hk[a:a + CHUNK], off=a, stream=eng.stream)
                sg.download(hs[a:a + CHUNK], off=32 * a, stream=eng.stream)
            eng.sync()
            miss = np.nonzero(hk == cgck.PCB_MISS)[0]
            s = hs[miss]
            r = np.zeros(len(miss), l4bref.SEG_DTYPE)
            ack = (s["th_flags"] & 0x10) != 0
            r["sport"], r["dport"] = s["dport"], s["sport"]
            r["seq"] = np.where(ack, s["ack"], 0)
            r["ack"] = np.where(ack, 0, s["seq"] + s["pay_len"] + ((s["th_flags"] >> 1) & 1))
            r["th_flags"] = np.where(ack, 0x04, 0x14)
            f = flow[records(miss)[2]]                  # the receiver's flow of the frame's connection: the swapped addresses
            f["eth_dst"], f["eth_src"], f["ttl"] = link["eth_dst"], link["eth_src"], link["ttl"]
            for a in range(0, len(miss), CHUNK):
                rseg.upload(r[a:a + CHUNK], off=32 * a, stream=eng.stream)
                rflow.upload(f[a:a + CHUNK], off=48 * a, stream=eng.stream)
            eng.sync()

        def wall(eng_, launch):
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                launch()
                ms.append(1e3 * (time.perf_counter() - t0))
            return statistics.median(ms), min(ms), max(ms)

        def shaped(shape, fn):
            def clock(eng_, launch):
                cgck.l4_reply_store(shape)
                try:
                    return pcb_ab.timed(eng_, launch)
                finally:
                    cgck.l4_reply_store(cgck.L4R_STORE_DEFAULT)
            return fn, clock

        packed()                                        # pat: the packed order, the `at` of the two at legs
        eng.sync()
        legs = ((reply, pcb_ab.timed), (lambda: reply(allout=False), pcb_ab.timed),
                shaped(cgck.L4R_STORE_OWN, lambda: reply(at=pat.ptr)), shaped(cgck.L4R_STORE_TURNED, lambda: reply(at=pat.ptr)),
                shaped(cgck.L4R_STORE_OWN, packed), shaped(cgck.L4R_STORE_TURNED, packed),
                (lambda: eng.l4_desc(buf.ptr, desc.ptr, n, seg=scr.ptr, cls=scls.ptr), pcb_ab.timed),
                (lambda: eng.pcb_lookup(buf.ptr, desc.ptr, sg.ptr, n, pcb, cls=c4.ptr, kind=kind.ptr), pcb_ab.timed),
                (chain, pcb_ab.timed), (host_route, wall))
        for rnd in (0, 1):
            for leg, (fn, clock) in zip(LEGS, legs):
                if leg == "h_host_route" and rnd == 1:
                    continue
                cnt.upload(np.zeros(l4rref.NCOUNT, np.uint32), stream=eng.stream)
                med, lo, hi = clock(eng, fn)
                kern = eng.last_kernel
                miss = 0
                if leg in CHECKED:
                    at = ks if leg == "r_reply_all" else want_at
                    miss += int(np.count_nonzero(pcb_ab.fetch(eng, rseg, at, l4bref.SEG_DTYPE) != ws))
                    miss += int(np.count_nonzero(pcb_ab.fetch(eng, rflow, at, l4bref.FLOW_DTYPE) != wf))
                    miss += int(np.count_nonzero(pcb_ab.fetch(eng, rcls, at, np.uint8) != wc))
                    gn = np.zeros(l4rref.NCOUNT, np.uint32)
                    cnt.download(gn, stream=eng.stream)
                    eng.sync()
                    miss += int(int(gn[l4rref.RST]) != 25 * nrst) + int(int(gn[l4rref.NOTMISS]) != 25 * (n - nrst))
                    if leg.startswith("p"):
                        go = np.zeros(3, np.uint32)
                        qoff.download(go, stream=eng.stream)
                        eng.sync()
                        miss += int(go.tolist() != [0, nrst, n])
                        miss += int(np.count_nonzero(pcb_ab.fetch(eng, pat, ks, np.uint32) != want_at))
                r = {"alloc": alloc, "leg": leg, "round": rnd, "packets": n, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                     "ms_max": round(hi, 4), "kernel": kern, "referee_mismatches": miss, "sampled": len(ks) if leg in CHECKED else 0}
                rows.append(r)
                emit(json.dumps(r))
    for b in held:
        b.free()
    eng.close()

    def med_of(leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["leg"] == leg and alloc in (None, r["alloc"]))

    emit("")
    emit(f"{n} frames, every second one an RST, {NCONN} connections")
    emit(f"{'leg':20} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1)) + "   median  margin %   / c     / l    kernel")
    c, l = med_of("c_l4_desc"), med_of("l_pcb_lookup_kind")
    for leg in LEGS:
        sel = [r for r in rows if r["leg"] == leg]
        med, m0, m1 = med_of(leg), med_of(leg, 0), med_of(leg, 1)
        emit(f"{leg:20} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel) + " " * (9 * (4 - len(sel)))
             + f"  {med:7.4f}  {100 * abs(m0 - m1) / min(m0, m1):8.2f}  {med / c:6.3f}  {med / l:6.3f}  {sel[0]['kernel']}")
    emit(f"at / ao = {med_of('at_reply_at_turned') / med_of('ao_reply_at_own'):.3f}, "
         f"pt / po = {med_of('pt_packed_turned') / med_of('po_packed_own'):.3f}, "
         f"h / po = {med_of('h_host_route') / med_of('po_packed_own'):.1f}")
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    emit("not measured: bursts of a few hundred frames, a random `at`, verdict and l2cls arrays, the flags, an all-IPv6 "
         "burst, a host route that reads the frames' addresses, counters from rocprofv3")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
