#!/usr/bin/env python3
"""cgck_l4_build (l4b_kernel) beside the parse of the frames it writes, in one process
(DESIGN.md section 5.14).

The method is tools/l4_ab.py's: HIP events through the binding's Event, 5 warm-ups
and the median of 20 calls per leg, the legs interleaved twice (a b at bt c d, twice),
the whole repeated on a second allocation made while the first is still held, and
64 sampled frames of every leg checked against the referees (tests/l4bref.py for
the frames and the builder's outputs, tests/l4ref.py for c, tests/rssref.py over the
oracle's port for d).  The set is 16M well-formed, header-only frames in 2048-byte
slots with the IP header at byte 18: two in five IPv6, a tagged frame every eighth,
and by k % 4 a SYN (MSS + WS + TS), an ACK (TS), a FIN | ACK without options and a
UDP datagram, over 4000 flows.  Legs (a and b with every dword stored from its own
lane, at and bt the same calls with the header's whole 16-byte granules turned through
LDS: the store shapes are pinned with cgck_test_l4_build_store):
  a   cgck_l4_build, raw_out + desc_out + cls + count   l4b_kernel<true, true, false>
  b   cgck_l4_build, frames only                        l4b_kernel<false, false, false>
  at  as a, turned                                      l4b_kernel<true, true, true>
  bt  as b, turned                                      l4b_kernel<false, false, true>
  c   cgck_l4_desc, seg only, over the frames b wrote   l4d_kernel<true, false>: the yardstick
  d   cgck_rss_desc (hash only), same descriptors       rssf_kernel<true, false>

    python tools/l4b_ab.py [--packets N] [--small] [--out FILE]

One JSON line per leg, then a table with a / c, b / c, at / c and bt / c, each leg's spread between
the two allocations as its margin.  Bytes are counted from the shapes: the 128-byte
line that holds a frame's header (written by a and b, read by c and d: one line per
frame in this layout), the per-frame inputs (slot 12, seg 32, cls 1, fidx 4 for the
build; the descriptor 12 for c and d) and the outputs; the 192 KB flow table stays
in the caches and is not counted.  --small adds the microseconds per call of a, at,
c and d at 256 and 4096 frames, where a call is launch-bound.
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
import l4bref  # noqa: E402
import l4ref  # noqa: E402
import oracle  # noqa: E402
import rssref  # noqa: E402

HBM_PEAK = 8.0e12
STRIDE, NFLOW, ID0, IP_OFF = 2048, 4000, 0xFFF0, 0x4000
LEGS = ("a_build_all", "b_build_frames", "at_build_all_turned", "bt_build_frames_turned", "c_l4_desc_seg", "d_rss_desc")
BUILD_ALL, BUILD_FRAMES = ("a_build_all", "at_build_all_turned"), ("b_build_frames", "bt_build_frames_turned")
HF = cgck.RSS_TCP | cgck.RSS_UDP
CHUNK = 1 << 20


def flows():
    rng = np.random.default_rng(0xF10)
    f = np.zeros(NFLOW, l4bref.FLOW_DTYPE)
    f.view(np.uint8)[:] = rng.integers(0, 256, f.nbytes, dtype=np.uint8)
    i = np.arange(NFLOW)
    f["flags"] = np.where(i % 5 < 2, l4bref.FLOW_IP6, 0) | np.where(i % 8 == 0, l4bref.FLOW_VLAN, 0)
    f["ttl"] = 64
    f["eth_dst"][:, 0] &= 0xFE                           # unicast
    return f


def hdr_len(k, flow):
    """L of the frames k: every frame is header-only."""
    k = np.asarray(k, np.uint64)
    ff = flow["flags"][(k % NFLOW).astype(np.int64)]
    return (np.where(ff & l4bref.FLOW_VLAN, 18, 14) + np.where(ff & l4bref.FLOW_IP6, 40, 20)
            + np.array([40, 32, 20, 8])[(k % 4).astype(np.int64)]).astype(np.int64)


def records(k, flow, at=None):
    """(slot, seg, cls, fidx) of the frames k (an index array).  at: the frames'
    offsets in the packed layout (cap == L, l3_off 0); None: 2048-byte slots."""
    k = np.asarray(k, np.uint64)
    kind = (k % 4).astype(np.int64)
    seg = np.zeros(len(k), l4bref.SEG_DTYPE)
    seg["seq"] = (k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    seg["ack"] = np.where(kind == 0, 0, (k * np.uint64(40503) + np.uint64(1)) & np.uint64(0xFFFFFFFF))
    seg["sport"], seg["dport"] = 1024 + k % 60000, 0x5000
    tcp, opt = kind != 3, np.array([7, 4, 0, 0])[kind]
    seg["win"] = np.where(tcp, 0xFFFF, 0)
    seg["th_flags"] = np.array([0x02, 0x10, 0x11, 0])[kind]
    seg["opt"] = opt
    seg["mss"], seg["wscale"] = np.where(opt & 1, 1460, 0), np.where(opt & 2, 7, 0)
    seg["ts_val"] = np.where(opt & 4, k & np.uint64(0xFFFFFFFF), 0)
    seg["ts_ecr"] = np.where((opt & 4) != 0, (k ^ np.uint64(0x5A5A5A5A)) & np.uint64(0xFFFFFFFF), 0)
    fidx = (k % NFLOW).astype(np.uint32)
    slot = np.zeros(len(k), l4bref.DESC_DTYPE)
    slot["frame_off"] = k * np.uint64(STRIDE)
    slot["l3_off"] = np.where(flow["flags"][fidx] & l4bref.FLOW_VLAN, 0, 4)    # the IP header at byte 18 either way
    slot["ip_len"] = STRIDE - slot["l3_off"]
    if at is not None:
        slot["frame_off"], slot["l3_off"], slot["ip_len"] = at, 0, hdr_len(k, flow)
    return slot, seg, np.where(tcp, l4bref.SEG_TCP, l4bref.SEG_UDP).astype(np.uint8), fidx


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
    """Elements ks of a device array (unit: bytes between elements)."""
    got = np.zeros(len(ks), dtype)
    step = got.itemsize if unit is None else unit
    for i, k in enumerate(ks):
        dev.download(got[i:i + 1], off=step * int(k), stream=eng.stream)
    eng.sync()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16 << 20)
    ap.add_argument("--small", action="store_true", help="also time bursts of 256 and 4096 frames")
    ap.add_argument("--packed", action="store_true", help="the frames back to back (cap == L) instead of in 2048-byte slots")
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

    flow = flows()
    # 64 frames spread over the set, every family, tag and kind among them; the referee's frames and outputs
    ks = np.unique(np.minimum(np.linspace(0, n - 1, 64).astype(np.int64) + np.arange(64) % 41, n - 1))
    off = None                                          # --packed: every frame's offset
    if args.packed:
        L = np.concatenate([hdr_len(np.arange(a, min(a + CHUNK, n)), flow) for a in range(0, n, CHUNK)])
        off = np.cumsum(L) - L
        nbytes = int(L.sum())
        emit(f"packed layout: {nbytes} bytes of frames back to back, cap == L")
    else:
        nbytes = n * STRIDE
    sslot, sseg, scls, sfidx = records(ks, flow, None if off is None else off[ks])
    rel = sslot.copy()
    rel["frame_off"] = np.arange(len(ks)) * 128
    want_buf = np.full(128 * len(ks), 0xEE, np.uint8)
    want_raw, want_desc, want_cls = [], [], np.zeros(len(ks), np.uint8)
    for i, k in enumerate(ks):                          # one frame a call: ip_id0 + k is the id
        r, d, c, _ = l4bref.build(want_buf, rel[i:i + 1], sseg[i:i + 1], flow, scls[i:i + 1], sfidx[i:i + 1],
                                  (ID0 + int(k)) & 0xFFFF, IP_OFF)
        r["frame_off"] = d["frame_off"] = int(sslot["frame_off"][i])
        want_raw.append(r[0])
        want_desc.append(d[0])
        want_cls[i] = c[0]
    want_raw, want_desc = np.array(want_raw, l4bref.DESC_DTYPE), np.array(want_desc, l4bref.DESC_DTYPE)
    want_frames = want_buf.reshape(len(ks), 128)
    rd = want_desc.copy()
    rd["frame_off"] = np.arange(len(ks)) * 128
    want_seg = l4ref.expect(want_buf, rd)[0]
    offs = rd["frame_off"].astype(np.int64) + rd["l3_off"]
    want_hash = rssref.expect(P, want_buf, offs, rd["ip_len"].astype(np.int64), key, HF)[0]
    emit("sampled classes: " + json.dumps({f"{l4bref.NAMES[int(c) & 15]}{'6' if c & 16 else '4'}": int(np.count_nonzero(want_cls == c))
                                           for c in sorted(set(want_cls.tolist()))}))
    hdr = int(sum(int(r) for r in want_raw["ip_len"])) / len(ks)
    spec = cgck.Engine.rss_spec(key, 0xFFFFFFFF, HF, 0)
    per_in = 12 + 32 + 1 + 4
    line = nbytes / n if args.packed else 128           # bytes of frame memory a frame's header touches
    moved = {"a_build_all": (line + per_in + 12 + 12 + 1) * n, "b_build_frames": (line + per_in) * n,
             "at_build_all_turned": (line + per_in + 12 + 12 + 1) * n, "bt_build_frames_turned": (line + per_in) * n,
             "c_l4_desc_seg": (line + 12 + 32) * n, "d_rss_desc": (line + 12 + 4) * n}
    moved = {x: int(v) for x, v in moved.items()}
    rows, held, small = [], [], []
    for alloc in (0, 1):
        buf = cgck.DeviceBuffer(nbytes)
        slot, seg, cls, fidx, fl = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(n),
                                    cgck.DeviceBuffer(4 * n), cgck.DeviceBuffer(48 * NFLOW))
        raw, desc, co, cnt = (cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(12 * n), cgck.DeviceBuffer(n),
                              cgck.DeviceBuffer(4 * l4bref.NCOUNT))
        sg, hsh = cgck.DeviceBuffer(32 * n), cgck.DeviceBuffer(4 * n)
        held += [buf, slot, seg, cls, fidx, fl, raw, desc, co, cnt, sg, hsh]    # the second allocation is made while the first is held
        fl.upload(flow, stream=eng.stream)
        for a in range(0, n, CHUNK):
            s_, g_, c_, f_ = records(np.arange(a, min(a + CHUNK, n)), flow, None if off is None else off[a:a + CHUNK])
            slot.upload(s_, off=12 * a, stream=eng.stream)
            seg.upload(g_, off=32 * a, stream=eng.stream)
            cls.upload(c_, off=a, stream=eng.stream)
            fidx.upload(f_, off=4 * a, stream=eng.stream)
            eng.sync()

        def leg_a(m=n):
            eng.l4_build(buf.ptr, m, slot.ptr, seg.ptr, fl.ptr, NFLOW, cls=cls.ptr, fidx=fidx.ptr, ip_id0=ID0, ip_off=IP_OFF,
                         raw_out=raw.ptr, desc_out=desc.ptr, cls_out=co.ptr, count=cnt.ptr)

        def leg_b(m=n):
            eng.l4_build(buf.ptr, m, slot.ptr, seg.ptr, fl.ptr, NFLOW, cls=cls.ptr, fidx=fidx.ptr, ip_id0=ID0, ip_off=IP_OFF)

        def pinned(fn, shape):
            """timed(fn) with the store shape pinned around the whole of it."""
            def run(eng_, launch):
                cgck.l4_build_store(shape)
                try:
                    return timed(eng_, launch)
                finally:
                    cgck.l4_build_store(cgck.L4B_STORE_DEFAULT)
            return fn, run

        def leg_c(m=n):
            eng.l4_desc(buf.ptr, desc.ptr, m, seg=sg.ptr)

        def leg_d(m=n):
            eng.rss_desc(buf.ptr, desc.ptr, m, spec, hash=hsh.ptr)

        def frames_miss():
            if not args.packed:
                got = fetch(eng, buf, ks, np.dtype((np.uint8, 128)), STRIDE)
                return int(np.count_nonzero(got != want_frames))
            bad = 0
            for i in range(len(ks)):                        # the frame's own bytes: its neighbours own the rest
                got = np.zeros(int(want_raw["ip_len"][i]), np.uint8)
                buf.download(got, off=int(sslot["frame_off"][i]), stream=eng.stream)
                eng.sync()
                bad += int(np.count_nonzero(got != want_frames[i][:len(got)]))
            return bad

        for rnd in (0, 1):
            for leg, (fn, clock) in zip(LEGS, (pinned(leg_a, cgck.L4B_STORE_DIRECT), pinned(leg_b, cgck.L4B_STORE_DIRECT),
                                               pinned(leg_a, cgck.L4B_STORE_TURNED), pinned(leg_b, cgck.L4B_STORE_TURNED),
                                               (leg_c, timed), (leg_d, timed))):
                for i, k in enumerate(ks):                  # what this leg writes of the sampled frames is written anew
                    if leg in BUILD_ALL + BUILD_FRAMES:
                        buf.upload(np.full(int(want_raw["ip_len"][i]) if args.packed else 128, 0xEE, np.uint8),
                                   off=int(sslot["frame_off"][i]), stream=eng.stream)
                    if leg in BUILD_ALL:
                        raw.upload(np.full(12, 0xEE, np.uint8), off=12 * int(k), stream=eng.stream)
                        desc.upload(np.full(12, 0xEE, np.uint8), off=12 * int(k), stream=eng.stream)
                        co.upload(np.full(1, 0xEE, np.uint8), off=int(k), stream=eng.stream)
                    if leg == "c_l4_desc_seg":
                        sg.upload(np.full(32, 0xEE, np.uint8), off=32 * int(k), stream=eng.stream)
                    if leg == "d_rss_desc":
                        hsh.upload(np.full(4, 0xEE, np.uint8), off=4 * int(k), stream=eng.stream)
                cnt.upload(np.zeros(l4bref.NCOUNT, np.uint32), stream=eng.stream)
                med, lo, hi = clock(eng, fn)
                kern = eng.last_kernel
                miss = 0
                if leg in BUILD_ALL + BUILD_FRAMES:
                    miss += frames_miss()
                if leg in BUILD_ALL:
                    gn = np.zeros(l4bref.NCOUNT, np.uint32)
                    cnt.download(gn, stream=eng.stream)
                    eng.sync()
                    miss += int(np.count_nonzero(fetch(eng, raw, ks, l4bref.DESC_DTYPE) != want_raw))
                    miss += int(np.count_nonzero(fetch(eng, desc, ks, l4bref.DESC_DTYPE) != want_desc))
                    miss += int(np.count_nonzero(fetch(eng, co, ks, np.uint8) != want_cls))
                    # 25 calls (5 warm-ups, 20 timed), every frame built; two frames in five are IPv6
                    miss += int(int(gn[:2].sum()) != 25 * n) + int(int(gn[2:6].sum()) != 0) + int(int(gn[7]) != 0)
                    miss += int(int(gn[6]) != 25 * int(np.count_nonzero((np.arange(n, dtype=np.int64) % NFLOW) % 5 < 2)))
                if leg == "c_l4_desc_seg":
                    miss += int(np.count_nonzero(fetch(eng, sg, ks, l4ref.SEG_DTYPE) != want_seg))
                if leg == "d_rss_desc":
                    miss += int(np.count_nonzero(fetch(eng, hsh, ks, np.uint32) != want_hash))
                r = {"alloc": alloc, "leg": leg, "round": rnd, "packets": n, "ms_median": round(med, 4),
                     "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes_counted": moved[leg],
                     "pct_hbm_peak": round(100 * moved[leg] / (med * 1e-3) / HBM_PEAK, 1), "kernel": kern,
                     "referee_mismatches": miss, "sampled": len(ks)}
                if leg in BUILD_ALL:
                    r["classes_per_call"] = {l4bref.NAMES[c]: int(gn[c]) // 25 for c in range(l4bref.NCLASS)}
                rows.append(r)
                emit(json.dumps(r))
        if args.small and alloc == 0:
            for m in (256, 4096):
                for leg, (fn, clock) in (("a_build_all", pinned(leg_a, cgck.L4B_STORE_DIRECT)),
                                         ("at_build_all_turned", pinned(leg_a, cgck.L4B_STORE_TURNED)),
                                         ("c_l4_desc_seg", (leg_c, timed)), ("d_rss_desc", (leg_d, timed))):
                    med, lo, hi = clock(eng, lambda: fn(m))
                    small.append({"leg": leg, "packets": m, "us_median": round(1e3 * med, 2), "us_min": round(1e3 * lo, 2),
                                  "us_max": round(1e3 * hi, 2), "kernel": eng.last_kernel})
                    emit(json.dumps(small[-1]))
    for b in held:
        b.free()
    eng.close()

    def med_of(leg, alloc=None):
        return statistics.median(r["ms_median"] for r in rows if r["leg"] == leg and alloc in (None, r["alloc"]))

    emit("")
    emit(f"header bytes written per frame (mean of the sample): {hdr:.1f}")
    emit(f"{'leg':23} " + " ".join(f"a{a}r{r} ms" for a in (0, 1) for r in (0, 1))
         + "   median  margin %   MB counted  % of 8 TB/s  kernel")
    for leg in LEGS:
        sel = [r for r in rows if r["leg"] == leg]
        med, m0, m1 = med_of(leg), med_of(leg, 0), med_of(leg, 1)
        emit(f"{leg:23} " + " ".join(f"{r['ms_median']:8.4f}" for r in sel)
             + f"  {med:7.4f}  {100 * abs(m0 - m1) / min(m0, m1):8.2f}  {moved[leg] / 1e6:10.1f}"
             + f"  {100 * moved[leg] / (med * 1e-3) / HBM_PEAK:11.1f}  {sel[0]['kernel']}")
    a, b, at, bt, c, d = (med_of(leg) for leg in LEGS)
    emit(f"a / c = {a / c:.3f}, b / c = {b / c:.3f}, at / c = {at / c:.3f}, bt / c = {bt / c:.3f}, at / a = {at / a:.3f}, "
         f"bt / b = {bt / b:.3f}, c / d = {c / d:.3f}; each leg's margin is its spread between the "
         f"two allocations")
    if small:
        emit("small bursts, microseconds per call (median of 20): "
             + ", ".join(f"{s['leg']} at {s['packets']}: {s['us_median']}" for s in small))
    emit(f"referee mismatches over all legs: {sum(r['referee_mismatches'] for r in rows)}")
    emit("not measured: frames with payload followed by the streamed fill, bursts packed back to back, a burst whose "
         "flow table exceeds the caches")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
