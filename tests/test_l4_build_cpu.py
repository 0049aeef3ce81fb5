"""CPU tests of cgck_l4_build's test infrastructure and host side (no GPU): the
referee (tests/l4bref.py) builds the frames the reference stack's replay builds
(oracle/stack_replay.c: tcp_respond + ip_output), its frames read back through the
referees of cgck_l2_desc and cgck_l4_desc to the records that went in and carry
sums that verify, the corpus reaches what the contract names, and the binding's
constants, layouts and cgck_l4_build_hdr_bytes are the header's.

The first five tests pin the referee and the corpus to the reference and to the
existing referees; they do not call the library and pass without the feature.  The
library's host side is covered by the last three (constants and exports,
cgck_l4_build_hdr_bytes, the argument checks), which fail without it; the kernel is
covered by tests/test_gpu_l4_build.py."""
import ctypes
import os
import re

import numpy as np

import cgck
import l2ref
import l4bbatches as LB
import l4bref as R
import l4ref
import mixedref
import refcases
import rxcorpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
ETH_DST, ETH_SRC = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2)      # ip_output.c:65-67 as the replay writes them


def replay_flow(src, dst):
    """The flow of a frame the replay sends from src to dst (4 wire bytes each)."""
    f = np.zeros(1, R.FLOW_DTYPE)
    f["eth_dst"], f["eth_src"], f["ttl"] = ETH_DST, ETH_SRC, 64
    f["laddr"][0, :4], f["faddr"][0, :4] = src, dst
    return f[0]


def tx_ring(n, slot):
    desc = np.zeros(n, R.DESC_DTYPE)
    desc["frame_off"] = np.arange(n) * slot
    desc["ip_len"] = slot
    return np.full(n * slot, POISON, np.uint8), desc


# -- 1, 2. the referee against the reference's transmit path ------------------------------

def test_keepalives_against_reference_replay(port):
    """check_timers' keepalive probes (tcp_timer.c:214 -> tcp_respond, tcp_subr.c:52-123
    -> ip_output) as the oracle replays them, against the referee's frames from the
    equivalent records, byte for byte, with an ip_id that wraps."""
    n, slot, id0 = 37, 128, 0xFFF0
    ka = refcases.keepalives(np.random.default_rng(91), n)
    fns = port.fn_pointers()
    tx, desc = tx_ring(n, slot)
    local = np.zeros(2048, np.uint8)
    _, _, txs, idn = port.replay_rx_rsp(fns[0], fns[1], np.zeros(16, np.uint8), np.zeros(12, np.uint8), 0, 1, 1,
                                        tx, slot, n, local, rxcorpus.LADDR, ka, id0)
    assert txs.tolist() == [n, 0, 0, 0, 0, n] and idn == (id0 + n) & 0xFFFF and idn < id0
    raw = ka.view(np.uint8).reshape(n, -1)
    flow = np.array([replay_flow(raw[k, 0:4], raw[k, 4:8]) for k in range(n)], R.FLOW_DTYPE)
    seg = np.zeros(n, R.SEG_DTYPE)
    seg["sport"], seg["dport"] = ka["lport"], ka["fport"]
    seg["seq"], seg["ack"], seg["th_flags"] = ka["snd_una"] - np.uint32(1), ka["rcv_nxt"], 0x10
    seg["win"] = (ka["hiwat"] >> ka["scale"]) & 0xFFFF
    seg["l4_off"], seg["hdr_len"] = 0x7777, 0x77        # ignored
    mine, _ = tx_ring(n, slot)
    raw_out, desc_out, cls, count = R.build(mine, desc, seg, flow, ip_id0=id0, ip_off=0x4000)
    assert np.all(cls == R.TCP) and count.tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
    assert np.all(raw_out["ip_len"] == 54) and np.all(desc_out["l3_off"] == 14) and np.all(desc_out["ip_len"] == 40)
    assert np.array_equal(mine, tx)
    assert np.all(tx.reshape(n, slot)[:, 54:] == POISON) and not np.any(np.all(tx.reshape(n, slot)[:, :54] == POISON, axis=1))


def test_rsts_against_reference_replay(port):
    """The RSTs tcp_input sends for segments to closed ports (tcp_input.c:881-899):
    the records follow from l4ref's records of the received frames by tcp_respond's
    rules (tcp_subr.c:104-115)."""
    rng = np.random.default_rng(92)
    frames = []
    for k in range(48):
        off = (5, 5, 6, 8, 15)[k % 5]
        flags = (0x02, 0x10, 0x12, 0x18, 0x11, 0x00, 0x01, 0x03, 0x04, 0x14)[k % 10]
        dst = rxcorpus.LADDR[0] + k % 4

        def pre(p, hl, dst=dst, flags=flags):
            p[16:20] = [(dst >> s) & 255 for s in (24, 16, 8, 0)]
            p[hl + 13] = flags
        frames.append(rxcorpus.frame(rng, port, 6, 4 * off + (0, 1, 333)[k % 3], ihl=(5, 5, 7)[k % 3], tcp_off=off, pre=pre))
    n, slot, id0 = len(frames), 128, 0xFFE0
    buf, rx = rxcorpus.ring(frames)
    seg_in, cls_in, _, _ = l4ref.expect(buf, rx)
    assert np.all(cls_in == l4ref.TCP)
    fns = port.fn_pointers()
    tx, desc = tx_ring(n, slot)
    res, _, txs, idn = port.replay_rx_rsp(fns[0], fns[1], buf.copy(), rx.view(np.uint8), n, 1, 1, tx, slot, n,
                                          np.zeros(2048, np.uint8), rxcorpus.LADDR, None, id0)
    assert np.all(res == port.R_ACCEPT) and txs.tolist() == [n, 0, n, 0, 0, 0] and idn < id0
    seg = np.zeros(n, R.SEG_DTYPE)
    flow = np.zeros(n, R.FLOW_DTYPE)
    for k, p in enumerate(frames):
        r = seg_in[k]
        flow[k] = replay_flow(p[16:20], p[12:16])                       # :104-107 the addresses swapped
        seg[k]["sport"], seg[k]["dport"] = r["dport"], r["sport"]       # :108-110 the ports swapped
        if int(r["th_flags"]) & 0x10:                                   # tcp_input.c:891-892
            seg[k]["seq"], seg[k]["th_flags"] = r["ack"], 0x04
        else:                                                           # :893-897
            tlen = int(r["pay_len"]) + bool(int(r["th_flags"]) & 0x02)
            seg[k]["ack"], seg[k]["th_flags"] = (int(r["seq"]) + tlen) & 0xFFFFFFFF, 0x14
    mine, _ = tx_ring(n, slot)
    R.build(mine, desc, seg, flow, ip_id0=id0, ip_off=0x4000)
    assert np.array_equal(mine, tx)
    assert np.all(tx.reshape(n, slot)[:, 54:] == POISON)


# -- 3, 4. the corpus through the existing referees ---------------------------------------

def source_word(fl):
    """F of cgck_l4_desc's hash for a frame of this flow: the source address."""
    w = fl["laddr"].view("<u4")
    return int(w[0] ^ w[1] ^ w[2] ^ w[3]) if int(fl["flags"]) & R.FLOW_IP6 else int(w[0])


def test_corpus_covers_and_round_trips():
    C = LB.Corpus(np.random.default_rng(31))
    assert C.m < 200
    buf, slot = LB.lay(C, 7)
    before = buf.copy()
    raw, desc, cls, count = R.build(buf, slot, C.seg, C.flow, C.cls, C.fidx, 0xFFC0, 0x4000)
    # every class; the family flag beside every class that can carry it; PAYLOAD beside both built ones
    want = {c | f for c in (R.TCP, R.UDP, R.BADSEG, R.NOROOM) for f in (0, R.IP6)} | {R.SKIP, R.BADFLOW}
    want |= {c | f | R.PAYLOAD for c in (R.TCP, R.UDP) for f in (0, R.IP6)}
    assert {int(c) for c in cls} == want
    assert np.array_equal(count, R.counts(cls)) and int(count[:R.NCLASS].sum()) == C.m and np.all(count > 0)
    built = (cls & 15) <= R.UDP
    flags = np.array([int(C.flow["flags"][f]) if f < LB.NFLOW else 0 for f in C.fidx])
    for f in LB.GOOD:                                   # each option subset built under every flow shape
        sel = built & (C.fidx == f) & (C.cls & 15 == R.SEG_TCP)
        assert {int(o) for o in C.seg["opt"][sel]} == set(range(8))
        for capd, b in ((-1, False), (0, True), (1, True)):            # cap at L - 1, L, L + 1
            at = [i for i in range(C.m) if C.capd[i] == capd and C.capd[i] is not None and int(C.fidx[i]) == f
                  and not isinstance(C.capd[i], tuple) and C.L(i)[0]]
            assert len(at) >= 3 and all(bool(built[i]) == b for i in at), (f, capd)
    assert int(raw["ip_len"][built].max()) == 18 + 40 + 20 + 1400
    v4 = built & ((cls & R.IP6) == 0)
    ids = (buf[(desc["frame_off"] + desc["l3_off"])[v4].astype(np.int64) + 4].astype(int) << 8) | \
        buf[(desc["frame_off"] + desc["l3_off"])[v4].astype(np.int64) + 5]
    assert ids.tolist() == [(0xFFC0 + k) & 0xFFFF for k in np.nonzero(v4)[0]] and ids.min() < 0x40 < 0xFFC0 < ids.max()
    # nothing but the headers changed, and a frame that is not built changed nothing
    changed = np.nonzero(buf != before)[0]
    own = np.zeros(len(buf), bool)
    for k in np.nonzero(built)[0]:
        o = int(slot["frame_off"][k]) + int(slot["l3_off"][k])
        own[o:o + int(raw["ip_len"][k]) - int(C.seg["pay_len"][k])] = True
    assert np.all(own[changed])
    assert np.all(raw["ip_len"][~built] == 0) and np.all(desc["ip_len"][~built] == 0)
    assert np.array_equal(raw["l3_off"], slot["l3_off"]) and np.array_equal(desc["l3_off"][~built], slot["l3_off"][~built])
    assert np.array_equal(raw["frame_off"], slot["frame_off"]) and np.array_equal(desc["frame_off"], slot["frame_off"])

    # through cgck_l2_desc's referee: the trimmed descriptors are desc_out
    d2, c2, _ = l2ref.expect(buf, raw[built])
    assert np.array_equal(d2, desc[built])
    fb = flags[built]
    assert np.array_equal(c2 & 15, np.where(fb & R.FLOW_IP6, l2ref.IP6, l2ref.IP4))
    assert np.array_equal((c2 & l2ref.VLAN) != 0, (fb & R.FLOW_VLAN) != 0)
    # through cgck_l4_desc's referee: the records that went in
    seg, c4, hsh, _ = l4ref.expect(buf, desc)
    assert np.all(c4[~built] == l4ref.NONE)
    for k in np.nonzero(built)[0]:
        s, g, fl = C.seg[k], seg[k], C.flow[int(C.fidx[k])]
        tcp = int(C.cls[k]) & 15 == R.SEG_TCP
        h, iph, l4h = R.lengths(int(fl["flags"]), int(C.cls[k]) & 15, int(s["opt"]))
        assert int(c4[k]) == (l4ref.TCP if tcp else l4ref.UDP) | (l4ref.IP6 if iph == 40 else 0), k
        assert (int(g["l4_off"]), int(g["hdr_len"]), int(g["pay_len"])) == (iph, l4h, int(s["pay_len"])), k
        assert (int(g["sport"]), int(g["dport"])) == (int(s["sport"]), int(s["dport"])), k
        assert int(hsh[k]) == l4ref.so_hash(source_word(fl), int(s["dport"]), int(s["sport"])), k
        if not tcp:
            assert all(int(g[x]) == 0 for x in ("seq", "ack", "win", "th_flags", "opt", "mss", "wscale", "ts_val", "ts_ecr"))
            continue
        assert all(int(g[x]) == int(s[x]) for x in ("seq", "ack", "win", "th_flags", "opt")), k
        opt = int(s["opt"])
        assert not opt & 3 or int(s["th_flags"]) & 0x02                 # MSS / WS are read back on SYN records only
        assert int(g["mss"]) == (int(s["mss"]) if opt & R.MSS else 0), k
        assert int(g["wscale"]) == (int(s["wscale"]) if opt & R.WS else 0), k
        assert (int(g["ts_val"]), int(g["ts_ecr"])) == ((int(s["ts_val"]), int(s["ts_ecr"])) if opt & R.TS else (0, 0)), k


def test_built_frames_verify(port):
    """Header-only frames carry final sums; a frame with payload has a zero L4 field
    and verifies after the fill the contract names."""
    C = LB.Corpus(np.random.default_rng(32))
    buf, slot = LB.lay(C, 2)
    raw, desc, cls, _ = R.build(buf, slot, C.seg, C.flow, C.cls, C.fidx, 9, 0)
    built = (cls & 15) <= R.UDP
    paid = built & ((cls & R.PAYLOAD) != 0)
    assert np.count_nonzero(paid) >= 16 and np.count_nonzero(built & ~paid) >= 60
    offs, lens = desc["frame_off"].astype(np.int64) + desc["l3_off"], desc["ip_len"].astype(np.int64)
    flags = mixedref.IP | mixedref.L4 | mixedref.VERIFY
    _, ver = mixedref.expect(port, buf, offs[built & ~paid], lens[built & ~paid], flags)
    assert not np.any(ver)
    for k in np.nonzero(paid)[0]:
        iph = 40 if cls[k] & R.IP6 else 20
        at = int(offs[k]) + iph + (16 if cls[k] & 15 == R.TCP else 6)
        assert buf[at] == 0 and buf[at + 1] == 0
    _, ver = mixedref.expect(port, buf, offs[paid], lens[paid], flags)
    assert np.all(ver & mixedref.BAD_L4) and not np.any(ver & mixedref.BAD_IP)        # random payload: a zero field is wrong
    R.fill(buf, desc, cls)
    _, ver = mixedref.expect(port, buf, offs[built], lens[built], flags)
    assert not np.any(ver)


def test_layouts():
    C = LB.Corpus(np.random.default_rng(33))
    for align in (0, 9):
        buf, slot = LB.lay(C, align)
        o = slot["frame_off"].astype(np.int64) + slot["l3_off"]
        assert np.all((o & 15) == align) and np.all(buf[slot["frame_off"].astype(np.int64) - 1] == LB.POISON)
        assert int(o[-1]) + int(slot["ip_len"][-1]) == len(buf)
    buf, slot, cls, fidx, seg = LB.packed(C, 3)
    o = slot["frame_off"].astype(np.int64)
    assert o[0] == 3 and np.array_equal(o[1:], (o + slot["ip_len"])[:-1]) and len(slot) > 200
    # every header is 2 mod 4 bytes long: an odd start gives every odd alignment, an even one every even
    assert set((o & 15).tolist()) == set(range(1, 16, 2))
    assert set((LB.packed(C, 6)[1]["frame_off"].astype(np.int64) & 15).tolist()) == set(range(0, 16, 2))
    raw, desc, out, _ = R.build(buf, slot, seg, C.flow, cls, fidx)
    assert np.all((out & 15) <= R.UDP) and np.array_equal(raw["ip_len"], slot["ip_len"])
    assert np.all(buf[:3] == LB.POISON) and np.all(buf[-13:] == LB.POISON) and np.count_nonzero(buf[3:-13] == LB.POISON) < len(buf) // 50
    # the ids of a later call, restated over arrays for the piecewise comparison of a long burst
    b0, slot, cls, fidx, seg = LB.tiled(C, 700)
    b1 = b0.copy()
    _, d0, c0, _ = R.build(b0, slot, seg, C.flow, cls, fidx, 0, 0x4000)
    R.build(b1, slot, seg, C.flow, cls, fidx, 0xFF00, 0x4000)
    assert not np.array_equal(b0, b1) and np.array_equal(LB.with_ids(b0, d0, c0, 0xFF00), b1)


# -- 5, 6. the binding against the header ------------------------------------------------

def test_constants_layouts_and_exports():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    for i, x in enumerate(R.NAMES + ("NCLASS",)):
        m = re.search(rf"\bCGCK_BLD_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == i == getattr(cgck, f"BLD_{x}"), x
        if x != "NCLASS":
            assert getattr(R, x) == i
    for x, v in (("IP6", 16), ("PAYLOAD", 32)):
        m = re.search(rf"\bCGCK_BLD_{x} = 1u << (\d+)", hdr)
        assert m and 1 << int(m.group(1)) == v == getattr(cgck, f"BLD_{x}") == getattr(R, x), x
    for x, v in (("IP6", 1), ("VLAN", 2)):
        m = re.search(rf"\bCGCK_FLOW_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == v == getattr(cgck, f"FLOW_{x}") == getattr(R, f"FLOW_{x}"), x
    m = re.search(r"#define CGCK_BLD_NCOUNT (\d+)", hdr)
    assert m and int(m.group(1)) == cgck.BLD_NCOUNT == R.NCOUNT == 8
    assert (R.SEG_TCP, R.SEG_UDP, R.MSS, R.WS, R.TS, R.OPT_BAD) == \
        (cgck.SEG_TCP, cgck.SEG_UDP, cgck.SEG_MSS, cgck.SEG_WS, cgck.SEG_TS, cgck.SEG_OPT_BAD)
    # sizeof(cgck_flow_t) == 48 == FLOW_DTYPE.itemsize, field by field as the header declares them
    body = re.search(r"typedef struct cgck_flow \{(.*?)\} cgck_flow_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    off, names = 0, []
    for typ, ids in re.findall(r"(uint\d+_t)\s+([a-z_0-9, \[\]]+);", body):
        for name in ids.split(","):
            name, cnt = re.fullmatch(r"\s*([a-z_0-9]+)(?:\[(\d+)\])?\s*", name).groups()
            cnt = int(cnt or 1)
            assert off % size[typ] == 0
            dt, at = cgck.FLOW_DTYPE.fields[name][:2]
            assert at == off and dt.itemsize == size[typ] * cnt and dt.base.itemsize == size[typ], name
            names.append(name)
            off += size[typ] * cnt
    assert off == 48 == cgck.FLOW_DTYPE.itemsize == R.FLOW_DTYPE.itemsize
    assert tuple(names) == cgck.FLOW_DTYPE.names == R.FLOW_DTYPE.names
    assert cgck.SEG_DTYPE == R.SEG_DTYPE and cgck.DESC_DTYPE.itemsize == R.DESC_DTYPE.itemsize == 12
    # the two argument structs as the header declares them
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(cgck.L4BuildRes) == 4 * vp and ctypes.sizeof(cgck.L4BuildIn) == 5 * vp + 8
    body = re.search(r"typedef struct cgck_l4_build_in \{(.*?)\} cgck_l4_build_in_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+);", body) == [f[0] for f in cgck.L4BuildIn._fields_]
    assert (cgck.L4BuildIn.nflow.offset, cgck.L4BuildIn.ip_id0.offset, cgck.L4BuildIn.ip_off.offset) == (5 * vp, 5 * vp + 4, 5 * vp + 6)
    body = re.search(r"typedef struct cgck_l4_build_res \{(.*?)\} cgck_l4_build_res_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+);", body) == [f[0] for f in cgck.L4BuildRes._fields_]
    L = cgck.load()
    for name in ("cgck_l4_build", "cgck_l4_build_hdr_bytes", "cgck_test_l4_build_pass", "cgck_test_l4_build_store"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert "#define CGCK_ABI_VERSION 2" in hdr and L.cgck_abi_version() == 2


def test_hdr_bytes_every_argument():
    """cgck_l4_build_hdr_bytes over all 4 x 16 x 256 arguments against the referee's
    lengths, and its extremes by hand."""
    assert cgck.l4_build_hdr_bytes(0, R.SEG_UDP, 0) == 42 and cgck.l4_build_hdr_bytes(3, R.SEG_TCP, 7) == 98
    assert cgck.l4_build_hdr_bytes(0, R.SEG_TCP, 0) == 54 and cgck.l4_build_hdr_bytes(0, R.SEG_TCP, R.OPT_BAD) == 0
    assert cgck.l4_build_hdr_bytes(0, 2, 0) == 0 and cgck.l4_build_hdr_bytes(1, R.SEG_UDP, 0xFF) == 62
    L = cgck.load()
    n = 0
    for ff in range(4):
        for c in range(16):
            for opt in range(256):
                got, want = L.cgck_l4_build_hdr_bytes(ff, c, opt), R.hdr_bytes(ff, c, opt)
                assert got == want, (ff, c, opt, got, want)
                n += want > 0
    assert n == 4 * (8 + 256)
    assert L.cgck_l4_build_hdr_bytes(4, 0, 0) == 0 and L.cgck_l4_build_hdr_bytes(3, 0x10, 4) == 18 + 40 + 32


def test_arguments_without_device():
    """The argument checks come before any device work."""
    L = cgck.load()
    arg = cgck.L4BuildIn()
    assert L.cgck_l4_build(None, 16, 0, ctypes.byref(arg), None, None) == -22
    assert L.cgck_test_l4_build_pass(None, None) == -22
    # the store-shape pin: returns the previous value, refuses anything but 0, 1, 2
    assert L.cgck_test_l4_build_store(3) == -22 and L.cgck_test_l4_build_store(-1) == -22
    assert cgck.l4_build_store(cgck.L4B_STORE_TURNED) == cgck.L4B_STORE_DEFAULT
    assert cgck.l4_build_store(cgck.L4B_STORE_DIRECT) == cgck.L4B_STORE_TURNED
    assert cgck.l4_build_store(cgck.L4B_STORE_DEFAULT) == cgck.L4B_STORE_DIRECT
