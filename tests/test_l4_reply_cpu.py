"""CPU tests of cgck_l4_reply's rule, referee and host side (no GPU).

cgck_l4_reply_rule, the text l4r_kernel compiles, runs over every corpus frame
under every (vmask, flags) pair and is compared with the referee (tests/l4rref.py);
the referee's chain (l4ref, a table-less lookup, l4rref packed, l4bref) is compared
with the reference stack's replay (oracle/stack_replay.c: tcp_input without a PCB,
tcp_respond, ip_output), transmit ring against transmit ring; and the binding's
constants and layouts are the header's.

The replay test pins the referee to the reference and passes without the feature;
the others call the library and fail without it.  The kernel is covered by
tests/test_gpu_l4_reply.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import cgck
import l4bref
import l4rbatches as LB
import l4ref
import l4rref as R
import mixedref
import pcbref
import rxcorpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5


@pytest.fixture(scope="module")
def corpus():
    return LB.corpus()


def rule(b, k, vm, flags, drop=()):
    """cgck_l4_reply_rule for corpus frame k; a selector in `drop` takes the value a
    NULL array stands for."""
    sel = {"cls": int(b.cls[k]), "kind": int(b.kind[k]), "verdict": int(b.verdict[k]), "l2cls": int(b.l2cls[k])}
    sel.update({x: {"cls": cgck.SEG_TCP, "kind": cgck.PCB_MISS, "verdict": 0, "l2cls": 0}[x] for x in drop})
    return cgck.l4_reply_rule(b.seg[k], R.frame_bytes(b.buf, b.desc, k).copy(), LB.LINK, vmask=vm, flags=flags, **sel)


def same_record(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, got, want)


# -- 1. the rule against the referee -------------------------------------------------------

def test_corpus_reaches_what_the_contract_names(corpus):
    b = corpus
    n = len(b.desc)
    seen = set()
    for vm, flags in LB.CONFIGS:
        seen |= {int(c) for c in R.per_frame(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, **b.sel())[0]}
    # every class in both families (the class values are 0 and 2..6: 1 is cgck_l4_build's UDP and no class here)
    assert seen == {c | f for c in R.CLASSES for f in (0, R.IP6)} and len(R.CLASSES) == 6 and R.NCLASS == 7
    plain = [k for k in range(n) if b.tags[k].startswith(("flags", "wrap", "options", "max"))]
    th, pay = b.seg["th_flags"][plain], b.seg["pay_len"][plain]
    assert np.any(th & 0x10) and np.any((th & 0x10) == 0) and np.any(th & 0x02) and np.any(th & 0x04)
    assert np.any(pay > 0) and np.any(pay == 0)
    big = b.tags.index("max payload")
    assert int(b.seg["pay_len"][big]) == 65495 and int(b.seg["th_flags"][big]) & 0x02 and int(b.desc["ip_len"][big]) == 65535
    wraps = [k for k in plain if not int(b.seg["th_flags"][k]) & 0x10
             and int(b.seg["seq"][k]) + int(b.seg["pay_len"][k]) + bool(int(b.seg["th_flags"][k]) & 2) >= 2 ** 32]
    assert len(wraps) >= 4 and any(R.one(b.seg[k], None, None, None, 0, None, 0, R.frame_bytes(b.buf, b.desc, k), LB.LINK)[1]["ack"] == 0
                                   for k in wraps)
    opt4 = [k for k in range(n) if b.tags[k].startswith("options") and int(b.seg["l4_off"][k]) == 28]
    opt6 = [k for k in range(n) if b.tags[k].startswith("options") and int(b.seg["l4_off"][k]) == 56]
    assert len(opt4) == 2 and len(opt6) == 2 and all(int(b.seg["hdr_len"][k]) == 24 for k in opt4 + opt6)
    # multicast by the L2 bits, by a class-D destination and by ff00::/8, each quiet only under NO_MCAST
    for tag in ("l2 mcast", "l2 bcast", "mcast dst"):
        for six in (False, True):
            k = [i for i in range(n) if b.tags[i] == tag and bool(int(b.l2cls[i]) & 1) == six][0]
            fb = R.frame_bytes(b.buf, b.desc, k)
            args = (b.seg[k], b.cls[k], b.kind[k], b.verdict[k], 0, b.l2cls[k])
            assert R.classify(*args, R.NO_MCAST, fb) == R.QUIET and R.classify(*args, R.NO_RST, fb) == R.RST
    assert {f for _, f in LB.CONFIGS} == {0, R.NO_RST, R.NO_MCAST, R.NO_RST | R.NO_MCAST}
    assert {7, 4} <= {v for v, _ in LB.CONFIGS}
    assert set((b.desc["frame_off"].astype(np.int64) + b.desc["l3_off"]) % 16) == set(range(16))


@pytest.mark.parametrize("vm,flags", LB.CONFIGS)
def test_rule_against_referee(corpus, vm, flags):
    b = corpus
    want = R.per_frame(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, **b.sel())
    for k in range(len(b.desc)):
        c, r, f = rule(b, k, vm, flags)
        assert c == int(want[0][k]), (k, b.tags[k], c, int(want[0][k]))
        same_record(r, want[1][k], (k, b.tags[k], "seg"))
        same_record(f, want[2][k], (k, b.tags[k], "flow"))
        if c & 15 != R.RST:
            assert not np.any(r.tobytes()) and not any(f.tobytes())


@pytest.mark.parametrize("drop", ["cls", "kind", "verdict", "l2cls"])
def test_rule_with_a_selector_absent(corpus, drop):
    """The value a NULL selector array stands for, against the referee's None."""
    b = corpus
    vm, flags = 7, R.NO_RST | R.NO_MCAST
    want = R.per_frame(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, **b.sel(drop=(drop,)))
    full = R.per_frame(b.buf, b.desc, b.seg, LB.LINK, vm=vm, flags=flags, **b.sel())
    assert not np.array_equal(want[0], full[0])         # the selector mattered
    for k in range(len(b.desc)):
        c, r, f = rule(b, k, vm, flags, drop=(drop,))
        assert c == int(want[0][k]), (k, b.tags[k])
        same_record(r, want[1][k], (k, "seg"))
        same_record(f, want[2][k], (k, "flow"))


def test_rule_reads_no_byte_past_ip_len(corpus):
    """Bytes at and past ip_len are not the frame's: two copies that differ there agree."""
    b = corpus
    for k in range(len(b.desc)):
        n = int(b.desc["ip_len"][k])
        if n >= 48:
            continue
        pad = np.zeros(64, np.uint8)
        pad[:n] = R.frame_bytes(b.buf, b.desc, k)
        alt = pad.copy()
        alt[n:] = 0xFF
        got = [cgck.l4_reply_rule(b.seg[k], x, LB.LINK, cls=int(b.cls[k]), kind=int(b.kind[k]), flags=3, ip_len=n)
               for x in (pad, alt)]
        assert got[0][0] == got[1][0] and got[0][1].tobytes() == got[1][1].tobytes() and got[0][2].tobytes() == got[1][2].tobytes()


def test_rule_arguments():
    L = cgck.load()
    s, r, f = np.zeros(1, cgck.SEG_DTYPE), np.zeros(1, cgck.SEG_DTYPE), np.zeros(1, cgck.FLOW_DTYPE)
    ip = np.zeros(40, np.uint8)
    lk = cgck.Flow.of(LB.LINK)

    def rc(s=s.ctypes.data, ip=ip.ctypes.data, n=40, lk=lk, r=r.ctypes.data, f=f.ctypes.data, flags=0):
        return L.cgck_l4_reply_rule(s, 0, 2, 0, 0, 0, flags, ip, n, None if lk is None else ctypes.byref(lk), r, f)

    bad = cgck.Flow.of(LB.LINK)
    bad.flags = 4
    for what, got in (("NULL s", rc(s=None)), ("NULL ip", rc(ip=None)), ("NULL link", rc(lk=None)), ("NULL r", rc(r=None)),
                      ("NULL f", rc(f=None)), ("flags", rc(flags=4)), ("link.flags", rc(lk=bad))):
        assert got == -22, (what, got)
    assert rc(ip=None, n=0) == R.NONE_ and rc() == R.NONE_             # version 0


# -- 2. the referee against the reference's own behaviour ---------------------------------

def tx_ring(n, slot):
    desc = np.zeros(n, l4bref.DESC_DTYPE)
    desc["frame_off"] = np.arange(n) * slot
    desc["ip_len"] = slot
    return np.full(n * slot, POISON, np.uint8), desc


def referee_chain(port, buf, rx, ip_in, tcp_in, id0, slot):
    """l4ref, a table-less lookup, l4rref packed, l4bref: (transmit ring, R)."""
    n = len(rx)
    seg, cls, _, _ = l4ref.expect(buf, rx)
    offs, lens = rx["frame_off"].astype(np.int64) + rx["l3_off"], rx["ip_len"].astype(np.int64)
    _, ver = mixedref.expect(port, buf, offs, lens, mixedref.IP | mixedref.L4 | mixedref.VERIFY | mixedref.V_IP_ZERO_IS_FFFF)
    _, _, kind, _ = pcbref.lookup(buf, rx, seg, cls, np.zeros(0, pcbref.CONN_DTYPE), np.zeros(0, l4bref.FLOW_DTYPE))
    link = np.zeros(1, R.FLOW_DTYPE)[0]
    link["eth_dst"], link["eth_src"], link["ttl"] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2), 64     # the replay's (ip_output.c:65-68)
    p = R.packed(buf, rx, seg, link, cls=cls, kind=kind, verdict=ver, vm=R.vmask(ip_in, tcp_in))
    ring, txd = tx_ring(n, slot)
    _, _, bcls, _ = l4bref.build(ring, txd, p["seg"], p["flow"], p["cls"], None, id0, 0x4000)
    nrst = int(p["qoff"][1])
    assert np.all(bcls[:nrst] == l4bref.TCP) and np.all(bcls[nrst:] == l4bref.SKIP)
    return ring, nrst, ver, cls


@pytest.mark.parametrize("ip_in,tcp_in", [(2, 2), (1, 1), (0, 0)])
def test_referee_chain_against_reference_replay(port, ip_in, tcp_in):
    frames = LB.replay_frames(np.random.default_rng(93), port)
    kinds = [k for k, _ in frames]
    assert {"good", "bad ip", "bad l4", "both", "short", "bad off", "off long"} == set(kinds)
    n, slot, id0 = len(frames), 128, 0xFFE8
    buf, rx = rxcorpus.ring([p for _, p in frames])
    fns = port.fn_pointers()
    tx, _ = tx_ring(n, slot)
    res, _, txs, idn = port.replay_rx_rsp(fns[0], fns[1], buf.copy(), rx.view(np.uint8), n, ip_in, tcp_in, tx, slot, n,
                                          np.zeros(2048, np.uint8), rxcorpus.LADDR, None, id0)
    # the replay alone answers every accepted frame with an RST and sends nothing else
    acc = int(np.count_nonzero(res == port.R_ACCEPT))
    assert txs.tolist() == [acc, 0, acc, 0, 0, 0] and idn == (id0 + acc) & 0xFFFF and idn < id0
    assert not np.any(res == port.R_NOTOURS)
    mine, nrst, ver, cls = referee_chain(port, buf, rx, ip_in, tcp_in, id0, slot)
    assert nrst == int(txs[2])
    assert np.array_equal(mine, tx)
    assert np.all(tx.reshape(n, slot)[acc:] == POISON)
    # the policy decided something: the verdicts hold both bad sums, and the three policies send different counts
    assert np.any(ver & R.BAD_IP) and np.any(ver & R.BAD_L4) and np.any((cls & 15) != l4ref.TCP)
    good = sum(k in ("good", "bad ip", "bad l4", "both") for k in kinds)
    assert acc == {2: sum(k == "good" for k in kinds), 1: sum(k in ("good", "bad l4") for k in kinds), 0: good}[ip_in]


# -- 3. the binding against the header -----------------------------------------------------

def struct_fields(hdr, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name}_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in re.findall(r"([^;]+);", body):
        for part in decl.split(","):
            out.append(re.search(r"\*?\s*([a-z_0-9]+)\s*$", part.strip()).group(1))
    return out


def test_constants_layouts_and_exports():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    vals = {"RST": 0, "SKIP": 2, "NOTMISS": 3, "DROPPED": 4, "NONE": 5, "QUIET": 6, "NCLASS": 7}
    for x, v in vals.items():
        m = re.search(rf"\bCGCK_RPL_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == v == getattr(cgck, f"RPL_{x}"), x
    assert (R.RST, R.SKIP, R.NOTMISS, R.DROPPED, R.NONE_, R.QUIET, R.NCLASS) == tuple(vals.values())
    # the class byte is cgck_l4_build's in.cls: an RST builds as TCP, the builder skips every other class
    assert cgck.RPL_RST == cgck.SEG_TCP == l4bref.SEG_TCP and cgck.RPL_IP6 == cgck.SEG_IP6 == cgck.BLD_IP6 == R.IP6
    assert all(v not in (cgck.SEG_TCP, cgck.SEG_UDP) and v < 16 for x, v in vals.items() if x not in ("RST", "NCLASS"))
    assert re.search(r"\bCGCK_RPL_IP6 = 1u << 4\b", hdr)
    for x, v in (("NO_RST", 1), ("NO_MCAST", 2)):
        m = re.search(rf"\bCGCK_RPL_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == v == getattr(cgck, f"RPL_{x}") == getattr(R, x), x
    m = re.search(r"#define CGCK_RPL_NCOUNT (\d+)", hdr)
    assert m and int(m.group(1)) == cgck.RPL_NCOUNT == R.NCOUNT == 8
    assert (R.PCB_MISS, R.L2_BCAST, R.L2_MCAST, R.BAD_IP, R.BAD_L4, R.BAD_LEN) == \
        (cgck.PCB_MISS, cgck.L2_BCAST, cgck.L2_MCAST, cgck.BAD_IP, cgck.BAD_L4, cgck.BAD_LEN)
    assert R.SEG_DTYPE == cgck.SEG_DTYPE and R.FLOW_DTYPE == cgck.FLOW_DTYPE
    # the three argument structs, field by field in the header's order
    for name, typ in (("cgck_l4_reply_in", cgck.L4ReplyIn), ("cgck_l4_reply_res", cgck.L4ReplyRes),
                      ("cgck_l4_reply_pack", cgck.L4ReplyPack)):
        assert struct_fields(hdr, name) == [f[0] for f in typ._fields_], name
    vp = ctypes.sizeof(ctypes.c_void_p)
    I = cgck.L4ReplyIn
    assert [getattr(I, f).offset for f in ("desc", "seg", "cls", "kind", "verdict", "l2cls", "at")] == [i * vp for i in range(7)]
    assert (I.link.offset, I.vmask.offset, I.flags.offset, ctypes.sizeof(I)) == (7 * vp, 7 * vp + 48, 7 * vp + 52, 7 * vp + 56)
    assert ctypes.sizeof(cgck.L4ReplyRes) == 5 * vp and ctypes.sizeof(cgck.L4ReplyPack) == 4 * vp
    assert ctypes.sizeof(cgck.Flow) == 48 == cgck.FLOW_DTYPE.itemsize
    for f, _ in cgck.Flow._fields_:
        assert getattr(cgck.Flow, f).offset == cgck.FLOW_DTYPE.fields[f][1], f
    L = cgck.load()
    for name in ("cgck_l4_reply", "cgck_l4_reply_packed", "cgck_l4_reply_rule", "cgck_test_l4_reply_pass",
                 "cgck_test_l4_reply_store"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert "#define CGCK_ABI_VERSION 2" in hdr and L.cgck_abi_version() == 2


def test_arguments_without_device():
    """The argument checks come before any device work."""
    L = cgck.load()
    arg, res, pk = cgck.L4ReplyIn(), cgck.L4ReplyRes(), cgck.L4ReplyPack()
    assert L.cgck_l4_reply(None, 16, 0, ctypes.byref(arg), ctypes.byref(res), None) == -22
    assert L.cgck_l4_reply_packed(None, 16, 0, ctypes.byref(arg), ctypes.byref(res), ctypes.byref(pk), None) == -22
    assert L.cgck_test_l4_reply_pass(None, None) == -22
    assert L.cgck_test_l4_reply_store(3) == -22 and L.cgck_test_l4_reply_store(-1) == -22
    assert cgck.l4_reply_store(cgck.L4R_STORE_TURNED) == cgck.L4R_STORE_DEFAULT
    assert cgck.l4_reply_store(cgck.L4R_STORE_OWN) == cgck.L4R_STORE_TURNED
    assert cgck.l4_reply_store(cgck.L4R_STORE_DEFAULT) == cgck.L4R_STORE_OWN
