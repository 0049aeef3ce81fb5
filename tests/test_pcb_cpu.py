"""CPU tests of cgck_pcb_build / cgck_pcb_lookup (no GPU): the referee
(tests/pcbref.py) against a brute-force scan, the corpus (tests/pcbbatches.py)
against what the contract names, the round trip through the referees of
cgck_l4_build, cgck_l2_desc and cgck_l4_desc, the kernels' probe text compiled for
the CPU under the sanitizers (tools/pcb_model) against the referee in every mode,
cgck_pcb_table_bytes, and the binding against the header.

The corpus is typed with the binding's record (CONN below), so nothing here runs
without the feature; the first three tests pin the referee and the corpus, the rest
the library's host side, the probe text and the binding.  The kernels are covered by
tests/test_gpu_pcb.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cgck
import l2ref
import l4bref
import l4ref
import pcbbatches as PB
import pcbref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
EINVAL = -22
CONN = cgck.CONN_DTYPE                                  # cgck_conn_t as the binding declares it
assert CONN == R.CONN_DTYPE, "the referee's connection record is not the binding's"


@pytest.fixture(scope="module")
def corpus():
    return PB.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return [R.lookup(c.burst.buf, c.burst.desc, c.burst.seg, c.burst.cls, c.table.conn, c.table.flow, c.table.bound)
            for c in corpus]


# -- 1. the referee against a scan --------------------------------------------------------

def test_referee_against_brute_force():
    """Random small tables over few distinct values, so that equal keys, twins of the
    other protocol and family, and unused and bad entries are common."""
    rng = np.random.default_rng(61)
    seen = set()
    for rep in range(12):
        nflow, nconn = int(rng.integers(1, 7)), int(rng.integers(0, 40))
        flow = np.zeros(nflow, l4bref.FLOW_DTYPE)
        for f in range(nflow):
            six = bool(rng.integers(0, 2))
            a = bytes(rng.integers(0, 2, 16 if six else 4, dtype=np.uint8))
            flow[f] = PB.flow_rec(rng, six, a, a[::-1])
            if rng.integers(0, 8) == 0:
                flow[f]["flags"] |= 0x10
        conn = np.zeros(nconn, R.CONN_DTYPE)
        conn["flow"] = rng.integers(0, nflow + 1, nconn)
        conn["lport"], conn["fport"] = PB.be16(80) + rng.integers(0, 2, nconn), rng.integers(0, 2, nconn)
        conn["proto"] = rng.choice([0, 6, 6, 17, 17], nconn)
        t = PB.Table("random", conn, flow, PB.bound_ports(nconn) if rep % 2 else None)
        specs = []
        for k in range(60):
            six = bool(rng.integers(0, 2))
            a = bytes(rng.integers(0, 2, 16 if six else 4, dtype=np.uint8))
            specs.append(("?", (six, int(rng.choice([6, 17])), a, a[::-1], PB.be16(80) + int(rng.integers(0, 2)),
                                int(rng.integers(0, 2))), None))
        b = PB.burst(specs, rng)
        cls = None if rep % 3 == 0 else b.cls
        got = R.lookup(b.buf, b.desc, b.seg, cls, t.conn, t.flow, t.bound)
        want = R.brute(b.buf, b.desc, b.seg, cls, t.conn, t.flow, t.bound)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        seen |= {int(x) for x in got[2]}
        _, stat = R.table(t.conn, t.flow)
        assert int(stat.sum()) == nconn
    assert seen == {R.HIT, R.BOUND, R.MISS}


# -- 2. the corpus ------------------------------------------------------------------------

def test_corpus_reaches_what_the_contract_names(corpus, expected):
    names = [c.name for c in corpus]
    assert names == ["dst-cache x1", "dst-cache x3", "dst-cache x64", "one SO_HASH", "duplicates", "mixed"]
    for c, (idx, fidx, kind, count) in zip(corpus, expected):
        t, b = c.table, c.burst
        tags = np.array(b.tags)
        # every kind in every class, and the kind each tag names
        assert {int(x) for x in kind} == set(range(R.NCLASS)), c.name
        assert np.array_equal(count[:5], np.bincount(kind, minlength=5)) and int(count[:5].sum()) == len(kind)
        assert np.all(kind[tags == "hit"] == R.HIT) and np.all(kind[tags == "bound"] == R.BOUND), c.name
        assert np.all(kind[tags == "skip"] == R.SKIP) and np.all(kind[np.char.startswith(tags, "none:")] == R.NONE_)
        assert {x for x in b.tags if x.startswith("none:")} == {"none:len0", "none:v4short", "none:v6short", "none:v6as20",
                                                                  "none:version"}
        for f in PB.ONE_FIELD:                          # each one-field miss is a miss
            sel = kind[tags == f"miss:{f}"]
            assert len(sel) == 3 and np.count_nonzero(sel == R.MISS) >= 1, (c.name, f)
            if c.name != "mixed":
                assert np.all(sel == R.MISS), (c.name, f)
        assert np.all(kind[tags == "miss:unbound"] == R.MISS)
        hit = kind == R.HIT
        assert np.array_equal(fidx[hit], t.conn["flow"][idx[hit]]) and np.all(fidx[~hit] == R.NOIDX)
        assert np.all(idx[(kind != R.HIT) & (kind != R.BOUND)] == R.NOIDX)
        assert np.all(b.desc["frame_off"] % PB.SLOT == 0) and len(b.buf) == len(b.desc) * PB.SLOT
    by = dict(zip(names, zip(corpus, expected)))
    # the dst-cache shape: one faddr, one fport, lports from 5000 up, 1 / 3 / 64 local addresses
    for name, nl in (("dst-cache x1", 1), ("dst-cache x3", 3), ("dst-cache x64", 64)):
        t = by[name][0].table
        keys = [t.spec(j) for j in range(len(t.conn))]
        assert len({k[2] for k in keys}) == nl and len({k[3] for k in keys}) == 1 and len({k[5] for k in keys}) == 1
        assert min(R.bswap16(k[4]) for k in keys) == 5000 and len(set(keys)) == len(keys)
    # one SO_HASH value over the whole class, and over the frames that hit it
    t = by["one SO_HASH"][0].table
    fw = int(t.flow["faddr"][0][:4].view("<u4")[0])
    assert len({l4ref.so_hash(fw, int(c["lport"]), int(c["fport"])) for c in t.conn}) == 1 and len(t.conn) == 200
    # every duplicate distance, the lower index reported
    c, (idx, _, kind, _) = by["duplicates"]
    assert [b - a for a, b in c.table.pairs] == list(PB.DUP_DISTANCES)
    _, stat = R.table(c.table.conn, c.table.flow)
    assert stat.tolist() == [len(c.table.conn) - 4, 4, 0, 0]
    for a, b in c.table.pairs:
        assert c.table.spec(a) == c.table.spec(b) and int(c.table.conn["flow"][a]) != int(c.table.conn["flow"][b])
        at = [k for k in range(len(kind)) if kind[k] == R.HIT and int(idx[k]) == a]
        assert len(at) == 2 and not np.any(idx == b)    # the frames built from a and from b both resolve to a
    # mixed: equal IPv4 keys through other flow bytes, TCP and UDP apart, the families apart, unused and bad entries
    c, (idx, fidx, kind, count) = by["mixed"]
    t = c.table
    _, stat = R.table(t.conn, t.flow)
    assert stat.tolist() == [10, 1, 1, 4]
    assert t.spec(0) == t.spec(1) and t.spec(0)[1:] != t.spec(2)[1:] and t.spec(0)[2] == t.spec(3)[2][:4]
    hits = {int(x) for x in idx[kind == R.HIT]}
    assert hits == {0, 2, 3, 4, 5, 11, 12, 13, 15} and int(count[5]) >= 3
    assert int(t.bound[80]) != R.NOIDX                  # connection 13 is a HIT although its port is bound


def test_round_trip_with_referees_only():
    """Frames that l4bref builds from (flow, seg, fidx) with unique tuples, read back
    through l2ref and l4ref, look up to the fidx that went in."""
    rng = np.random.default_rng(62)
    nflow, n = 40, 150
    flow = np.zeros(nflow, l4bref.FLOW_DTYPE)           # the receiver's table: laddr is the frame's destination
    for f in range(nflow):
        six = f % 3 == 0
        flow[f] = PB.flow_rec(rng, six, bytes([10, 0, 0, f]) + bytes(12 if six else 0), bytes([10, 9, 0, f % 5]) + bytes(12 if six else 0))
    conn = np.zeros(nflow, R.CONN_DTYPE)
    conn["flow"], conn["lport"], conn["fport"] = np.arange(nflow), PB.be16(7000), PB.be16(80)
    conn["proto"] = np.where(np.arange(nflow) % 4 == 1, 17, 6)
    peer = flow.copy()                                  # the sender's view of the same flows
    peer["laddr"], peer["faddr"] = flow["faddr"], flow["laddr"]
    fidx = rng.integers(0, nflow, n).astype(np.uint32)
    seg = np.zeros(n, l4bref.SEG_DTYPE)
    seg["sport"], seg["dport"], seg["th_flags"] = PB.be16(80), PB.be16(7000), 0x10
    cls = np.where(conn["proto"][fidx] == 17, l4bref.SEG_UDP, l4bref.SEG_TCP).astype(np.uint8)
    slot = np.zeros(n, l4bref.DESC_DTYPE)
    slot["frame_off"], slot["ip_len"] = np.arange(n) * 128, 128
    buf = np.zeros(n * 128, np.uint8)
    raw, desc, bcls, _ = l4bref.build(buf, slot, seg, peer, cls, fidx, 1, 0x4000)
    assert np.all((bcls & 15) <= l4bref.UDP)
    d2, _, _ = l2ref.expect(buf, raw)
    assert np.array_equal(d2, desc)
    sg, c4, _, _ = l4ref.expect(buf, d2)
    idx, out, kind, count = R.lookup(buf, d2, sg, c4, conn, flow)
    assert np.all(kind == R.HIT) and np.array_equal(out, fidx) and np.array_equal(idx, fidx)
    assert int(count[0]) == n and int(count[5]) == np.count_nonzero(fidx % 3 == 0)


# -- 3. the probe text on the CPU, under the sanitizers -----------------------------------

@pytest.fixture(scope="module")
def model():
    subprocess.run(["make", "-s", "-C", TOOLS, "pcb_model"], check=True)
    return os.path.join(TOOLS, "pcb_model")


@pytest.mark.parametrize("mode", range(4))
def test_model_against_referee(model, corpus, expected, mode, tmp_path):
    """tools/pcb_model (cgck_pcb_probe.h over plain arrays, -fsanitize=address,undefined)
    over the whole corpus: stat, idx, fidx, kind and count are the referee's, and the
    sanitizers stay silent."""
    variants = [(c, e, True, True) for c, e in zip(corpus, expected)]
    c = corpus[-1]
    for use_cls, use_bound in ((False, True), (True, False)):
        e = R.lookup(c.burst.buf, c.burst.desc, c.burst.seg, c.burst.cls if use_cls else None, c.table.conn, c.table.flow,
                     c.table.bound if use_bound else None)
        variants.append((c, e, use_cls, use_bound))
    empty = PB.Table("empty", [], [], c.table.bound)    # nconn == 0: MISS, BOUND, SKIP or NONE
    e = R.lookup(c.burst.buf, c.burst.desc, c.burst.seg, c.burst.cls, empty.conn, empty.flow, empty.bound)
    assert R.HIT not in e[2] and {R.MISS, R.BOUND, R.SKIP, R.NONE_} == {int(x) for x in e[2]}
    variants.append((PB.Case(empty, c.burst), e, True, True))
    for i, (c, (idx, fidx, kind, count), use_cls, use_bound) in enumerate(variants):
        fin, fout = str(tmp_path / f"in{i}"), str(tmp_path / f"out{i}")
        PB.write_model_file(fin, c.table, c.burst, use_cls, use_bound)
        r = subprocess.run([model, fin, fout, str(mode)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (c.name, r.returncode, r.stderr[-2000:])
        stat, gi, gf, gk, gc = PB.read_model_file(fout, len(kind))
        what = (c.name, mode, use_cls, use_bound)
        assert np.array_equal(stat, R.table(c.table.conn, c.table.flow)[1]), what
        assert np.array_equal(gk, kind) and np.array_equal(gi, idx) and np.array_equal(gf, fidx), what
        assert np.array_equal(gc, count), what


# -- 4. cgck_pcb_table_bytes --------------------------------------------------------------

def test_table_bytes_sweep():
    ns = sorted({0, 1, 1 << 30} | {v for e in range(1, 31) for v in ((1 << e) - 1, 1 << e, (1 << e) + 1) if v <= 1 << 30})
    prev = 0
    for n in ns:
        got = cgck.pcb_table_bytes(n)
        slots = 2
        while slots < 2 * n:
            slots *= 2
        assert got == 8 * slots and got % 16 == 0 and got >= prev and got >= 16 * n, n
        prev = got
    assert cgck.pcb_table_bytes(0) == 16 and cgck.pcb_table_bytes(1) == 16 and cgck.pcb_table_bytes(3) == 64
    assert cgck.pcb_table_bytes(1 << 30) == 16 << 30
    for n in ((1 << 30) + 1, 1 << 31, 0xFFFFFFFF):
        assert cgck.pcb_table_bytes(n) == 0


# -- 5. the binding against the header ----------------------------------------------------

def struct_body(hdr, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name}_t;", hdr, re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def test_constants_layouts_and_exports():
    hdr = open(os.path.join(ROOT, "include", "cgck.h")).read()
    for i, x in enumerate(R.NAMES + ("NCLASS",)):
        m = re.search(rf"\bCGCK_PCB_{x} = (\d+)", hdr)
        assert m and int(m.group(1)) == i == getattr(cgck, f"PCB_{x}"), x
    assert (R.HIT, R.BOUND, R.MISS, R.SKIP, R.NONE_) == (0, 1, 2, 3, 4)
    for x, v in (("NCOUNT", 6), ("NBOUND", 5000)):
        m = re.search(rf"#define CGCK_PCB_{x} (\d+)", hdr)
        assert m and int(m.group(1)) == v == getattr(cgck, f"PCB_{x}") == getattr(R, x), x
    # sizeof(cgck_conn_t) == 12 == CONN_DTYPE.itemsize, field by field as the header declares them
    size = {"uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    off, names = 0, []
    for typ, ids in re.findall(r"(uint\d+_t)\s+([a-z_0-9, \[\]]+);", struct_body(hdr, "cgck_conn")):
        for name in ids.split(","):
            name, cnt = re.fullmatch(r"\s*([a-z_0-9]+)(?:\[(\d+)\])?\s*", name).groups()
            cnt = int(cnt or 1)
            assert off % size[typ] == 0
            dt, at = cgck.CONN_DTYPE.fields[name][:2]
            assert at == off and dt.itemsize == size[typ] * cnt and dt.base.itemsize == size[typ], name
            names.append(name)
            off += size[typ] * cnt
    assert off == 12 == cgck.CONN_DTYPE.itemsize == R.CONN_DTYPE.itemsize
    assert tuple(names) == cgck.CONN_DTYPE.names == R.CONN_DTYPE.names
    # the two argument structs as the header declares them
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert re.findall(r"\b([a-z_0-9]+);", struct_body(hdr, "cgck_pcb")) == [f[0] for f in cgck.Pcb._fields_]
    assert re.findall(r"\b([a-z_0-9]+);", struct_body(hdr, "cgck_pcb_res")) == [f[0] for f in cgck.PcbRes._fields_]
    assert ctypes.sizeof(cgck.PcbRes) == 4 * vp and ctypes.sizeof(cgck.Pcb) == 7 * vp
    assert [getattr(cgck.Pcb, f).offset for f, _ in cgck.Pcb._fields_] == [0, vp, 2 * vp, 3 * vp, 4 * vp, 5 * vp, 6 * vp]
    L = cgck.load()
    for name in ("cgck_pcb_table_bytes", "cgck_pcb_build", "cgck_pcb_lookup", "cgck_test_pcb_pass", "cgck_test_pcb_mode"):
        assert name in cgck.EXPORTS and hasattr(L, name), name
    assert "#define CGCK_ABI_VERSION 2" in hdr and L.cgck_abi_version() == 2


def test_arguments_without_device():
    """The argument checks come before any device work."""
    L = cgck.load()
    by = ctypes.byref
    need = cgck.pcb_table_bytes(4)
    ok = dict(conn=0x1000, nconn=4, flow=0x2000, nflow=4, table=0x3000, table_bytes=need, bound=0x4000)

    def pcb(**kw):
        return cgck.Pcb(**{**ok, **kw})
    res = cgck.PcbRes(0x5000, 0x6000, 0x7000, 0x8000)
    assert L.cgck_pcb_build(None, by(pcb()), None, None) == EINVAL
    assert L.cgck_pcb_lookup(None, 16, 16, 16, None, 1, by(pcb()), by(res), None) == EINVAL
    assert L.cgck_test_pcb_pass(None, None) == EINVAL
    # the mode pin: returns the previous value, refuses anything outside 0..3
    assert L.cgck_test_pcb_mode(4) == EINVAL and L.cgck_test_pcb_mode(-1) == EINVAL
    assert cgck.pcb_mode(3) == 0 and cgck.pcb_mode(1) == 3 and cgck.pcb_mode(0) == 1
