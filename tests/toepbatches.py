"""Inputs for the edge tests of cgck_toeplitz and cgck_dst_cache
(tests/test_gpu_rss.py, tests/test_rss_edges_cpu.py), and the dispatch rule of
launch_toeplitz (cgck_rss.hip) restated from its wording, not imported from the
library.  Plain numpy: no device, no library.

A batch case is (n, stride, cnt, data_shift, out_shift): n records of cnt bytes,
stride bytes apart, in an allocation of exactly (n - 1) * stride + cnt bytes that
starts data_shift bytes past a 16-byte boundary; out starts out_shift bytes past
one.

A dst-cache configuration is a dict with the fields of cgck_dst_params_t (host
order ranges as (min, max), fport as stored) and, where it is fixed, `cap`."""
import numpy as np

X4 = "toeplitz12x4_ab_kernel<12>"     # dense 12-byte records, 4 per lane, register ring of depth 12
W3 = "toeplitz_kernel<3, true>"       # cnt 12 as 3 dword loads, tables in LDS
W9 = "toeplitz_kernel<9, true>"       # cnt 36 as 9 dword loads, tables in LDS
B_LDS = "toeplitz_kernel<0, true>"    # any cnt up to 36 by byte loads, tables in LDS
B_GLB = "toeplitz_kernel<0, false>"   # cnt above 36: tables read from global memory
KERNELS = (X4, W3, W9, B_LDS, B_GLB)
LDS_MAX_CNT = 36                      # tables of up to 36 KiB are staged in LDS
MAX_CNT = 65536                       # the longest record cgck_toeplitz takes


def expected_kernel(n, stride, cnt, data_shift=0, out_shift=0):
    """The kernel name launch_toeplitz must report (None: nothing is launched).
    Dense 12-byte records with data and out on 16-byte boundaries and at least one
    group of four go to the x4 kernel (its n % 4 tail runs on the per-record kernel
    without renaming the call).  Otherwise records that start on dword boundaries
    (base and stride multiples of 4) of 12 or 36 bytes take the dword kernels, any
    other cnt up to the LDS limit the byte kernel, and longer ones the byte kernel
    with its tables in global memory."""
    if n == 0:
        return None
    if cnt == 12 and stride == 12 and data_shift % 16 == 0 and out_shift % 16 == 0 and n >= 4:
        return X4
    aligned = data_shift % 4 == 0 and stride % 4 == 0
    if aligned and cnt == 12:
        return W3
    if aligned and cnt == 36:
        return W9
    return B_LDS if cnt <= LDS_MAX_CNT else B_GLB


def data_bytes(n, stride, cnt):
    """The bytes n records span: the last record ends the allocation."""
    return (n - 1) * stride + cnt if n else 0


def records(n, stride, cnt, seed):
    """Random bytes for a case; overlapping records (stride < cnt) then differ too."""
    rng = np.random.default_rng([seed, n, stride, cnt])
    return rng.integers(0, 256, data_bytes(n, stride, cnt), dtype=np.uint8)


def key_bytes(size, seed):
    return np.random.default_rng([77, seed]).integers(0, 256, size, dtype=np.uint8)


# -- cgck_toeplitz -----------------------------------------------------------------------

# n = 4*256 + 4*37 + 3: a full 256-group block, a partial one and an n % 4 tail.
ALIGN_N = 1175
ALIGN_CASES = [(ALIGN_N, 12, 12, ds, os) for ds in (0, 4, 8, 12, 1) for os in (0, 4, 8, 12)]

# ng = n / 4 in {255, 256, 257} with every n % 4, the smallest x4 batches, and n < 4.
X4_SIZES = (1, 2, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1023, 1024, 1025, 1027, 1028, 1029)
X4_CASES = [(n, 12, 12, 0, 0) for n in X4_SIZES]

# (cnt, stride): around 12 and 36, the LDS limit 35 / 36 / 37, strides that are no
# multiple of 4, overlapping records (stride < cnt), stride 0, cnt 0 and 1.
GRID_N = 259
GRID = ((12, 16), (12, 4), (36, 36), (36, 40), (36, 4), (36, 37), (35, 36), (37, 40), (11, 12), (13, 16),
        (1, 1), (0, 8), (12, 0), (40, 1))
GRID_CASES = [(GRID_N, stride, cnt, 0, 0) for cnt, stride in GRID]

MASKS = (0xFFFFFFFF, 0x7F, 0, 0x80000001)
# one case per kernel name; the x4 one with a tail, which the per-record kernel masks
MASK_CASES = [(ALIGN_N, 12, 12, 0, 0), (GRID_N, 16, 12, 0, 0), (GRID_N, 36, 36, 0, 0), (GRID_N, 16, 13, 0, 0),
              (GRID_N, 40, 37, 0, 0)]

# (stride, cnt) of the second-pass cases, one per toeplitz_kernel instantiation;
# n = 2 * (records of one pass) + 257 comes from the device (Engine.rss_pass).
PASS_SHAPES = ((4, 12), (4, 36), (1, 13), (1, 37))


def pass_n(pass_records):
    return 2 * pass_records + 257


def cases_by_mask(pass_records=8 * 256 * 256):
    """{mask: the cases that run under it}."""
    full = ALIGN_CASES + X4_CASES + GRID_CASES + [(pass_n(pass_records), s, c, 0, 0) for s, c in PASS_SHAPES]
    return {m: (full if m == 0xFFFFFFFF else []) + MASK_CASES for m in MASKS}


# -- cgck_dst_cache ----------------------------------------------------------------------

NEPH, EPH_MIN = 65535 - 5000 + 1, 5000     # the ephemeral local ports of the loop
TILE_EDGE = 8192                           # every tile edge is a multiple of 256 * 32 tuples
L0, F0, FPORT = 167772161, 167837697, 20480    # 10.0.0.1, 10.1.0.1, port 80 as stored: the goldens' bases


def config(name, nl, nf, queue_num, queue_id, cap=None, l0=L0, f0=F0):
    return dict(name=name, laddr=(l0, (l0 + nl - 1) & 0xFFFFFFFF), faddr=(f0, (f0 + nf - 1) & 0xFFFFFFFF),
                fport=FPORT, queue_num=queue_num, queue_id=queue_id, cap=cap, nl=nl, nf=nf)


# caps on tile edges: edge_caps() of the full enumeration of each
EDGE_CONFIGS = [config("nofilter_nf3", 1, 3, 1, 0), config("q4_1_nl2_nf3", 2, 3, 4, 1),
                config("q128_127_nf3", 1, 3, 128, 127)]
# nf around the 64-tuple step of the cursor (the goldens hold 63, 64, 65 and 130)
NF_CONFIGS = [config(f"nf{nf}_q3_2", 1, nf, 3, 2, cap=5000) for nf in (1, 2, 3, 32, 128, 60536, 60537)]
# n close to 2^32 (4 237 520 000 tuples, half a million tiles) with an early stop
LARGE_CONFIGS = [config("nf70000_q4_1", 1, 70000, 4, 1, cap=1000, f0=167837696),
                 config("nf70000_nofilter", 1, 70000, 1, 0, cap=100000, f0=167837696)]
# n == 0 in 32-bit arithmetic: nf == 0 and nl == 0
EMPTY_CONFIGS = [dict(config("nf0", 1, 1, 4, 1, cap=100), faddr=(0, 0xFFFFFFFF), nf=0),
                 dict(config("nl0", 1, 1, 4, 1, cap=100), laddr=(0, 0xFFFFFFFF), nl=0)]


def tuples(c):
    """The tuple count as the loop forms it, in 32-bit unsigned arithmetic."""
    nl = (c["laddr"][1] - c["laddr"][0] + 1) & 0xFFFFFFFF
    nf = (c["faddr"][1] - c["faddr"][0] + 1) & 0xFFFFFFFF
    return (nl * nf * NEPH) & 0xFFFFFFFF


def referee(port, c, key, cap=None):
    """The referee's entries for a configuration (cap None: the whole enumeration)."""
    cap = tuples(c) + 1 if cap is None else cap
    return port.dst_cache(c["laddr"][0], c["laddr"][1], c["faddr"][0], c["faddr"][1], c["fport"], c["queue_num"],
                          c["queue_id"], key, cap)


def tuple_index(entries, l0, f0, nf):
    """The loop index i = ((la - l0) * 60536 + (lport - 5000)) * nf + (fa - f0) of
    each entry, from its fields in host order."""
    la = entries["laddr"].byteswap().astype(np.int64)
    fa = entries["faddr"].byteswap().astype(np.int64)
    lp = entries["lport"].byteswap().astype(np.int64)
    return ((la - l0) * NEPH + (lp - EPH_MIN)) * nf + (fa - f0)


def edge_counts(entries, l0, f0, nf, ks=(1, 2, 16)):
    """c_k: the entries among the first 8192 * k tuples."""
    i = tuple_index(entries, l0, f0, nf)
    return [int(np.count_nonzero(i < TILE_EDGE * k)) for k in ks]


def edge_caps(entries, l0, f0, nf, ks=(1, 2, 16)):
    """The caps at which a tile's inclusive count meets cap exactly, one below and
    one above, for the tiles that end at tuple 8192 * k; the same around the whole
    enumeration; and 1."""
    total = len(entries)
    caps = {1, total - 1, total, total + 1}
    for ck in edge_counts(entries, l0, f0, nf, ks):
        caps |= {ck - 1, ck, ck + 1}
    return sorted(c for c in caps if c >= 1)
