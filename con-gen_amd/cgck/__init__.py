"""cgck — Python binding of libcgck.so, the gfx950 Internet-checksum engine.

Mirrors the reference's checksum interface (subr.h:176-177, 373-374):

    in_cksum(buf, off, n)        uint16_t in_cksum(void *, int)
    udp_cksum(buf, ip_off, n)    uint16_t udp_cksum(struct ip *, int)
    ip_cksum(buf, ip_off)        #define ip_cksum(ip) in_cksum(ip, ip->ip_hl << 2)
    tcp_cksum                    #define tcp_cksum udp_cksum

plus the batched C-ABI of include/cgck.h (`Engine`).  Everything here calls
the HIP kernels through the C-ABI; there is no Python or host arithmetic
path, and loading fails loudly when the library is missing.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGCK_LIB", os.path.join(os.path.dirname(HERE), "libcgck.so"))

# Flags and verdict bits (include/cgck.h).
RAW = 1 << 0
IP = 1 << 1
L4 = 1 << 2
L4_NOPSEUDO = 1 << 3
ZERO_FIELDS = 1 << 4
STORE = 1 << 5
VERIFY = 1 << 6
V_IP_ZERO_IS_FFFF = 1 << 7
V_UDP_ZERO_SKIP = 1 << 8
IP6 = 1 << 9            # the record at l3_off is an IPv6 header (include/cgck.h, CGCK_IP6)
MIXED = 1 << 10         # each record is IPv4 or IPv6 by its own version nibble (CGCK_MIXED)
GEN_BOTH = IP | L4
FILL_BOTH = IP | L4 | ZERO_FIELDS | STORE
VERIFY_BSD = IP | L4 | VERIFY | V_IP_ZERO_IS_FFFF | V_UDP_ZERO_SKIP
VERIFY_TOY = IP | L4 | VERIFY
BAD_IP = 1
BAD_L4 = 2
BAD_LEN = 4
NOT_IP = 8              # CGCK_MIXED: the record is neither IPv4 nor IPv6
# Per-frame RSS hash (cgck_rss_strided / _desc / _desc_host): hf bits and kind bits.
RSS_TCP = 1 << 0        # hf: TCP frames hash their ports
RSS_UDP = 1 << 1        # hf: UDP frames hash their ports
RSS_L4 = 1 << 4         # kind: the ports were hashed
RSS_IP6 = 1 << 5        # kind: an IPv6 tuple

# cgck_dst_entry_t (include/cgck.h): the struct ip_socket fields con-gen.c:344-349 fills.
DST_DTYPE = np.dtype([("laddr", "<u4"), ("faddr", "<u4"), ("lport", "<u2"), ("fport", "<u2"),
                      ("hash", "<u4")])
assert DST_DTYPE.itemsize == 16


class DstParams(ctypes.Structure):
    """cgck_dst_params_t: the struct thread fields thread_init_dst_cache reads."""
    _fields_ = [("laddr_min", ctypes.c_uint32), ("laddr_max", ctypes.c_uint32),
                ("faddr_min", ctypes.c_uint32), ("faddr_max", ctypes.c_uint32),
                ("fport", ctypes.c_uint16), ("rss_queue_num", ctypes.c_uint8),
                ("rss_queue_id", ctypes.c_uint8), ("rss_key", ctypes.c_void_p),
                ("rss_key_size", ctypes.c_int)]


DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("l3_off", "<u2"), ("ip_len", "<u2")], align=False)
assert DESC_DTYPE.itemsize == 12


class RssSpec(ctypes.Structure):
    """cgck_rss_spec_t: key, mask, hashed protocols and queue count of a frame hash."""
    _fields_ = [("key", ctypes.c_void_p), ("key_size", ctypes.c_int), ("mask", ctypes.c_uint32),
                ("hf", ctypes.c_uint32), ("queue_num", ctypes.c_uint32)]


class RssRes(ctypes.Structure):
    """cgck_rss_res_t: the optional per-frame outputs and the queue counters."""
    _fields_ = [("hash", ctypes.c_void_p), ("kind", ctypes.c_void_p), ("queue", ctypes.c_void_p),
                ("qcount", ctypes.c_void_p)]


# cgck_l2_desc: the class in the low nibble of cls[k], the flag bits beside it,
# and the length of the counter array.
L2_IP4, L2_IP6, L2_ARP, L2_OTHER, L2_RUNT = 0, 1, 2, 3, 4
L2_TOOSMALL, L2_BADVERS, L2_BADHLEN, L2_BADLEN, L2_TOOSHORT = 5, 6, 7, 8, 9
L2_NCLASS = 10
L2_VLAN = 1 << 4
L2_BCAST = 1 << 6
L2_MCAST = 1 << 7
L2_NCOUNT = 12          # [class] for the ten classes, [10] BCAST or MCAST frames, [11] tagged frames


class L2Res(ctypes.Structure):
    """cgck_l2_res_t: the optional outputs of the raw-burst classifier."""
    _fields_ = [("desc_out", ctypes.c_void_p), ("cls", ctypes.c_void_p), ("count", ctypes.c_void_p)]


# cgck_l4_desc: the class in the low nibble of cls[k], the family bit beside it,
# the option bits of cgck_seg_t.opt, and the running counters.
SEG_TCP, SEG_UDP, SEG_ICMP, SEG_OTHER, SEG_FRAG, SEG_NONE = 0, 1, 2, 3, 4, 5
SEG_TCP_SHORT, SEG_TCP_BADOFF, SEG_TCP_OFFLONG, SEG_UDP_SHORT, SEG_UDP_BADLEN = 6, 7, 8, 9, 10
SEG_NCLASS = 11
SEG_IP6 = 1 << 4
SEG_MSS, SEG_WS, SEG_TS, SEG_OPT_BAD = 1, 2, 4, 0x80
SEG_NCOUNT = 12         # [class] for the eleven classes, [11] frames with SEG_IP6
# cgck_seg_t
SEG_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"),
                      ("sport", "<u2"), ("dport", "<u2"), ("win", "<u2"), ("mss", "<u2"),
                      ("l4_off", "<u2"), ("pay_len", "<u2"), ("th_flags", "u1"), ("hdr_len", "u1"),
                      ("wscale", "u1"), ("opt", "u1")])
assert SEG_DTYPE.itemsize == 32


class L4Res(ctypes.Structure):
    """cgck_l4_res_t: the optional outputs of the segment parser."""
    _fields_ = [("seg", ctypes.c_void_p), ("cls", ctypes.c_void_p), ("hash", ctypes.c_void_p),
                ("count", ctypes.c_void_p)]


# cgck_l4_build: the flow record, the flag bits of cgck_flow_t.flags, the class in
# the low nibble of cls[k] with the flag bits beside it, and the running counters.
FLOW_DTYPE = np.dtype([("eth_dst", "u1", (6,)), ("eth_src", "u1", (6,)), ("vlan_tci", "<u2"), ("flags", "u1"),
                       ("ttl", "u1"), ("laddr", "u1", (16,)), ("faddr", "u1", (16,))])
assert FLOW_DTYPE.itemsize == 48
FLOW_IP6, FLOW_VLAN = 1, 2
BLD_TCP, BLD_UDP, BLD_SKIP, BLD_BADFLOW, BLD_BADSEG, BLD_NOROOM = 0, 1, 2, 3, 4, 5
BLD_NCLASS = 6
BLD_IP6 = 1 << 4
BLD_PAYLOAD = 1 << 5
BLD_NCOUNT = 8          # [class] for the six classes, [6] built IPv6 frames, [7] built frames with BLD_PAYLOAD


class L4BuildIn(ctypes.Structure):
    """cgck_l4_build_in_t: where the frames go and what they are built from."""
    _fields_ = [("slot", ctypes.c_void_p), ("seg", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("flow", ctypes.c_void_p), ("fidx", ctypes.c_void_p), ("nflow", ctypes.c_uint32),
                ("ip_id0", ctypes.c_uint16), ("ip_off", ctypes.c_uint16)]


class L4BuildRes(ctypes.Structure):
    """cgck_l4_build_res_t: the optional outputs of the frame builder."""
    _fields_ = [("raw_out", ctypes.c_void_p), ("desc_out", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("count", ctypes.c_void_p)]


# cgck_pcb_build / cgck_pcb_lookup: the connection record, the kind of a frame's
# lookup, the running counters and the ports a listening socket binds.
CONN_DTYPE = np.dtype([("flow", "<u4"), ("lport", "<u2"), ("fport", "<u2"), ("proto", "u1"), ("rsv", "u1", (3,))])
assert CONN_DTYPE.itemsize == 12
PCB_HIT, PCB_BOUND, PCB_MISS, PCB_SKIP, PCB_NONE = 0, 1, 2, 3, 4
PCB_NCLASS = 5
PCB_NCOUNT = 6          # [kind] for the five kinds, [5] HITs on IPv6 frames
PCB_NBOUND = 5000       # EPHEMERAL_MIN
PCB_MODE_CHAIN = 1      # cgck_test_pcb_mode: every key's home slot is the table's last
PCB_MODE_UNTAGGED = 2   # cgck_test_pcb_mode: 4-byte slots, the index alone


class Pcb(ctypes.Structure):
    """cgck_pcb_t: the caller's connection and flow arrays, the table and the bound ports."""
    _fields_ = [("conn", ctypes.c_void_p), ("nconn", ctypes.c_uint32), ("flow", ctypes.c_void_p),
                ("nflow", ctypes.c_uint32), ("table", ctypes.c_void_p), ("table_bytes", ctypes.c_size_t),
                ("bound", ctypes.c_void_p)]


class PcbRes(ctypes.Structure):
    """cgck_pcb_res_t: the optional outputs of the connection lookup."""
    _fields_ = [("idx", ctypes.c_void_p), ("fidx", ctypes.c_void_p), ("kind", ctypes.c_void_p),
                ("count", ctypes.c_void_p)]


# cgck_l4_reply: the class in the low nibble of cls[k] (cgck_l4_build's in.cls: RPL_RST
# is SEG_TCP, every other class one the builder skips), the family bit beside it, the
# flags of the call and the running counters.
RPL_RST, RPL_SKIP, RPL_NOTMISS, RPL_DROPPED, RPL_NONE, RPL_QUIET = 0, 2, 3, 4, 5, 6
RPL_NCLASS = 7
RPL_IP6 = 1 << 4
RPL_NO_RST, RPL_NO_MCAST = 1, 2
RPL_NCOUNT = 8          # [class] for the seven class values, [7] RSTs on IPv6 frames
L4R_STORE_DEFAULT, L4R_STORE_OWN, L4R_STORE_TURNED = 0, 1, 2


class Flow(ctypes.Structure):
    """cgck_flow_t by value (FLOW_DTYPE's layout): cgck_l4_reply's link template."""
    _fields_ = [("eth_dst", ctypes.c_uint8 * 6), ("eth_src", ctypes.c_uint8 * 6), ("vlan_tci", ctypes.c_uint16),
                ("flags", ctypes.c_uint8), ("ttl", ctypes.c_uint8), ("laddr", ctypes.c_uint8 * 16),
                ("faddr", ctypes.c_uint8 * 16)]

    @classmethod
    def of(cls, rec):
        """From a FLOW_DTYPE record, a Flow, or None (all zero)."""
        if isinstance(rec, cls):
            return rec
        f = cls()
        if rec is not None:
            raw = np.asarray(rec, FLOW_DTYPE).reshape(1).view(np.uint8)
            ctypes.memmove(ctypes.byref(f), raw.ctypes.data, 48)
        return f


assert ctypes.sizeof(Flow) == 48


class L4ReplyIn(ctypes.Structure):
    """cgck_l4_reply_in_t: the received burst, the selectors and the link template."""
    _fields_ = [("desc", ctypes.c_void_p), ("seg", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("kind", ctypes.c_void_p), ("verdict", ctypes.c_void_p), ("l2cls", ctypes.c_void_p),
                ("at", ctypes.c_void_p), ("link", Flow), ("vmask", ctypes.c_uint8), ("flags", ctypes.c_uint32)]


class L4ReplyRes(ctypes.Structure):
    """cgck_l4_reply_res_t: the optional outputs of the reply rule."""
    _fields_ = [("seg", ctypes.c_void_p), ("flow", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("queue", ctypes.c_void_p), ("count", ctypes.c_void_p)]


class L4ReplyPack(ctypes.Structure):
    """cgck_l4_reply_pack_t: the caller's intermediates of cgck_l4_reply_packed."""
    _fields_ = [("queue", ctypes.c_void_p), ("at", ctypes.c_void_p), ("qoff", ctypes.c_void_p),
                ("work", ctypes.c_void_p)]


class SteerRes(ctypes.Structure):
    """cgck_steer_res_t: the optional outputs of the partition by queue id."""
    _fields_ = [("qoff", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("slot", ctypes.c_void_p),
                ("desc_out", ctypes.c_void_p)]

# Every symbol include/cgck.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "in_cksum", "udp_cksum", "cgck_last_error", "cgck_abi_version", "cgck_ctx_create",
    "cgck_ctx_destroy", "cgck_ctx_stream", "cgck_ctx_sync", "cgck_strided", "cgck_desc",
    "cgck_set_desc_len_hint", "cgck_desc_host", "cgck_host_register", "cgck_host_unregister",
    "cgck_thread_release", "cgck_tx_begin", "cgck_tx_flush", "cgck_synth_strided",
    "cgck_synth_imix", "cgck_imix_bytes", "cgck_device_count", "cgck_dev_alloc", "cgck_dev_free",
    "cgck_host_alloc", "cgck_host_free", "cgck_memcpy", "cgck_memset", "cgck_event_create",
    "cgck_event_destroy", "cgck_event_record", "cgck_event_elapsed_ms", "cgck_probe_read",
    "toeplitz_hash", "rss_hash4", "cgck_toeplitz", "cgck_dst_cache", "cgck_dst_cache_host",
    "cgck_burst_open", "cgck_burst_close", "cgck_thread_ctx", "cgck_set_error_handler",
    "cgck_rx_begin", "cgck_rx_end", "cgck_window_stats", "cgck_ctx_last_kernel", "cgck_set_desc_layout",
    "cgck_ctx_set_kernel", "cgck_synth_imix_ring", "cgck_burst_request", "cgck_host_device_ptr",
    "cgck_rx_post", "cgck_rx_begin_posted", "cgck_tx_post", "cgck_tx_complete",
    "cgck_rx_pending", "cgck_rx_ready", "cgck_tx_pending", "cgck_tx_ready",
    "cgck_window_stats_n", "cgck_thread_bind", "cgck_thread_device",
    "cgck_test_burst_seq", "cgck_test_burst_stale", "cgck_synth_strided_ip6",
    "cgck_synth_imix_ip6", "cgck_synth_imix_ring_ip6", "cgck_synth_imix_dual",
    "cgck_rss_strided", "cgck_rss_desc", "cgck_rss_desc_host",
    "cgck_test_burst_route", "cgck_test_burst_route_kind",
    "cgck_steer_work_bytes", "cgck_steer", "cgck_rss_steer_desc", "cgck_test_steer_plan",
    "cgck_l2_desc", "cgck_synth_eth", "cgck_test_l2_pass",
    "cgck_l4_desc", "cgck_test_l4_pass",
    "cgck_l4_build", "cgck_l4_build_hdr_bytes", "cgck_test_l4_build_pass", "cgck_test_l4_build_store",
    "cgck_pcb_table_bytes", "cgck_pcb_build", "cgck_pcb_lookup", "cgck_test_pcb_pass", "cgck_test_pcb_mode",
    "cgck_test_rss_pass",
    "cgck_l4_reply", "cgck_l4_reply_packed", "cgck_l4_reply_rule", "cgck_test_l4_reply_pass", "cgck_test_l4_reply_store",
)
# Descriptor layout hint (cgck_set_desc_layout)
LAYOUT_ANY = 0
LAYOUT_PACKED = 1
LAB_PATH = os.path.join(os.path.dirname(HERE), "libcgck_lab.so")

# cgck_error_fn: void (*)(const char *what, const char *msg, void *arg)
ERROR_FN = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p)


class CgckError(RuntimeError):
    pass


_lib = None
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32


def load(path=None):
    """Load libcgck.so (once).  Raises if it is missing: there is no fallback."""
    global _lib
    if _lib is None:
        _lib = bind(path or LIB_PATH)
    return _lib


def bind(path):
    """A ctypes binding of one libcgck.so build (tools/ab_inproc.py loads two
    builds into one process this way; everything else goes through load())."""
    if not os.path.exists(path):
        raise CgckError(f"libcgck.so not built at {path} (run make -C con-gen_amd)")
    L = ctypes.CDLL(path)
    L.in_cksum.restype = ctypes.c_uint16
    L.in_cksum.argtypes = [_vp, ctypes.c_int]
    L.udp_cksum.restype = ctypes.c_uint16
    L.udp_cksum.argtypes = [_vp, ctypes.c_int]
    L.cgck_last_error.restype = ctypes.c_char_p
    L.cgck_abi_version.restype = ctypes.c_int
    L.cgck_device_count.restype = ctypes.c_int
    L.cgck_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
    L.cgck_ctx_destroy.argtypes = [_vp]
    L.cgck_ctx_stream.restype = _vp
    L.cgck_ctx_stream.argtypes = [_vp]
    L.cgck_ctx_sync.argtypes = [_vp]
    L.cgck_ctx_set_kernel.argtypes = [_vp, ctypes.c_char_p]
    L.cgck_set_desc_len_hint.argtypes = [_vp, _u32]
    L.cgck_set_desc_layout.argtypes = [_vp, _u32]
    L.cgck_strided.argtypes = [_vp, _vp, _u64, _u64, _u32, _u32, _u32, _vp, _vp, _vp, _vp]
    L.cgck_desc.argtypes = [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp]
    L.cgck_desc_host.argtypes = [_vp, _vp, ctypes.c_size_t, _vp, _u64, _u32, _vp, _vp]
    L.cgck_host_register.argtypes = [_vp, ctypes.c_size_t]
    L.cgck_host_unregister.argtypes = [_vp]
    L.cgck_synth_strided.argtypes = [_vp, _vp, _u64, _u64, _u32, _u64, _vp]
    if hasattr(L, "cgck_synth_strided_ip6"):   # IPv6 addition (an older build loads without it)
        L.cgck_synth_strided_ip6.argtypes = [_vp, _vp, _u64, _u64, _u32, _u32, _u64, _vp]
    if hasattr(L, "cgck_synth_imix_ip6"):      # the IPv6 IMIX pair (an older build loads without it)
        L.cgck_synth_imix_ip6.argtypes = [_vp, _vp, _vp, _u64, _u32, _u64, _vp]
        L.cgck_synth_imix_ring_ip6.argtypes = [_vp, _vp, _vp, _u64, _u64, _u32, _u32, _u64, _vp]
    if hasattr(L, "cgck_synth_imix_dual"):     # the dual-stack IMIX set (an older build loads without it)
        L.cgck_synth_imix_dual.argtypes = [_vp, _vp, _vp, _u64, _u64, _u32, _u64, _vp]
    L.cgck_synth_imix.argtypes = [_vp, _vp, _vp, _u64, _u64, _vp]
    L.cgck_synth_imix_ring.argtypes = [_vp, _vp, _vp, _u64, _u64, _u32, _u64, _vp]
    L.cgck_imix_bytes.restype = _u64
    L.cgck_imix_bytes.argtypes = [_u64]
    L.cgck_dev_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(_vp)]
    L.cgck_dev_free.argtypes = [_vp]
    L.cgck_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(_vp)]
    L.cgck_host_free.argtypes = [_vp]
    L.cgck_memcpy.argtypes = [_vp, _vp, ctypes.c_size_t, _vp]
    L.cgck_memset.argtypes = [_vp, ctypes.c_int, ctypes.c_size_t, _vp]
    L.cgck_event_create.argtypes = [ctypes.POINTER(_vp)]
    L.cgck_event_destroy.argtypes = [_vp]
    L.cgck_event_record.argtypes = [_vp, _vp, _vp]
    L.cgck_event_elapsed_ms.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_float)]
    L.cgck_probe_read.argtypes = [_vp, _vp, _u64, _vp, _vp]
    L.toeplitz_hash.restype = _u32
    L.toeplitz_hash.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_int]
    L.rss_hash4.restype = _u32
    L.rss_hash4.argtypes = [_u32, _u32, ctypes.c_uint16, ctypes.c_uint16, _vp, ctypes.c_int]
    L.cgck_toeplitz.argtypes = [_vp, _vp, _u64, _u64, _u32, _vp, ctypes.c_int, _u32, _vp, _vp]
    if hasattr(L, "cgck_rss_desc"):            # the per-frame hash (an older build loads without it)
        _spec, _res = ctypes.POINTER(RssSpec), ctypes.POINTER(RssRes)
        L.cgck_rss_strided.argtypes = [_vp, _vp, _u64, _u64, _u32, _u32, _spec, _res, _vp]
        L.cgck_rss_desc.argtypes = [_vp, _vp, _vp, _u64, _spec, _res, _vp]
        L.cgck_rss_desc_host.argtypes = [_vp, _vp, ctypes.c_size_t, _vp, _u64, _spec, _res]
    if hasattr(L, "cgck_steer"):               # the partition by queue id (an older build loads without it)
        _spec, _res, _sres = ctypes.POINTER(RssSpec), ctypes.POINTER(RssRes), ctypes.POINTER(SteerRes)
        L.cgck_steer_work_bytes.restype = ctypes.c_size_t
        L.cgck_steer_work_bytes.argtypes = [_u64, _u32]
        L.cgck_steer.argtypes = [_vp, _vp, _u64, _u32, _vp, _sres, _vp, _vp]
        L.cgck_rss_steer_desc.argtypes = [_vp, _vp, _vp, _u64, _spec, _res, _sres, _vp, _vp]
        L.cgck_test_steer_plan.argtypes = [_u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                           ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(L, "cgck_l2_desc"):             # the raw-burst classifier (an older build loads without it)
        L.cgck_l2_desc.argtypes = [_vp, _vp, _vp, _u64, ctypes.POINTER(L2Res), _vp]
        L.cgck_synth_eth.argtypes = [_vp, _vp, _vp, _vp, _u64, _u32, _u64, _vp]
        L.cgck_test_l2_pass.argtypes = [_vp, ctypes.POINTER(_u64)]
    if hasattr(L, "cgck_l4_desc"):             # the segment parser (an older build loads without it)
        L.cgck_l4_desc.argtypes = [_vp, _vp, _vp, _u64, ctypes.POINTER(L4Res), _vp]
        L.cgck_test_l4_pass.argtypes = [_vp, ctypes.POINTER(_u64)]
    if hasattr(L, "cgck_l4_build"):            # the frame builder (an older build loads without it)
        L.cgck_l4_build.argtypes = [_vp, _vp, _u64, ctypes.POINTER(L4BuildIn), ctypes.POINTER(L4BuildRes), _vp]
        L.cgck_l4_build_hdr_bytes.restype = _u32
        L.cgck_l4_build_hdr_bytes.argtypes = [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]
        L.cgck_test_l4_build_pass.argtypes = [_vp, ctypes.POINTER(_u64)]
        L.cgck_test_l4_build_store.argtypes = [ctypes.c_int]
    if hasattr(L, "cgck_pcb_lookup"):          # the connection lookup (an older build loads without it)
        L.cgck_pcb_table_bytes.restype = ctypes.c_size_t
        L.cgck_pcb_table_bytes.argtypes = [_u32]
        L.cgck_pcb_build.argtypes = [_vp, ctypes.POINTER(Pcb), _vp, _vp]
        L.cgck_pcb_lookup.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, ctypes.POINTER(Pcb), ctypes.POINTER(PcbRes), _vp]
        L.cgck_test_pcb_pass.argtypes = [_vp, ctypes.POINTER(_u64)]
        L.cgck_test_pcb_mode.argtypes = [ctypes.c_int]
    if hasattr(L, "cgck_l4_reply"):            # tcp_respond's RSTs (an older build loads without them)
        _rin, _rres = ctypes.POINTER(L4ReplyIn), ctypes.POINTER(L4ReplyRes)
        L.cgck_l4_reply.argtypes = [_vp, _vp, _u64, _rin, _rres, _vp]
        L.cgck_l4_reply_packed.argtypes = [_vp, _vp, _u64, _rin, _rres, ctypes.POINTER(L4ReplyPack), _vp]
        L.cgck_l4_reply_rule.argtypes = [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                         _u32, _vp, _u32, ctypes.POINTER(Flow), _vp, _vp]
        L.cgck_test_l4_reply_pass.argtypes = [_vp, ctypes.POINTER(_u64)]
        L.cgck_test_l4_reply_store.argtypes = [ctypes.c_int]
    if hasattr(L, "cgck_test_rss_pass"):       # cgck_toeplitz's geometry (an older build loads without it)
        L.cgck_test_rss_pass.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.cgck_dst_cache.argtypes = [_vp, ctypes.POINTER(DstParams), _vp, _u32, _vp, _vp]
    L.cgck_dst_cache_host.argtypes = [_vp, ctypes.POINTER(DstParams), _vp, _u32,
                                      ctypes.POINTER(_u32)]
    L.cgck_burst_open.argtypes = [_vp, _u32, ctypes.c_size_t, _u32]
    L.cgck_burst_close.argtypes = [_vp]
    if hasattr(L, "cgck_burst_request"):   # ABI additions of round 4 (an older build loads without them)
        L.cgck_burst_request.argtypes = [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp]
        L.cgck_host_device_ptr.argtypes = [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]
    if hasattr(L, "cgck_test_burst_route"):
        L.cgck_test_burst_route.argtypes = [_u32, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _u64, _u32, _u64, _u32,
                                            _u32, ctypes.c_char_p, ctypes.c_size_t]
        L.cgck_test_burst_route_kind.argtypes = [_u32, ctypes.c_char_p, ctypes.c_size_t]
    L.cgck_thread_ctx.restype = _vp
    L.cgck_set_error_handler.restype = None
    L.cgck_set_error_handler.argtypes = [ERROR_FN, _vp]
    L.cgck_rx_begin.argtypes = [_vp, ctypes.c_size_t, _vp, _u64]
    if hasattr(L, "cgck_rx_post"):
        L.cgck_rx_post.argtypes = [_vp, ctypes.c_size_t, _vp, _u64]
    L.cgck_window_stats.argtypes = [ctypes.POINTER(_u64)]
    if hasattr(L, "cgck_window_stats_n"):   # ABI additions of round 6
        L.cgck_window_stats_n.argtypes = [ctypes.POINTER(_u64), ctypes.c_int]
        L.cgck_thread_bind.argtypes = [ctypes.c_int]
    L.cgck_ctx_last_kernel.restype = ctypes.c_char_p
    L.cgck_ctx_last_kernel.argtypes = [_vp]
    return L


def _check(rc, what):
    if rc < 0:
        msg = _lib.cgck_last_error().decode(errors="replace")
        raise CgckError(f"{what} failed ({rc}): {msg}")
    return rc


def device_count():
    return load().cgck_device_count()


# ---------------------------------------------------------------------------
# Drop-in interface (reference names and argument meaning).
# ---------------------------------------------------------------------------

def _addr(buf, off):
    if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8:
        raise TypeError("buf must be a numpy uint8 array")
    return buf.ctypes.data + off


def in_cksum(buf, off=0, n=None):
    """in_cksum(buf + off, n) — subr.c:186-195, on the GPU."""
    if n is None:
        n = len(buf) - off
    return load().in_cksum(_addr(buf, off), n)


def udp_cksum(buf, ip_off, n):
    """udp_cksum((struct ip *)(buf + ip_off), n) — subr.c:212-223, on the GPU."""
    return load().udp_cksum(_addr(buf, ip_off), n)


tcp_cksum = udp_cksum


def ip_cksum(buf, ip_off=0):
    """ip_cksum(ip) = in_cksum(ip, ip->ip_hl << 2) — subr.h:176."""
    return in_cksum(buf, ip_off, (int(buf[ip_off]) & 0x0F) << 2)


L4B_STORE_DEFAULT, L4B_STORE_DIRECT, L4B_STORE_TURNED = 0, 1, 2


def l4_build_store(shape):
    """cgck_test_l4_build_store: pin l4b_kernel's store shape for the process
    (L4B_STORE_*); returns the previous value."""
    return _check(load().cgck_test_l4_build_store(shape), "cgck_test_l4_build_store")


def l4_build_hdr_bytes(flow_flags, cls, opt):
    """cgck_l4_build_hdr_bytes: the bytes cgck_l4_build writes in front of the payload
    for a flow's flags, a class byte and a seg's opt; 0 when it refuses them."""
    return load().cgck_l4_build_hdr_bytes(flow_flags, cls, opt)


def pcb_table_bytes(nconn):
    """cgck_pcb_table_bytes: the bytes cgck_pcb_build's table needs for nconn entries
    (0 for nconn above 1 << 30)."""
    return load().cgck_pcb_table_bytes(nconn)


def pcb_mode(mode):
    """cgck_test_pcb_mode: pin the home slot (PCB_MODE_CHAIN) and the table shape
    (PCB_MODE_UNTAGGED) of every later pcb_build and pcb_lookup of the process;
    returns the previous value."""
    return _check(load().cgck_test_pcb_mode(mode), "cgck_test_pcb_mode")


def l4_reply_store(shape):
    """cgck_test_l4_reply_store: pin how l4r_kernel stores seg and flow under `at` for
    the process (L4R_STORE_*); returns the previous value."""
    return _check(load().cgck_test_l4_reply_store(shape), "cgck_test_l4_reply_store")


def l4_reply_rule(seg, ip, link, cls=SEG_TCP, kind=PCB_MISS, verdict=0, vmask=0, l2cls=0, flags=0, ip_len=None):
    """cgck_l4_reply_rule: the reply rule for one frame in host memory.  seg: a
    SEG_DTYPE record; ip: the frame's bytes from the IP header on (uint8 array; ip_len
    defaults to all of it); link: a FLOW_DTYPE record or Flow.  Returns (class byte,
    reply SEG_DTYPE record, reply FLOW_DTYPE record).  No device, no context."""
    s = np.array(seg, SEG_DTYPE).reshape(1)
    b = np.ascontiguousarray(ip, np.uint8)
    r, f = np.zeros(1, SEG_DTYPE), np.zeros(1, FLOW_DTYPE)
    lk = Flow.of(link)
    c = _check(load().cgck_l4_reply_rule(s.ctypes.data, cls, kind, verdict, vmask, l2cls, flags,
                                         b.ctypes.data if len(b) else None, len(b) if ip_len is None else ip_len,
                                         ctypes.byref(lk), r.ctypes.data, f.ctypes.data), "cgck_l4_reply_rule")
    return c, r[0], f[0]


def _u8(a):
    return np.ascontiguousarray(np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray))
                                else a, np.uint8)


def toeplitz_hash(data, key, cnt=None, key_size=None):
    """toeplitz_hash(data, cnt, key, key_size) — subr.c:482-502, on the GPU."""
    d, k = _u8(data), _u8(key)
    return load().toeplitz_hash(d.ctypes.data, len(d) if cnt is None else cnt, k.ctypes.data,
                                len(k) if key_size is None else key_size)


def rss_hash4(laddr, faddr, lport, fport, key, key_size=None):
    """rss_hash4(laddr, faddr, lport, fport, key, key_size) — subr.c:506-530
    (arguments in network order, as con-gen.c:338 passes them), on the GPU."""
    k = _u8(key)
    return load().rss_hash4(laddr, faddr, lport, fport, k.ctypes.data,
                            len(k) if key_size is None else key_size)


def burst_open(max_pkts=4096, max_bytes=4 << 20, idle_ms=0):
    """cgck_burst_open(NULL, ...): the resident burst server on this thread's
    drop-in context."""
    _check(load().cgck_burst_open(None, max_pkts, max_bytes, idle_ms), "cgck_burst_open")


def burst_close():
    _check(load().cgck_burst_close(None), "cgck_burst_close")


ROUTE_PAGEABLE, ROUTE_REGISTERED, ROUTE_REQUEST = 0, 1, 2


def burst_route(max_pkts, max_bytes, mem, lens, flags, posted=False, n1=0):
    """cgck_test_burst_route: the name of the route a request of packets of
    `lens` bytes takes on a server opened with (max_pkts, max_bytes); mem is
    ROUTE_PAGEABLE / ROUTE_REGISTERED (cgck_desc_host) or ROUTE_REQUEST
    (cgck_burst_request).  Needs no device."""
    lens = np.asarray(lens, np.int64)
    name = ctypes.create_string_buffer(64)
    rc = load().cgck_test_burst_route(max_pkts, max_bytes, mem, int(posted), len(lens), int(lens.max(initial=0)),
                                      int(((lens + 15) & ~15).sum()), flags, n1, name, len(name))
    if rc < 0:
        raise CgckError(f"cgck_test_burst_route failed ({rc})")
    return name.value.decode()


def burst_route_kinds():
    """cgck_test_burst_route_kind: {kind: a product request reaches it}."""
    kinds, buf, i = {}, ctypes.create_string_buffer(64), 0
    while (rc := load().cgck_test_burst_route_kind(i, buf, len(buf))) >= 0:
        kinds[buf.value.decode()] = bool(rc)
        i += 1
    return kinds


def steer_plan(n, queue_num):
    """cgck_test_steer_plan: (tile, tiles, work_bytes) of cgck_steer over n frames
    and queue_num queues.  Needs no device."""
    tile, tiles, work = _u32(), _u32(), ctypes.c_size_t()
    rc = load().cgck_test_steer_plan(n, queue_num, ctypes.byref(tile), ctypes.byref(tiles), ctypes.byref(work))
    if rc < 0:
        raise CgckError(f"cgck_test_steer_plan failed ({rc})")
    return tile.value, tiles.value, work.value


def steer_work_bytes(n, queue_num):
    """cgck_steer_work_bytes: the workspace cgck_steer needs (0: none, one tile).
    Needs no device."""
    return load().cgck_steer_work_bytes(n, queue_num)


def last_error():
    """cgck_last_error(): this thread's last error text."""
    return load().cgck_last_error().decode()


def host_device_ptr(arr, nbytes=None):
    """cgck_host_device_ptr: the device view of a registered numpy buffer."""
    p = _vp()
    _check(load().cgck_host_device_ptr(arr.ctypes.data, arr.nbytes if nbytes is None else nbytes,
                                       ctypes.byref(p)), "cgck_host_device_ptr")
    return p.value


def fn_pointers():
    """(in_cksum, udp_cksum) addresses in libcgck.so, for C harnesses that
    call the drop-in symbols (oracle.Port.replay_rx, oracle_cpu_bench)."""
    L = load()
    return (ctypes.cast(L.in_cksum, ctypes.c_void_p).value,
            ctypes.cast(L.udp_cksum, ctypes.c_void_p).value)


def rx_begin(base, desc):
    """cgck_rx_begin over a numpy byte array (the ring) and DESC_DTYPE
    descriptors (ip_len = bytes received after l3_off).  Returns the number
    of frames precomputed."""
    assert desc.dtype == DESC_DTYPE
    return _check(load().cgck_rx_begin(base.ctypes.data, base.nbytes, desc.ctypes.data, len(desc)),
                  "cgck_rx_begin")


def rx_end():
    """cgck_rx_end: returns how many drop-in calls the window answered."""
    return _check(load().cgck_rx_end(), "cgck_rx_end")


def rx_post(base, desc):
    """cgck_rx_post: post a burst (numpy ring + descriptors); returns the
    frames posted.  The ring and the descriptors' frames must stay unchanged
    until its window (rx_begin_posted .. rx_end) closes."""
    assert desc.dtype == DESC_DTYPE
    return _check(load().cgck_rx_post(base.ctypes.data, base.nbytes, desc.ctypes.data, len(desc)),
                  "cgck_rx_post")


def rx_begin_posted():
    """cgck_rx_begin_posted: open the window over the oldest posted burst."""
    return _check(load().cgck_rx_begin_posted(), "cgck_rx_begin_posted")


def rx_pending():
    """cgck_rx_pending: bursts posted and not yet opened (the drain rule)."""
    return _check(load().cgck_rx_pending(), "cgck_rx_pending")


def rx_ready():
    """cgck_rx_ready: 1 when the oldest posted burst's values are in, 0 while
    the GPU still computes it (no wait)."""
    return _check(load().cgck_rx_ready(), "cgck_rx_ready")


def tx_pending():
    """cgck_tx_pending: fills posted and not yet completed."""
    return _check(load().cgck_tx_pending(), "cgck_tx_pending")


def tx_ready():
    """cgck_tx_ready: 1 when the oldest posted fill's values are in (no wait)."""
    return _check(load().cgck_tx_ready(), "cgck_tx_ready")


def window_stats():
    """[rx served, rx synchronous, tx queued, tx synchronous] of this thread."""
    a = (_u64 * 4)()
    _check(load().cgck_window_stats(a), "cgck_window_stats")
    return list(a)


def window_stats_n():
    """window_stats() plus [4]: TX-window calls queued on a header of the
    last closed RX window's frames (cgck_window_stats_n)."""
    a = (_u64 * 8)()
    k = _check(load().cgck_window_stats_n(a, 8), "cgck_window_stats_n")
    return list(a)[:k]


def thread_bind(device):
    """cgck_thread_bind: this thread's drop-in context goes on `device`."""
    return _check(load().cgck_thread_bind(device), "cgck_thread_bind")


def thread_device():
    return load().cgck_thread_device()


_err_cb = None


def set_error_handler(fn):
    """cgck_set_error_handler: fn(what: str, msg: str) (None restores the
    default).  The drop-ins abort if the handler returns."""
    global _err_cb
    _err_cb = None if fn is None else ERROR_FN(lambda w, m, a: fn(w.decode(), m.decode()))
    load().cgck_set_error_handler(_err_cb if _err_cb is not None else ERROR_FN(), None)


def tx_begin():
    _check(load().cgck_tx_begin(), "cgck_tx_begin")


def tx_flush():
    return _check(load().cgck_tx_flush(), "cgck_tx_flush")


def tx_post():
    """cgck_tx_post: post the window's fill; returns the fields queued."""
    return _check(load().cgck_tx_post(), "cgck_tx_post")


def tx_complete():
    """cgck_tx_complete: wait for the oldest posted fill and write its fields."""
    return _check(load().cgck_tx_complete(), "cgck_tx_complete")


def thread_release():
    load().cgck_thread_release()


# ---------------------------------------------------------------------------
# Batched engine (device memory owned by the library).
# ---------------------------------------------------------------------------

class DeviceBuffer:
    def __init__(self, nbytes):
        L = load()
        p = _vp()
        _check(L.cgck_dev_alloc(nbytes, ctypes.byref(p)), "cgck_dev_alloc")
        self.ptr = p.value
        self.nbytes = nbytes

    def free(self):
        if self.ptr:
            load().cgck_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr, off=0, stream=None):
        arr = np.ascontiguousarray(arr)
        assert off + arr.nbytes <= self.nbytes
        _check(load().cgck_memcpy(self.ptr + off, arr.ctypes.data, arr.nbytes, stream), "upload")

    def download(self, arr, off=0, stream=None):
        assert arr.flags.c_contiguous and off + arr.nbytes <= self.nbytes
        _check(load().cgck_memcpy(arr.ctypes.data, self.ptr + off, arr.nbytes, stream), "download")


class Event:
    def __init__(self):
        p = _vp()
        _check(load().cgck_event_create(ctypes.byref(p)), "cgck_event_create")
        self.ptr = p.value

    def __del__(self):
        try:
            load().cgck_event_destroy(self.ptr)
        except Exception:
            pass


class Engine:
    """One context (stream + staging) on one device — use one per thread."""

    def __init__(self, device=0, kernel=None):
        L = load()
        p = _vp()
        _check(L.cgck_ctx_create(device, ctypes.byref(p)), "cgck_ctx_create")
        self.ctx = p.value
        self.device = device
        if kernel is not None:
            self.set_kernel(kernel)

    def set_kernel(self, family):
        """cgck_ctx_set_kernel: pin the kernel family by its name in kFamilyNames
        (csrc/cgck_params.h): "auto", "group", "lpp", "slot2", "lpa", "dstr", "lpd",
        "lpw"; the lab build also "slot", "str", "span", "slotd", "lpp<N>" and
        bare numbers."""
        _check(load().cgck_ctx_set_kernel(self.ctx, family.encode()), "cgck_ctx_set_kernel")

    def close(self):
        if self.ctx:
            load().cgck_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return load().cgck_ctx_stream(self.ctx)

    @property
    def last_kernel(self):
        """The kernel the dispatcher launched last on this context (the name
        rocprofv3 reports)."""
        return load().cgck_ctx_last_kernel(self.ctx).decode()

    def sync(self):
        _check(load().cgck_ctx_sync(self.ctx), "cgck_ctx_sync")

    def burst_open(self, max_pkts=4096, max_bytes=4 << 20, idle_ms=0):
        """cgck_burst_open: keep a burst server resident on this context."""
        _check(load().cgck_burst_open(self.ctx, max_pkts, max_bytes, idle_ms), "cgck_burst_open")

    def burst_close(self):
        _check(load().cgck_burst_close(self.ctx), "cgck_burst_close")

    def burst_request(self, dev_base, range_bytes, desc, flags, out=None, verdict=None):
        """cgck_burst_request: one request to the open server over device-visible
        memory [dev_base, +range_bytes); the server checks the descriptors.
        Returns the library's return code (0, -EIO refused, -ENOSPC)."""
        assert desc.dtype == DESC_DTYPE
        return load().cgck_burst_request(self.ctx, dev_base, range_bytes, desc.ctypes.data, len(desc), flags,
                                         None if out is None else out.ctypes.data,
                                         None if verdict is None else verdict.ctypes.data)

    def set_desc_len_hint(self, n):
        _check(load().cgck_set_desc_len_hint(self.ctx, n), "cgck_set_desc_len_hint")

    def set_desc_layout(self, layout):
        """cgck_set_desc_layout: LAYOUT_PACKED for descriptor batches whose
        frames lie back to back (lpw streams mid-size batches with or without
        it; a CGCK_STORE batch under it stays on slot2, without it takes lpf)."""
        _check(load().cgck_set_desc_layout(self.ctx, layout), "cgck_set_desc_layout")

    def strided(self, base, n, stride, l3_off, ip_len, flags, out=None, verdict=None, bad=None,
                stream=None):
        """Device pointers in, asynchronous (cgck_strided)."""
        _check(load().cgck_strided(self.ctx, base, n, stride, l3_off, ip_len, flags, out, verdict,
                                   bad, stream), "cgck_strided")

    def desc(self, base, desc, n, flags, out=None, verdict=None, bad=None, stream=None):
        _check(load().cgck_desc(self.ctx, base, desc, n, flags, out, verdict, bad, stream),
               "cgck_desc")

    def desc_host(self, base, desc, flags, out=None, verdict=None):
        """Host-resident batch (numpy): H2D, kernel, D2H.  Synchronous."""
        n = len(desc)
        assert desc.dtype == DESC_DTYPE
        _check(load().cgck_desc_host(self.ctx, base.ctypes.data, base.nbytes, desc.ctypes.data, n,
                                     flags, None if out is None else out.ctypes.data,
                                     None if verdict is None else verdict.ctypes.data),
               "cgck_desc_host")

    def synth_strided(self, base, n, stride, ip_len, seed, stream=None):
        _check(load().cgck_synth_strided(self.ctx, base, n, stride, ip_len, seed, stream),
               "cgck_synth_strided")

    def synth_strided_ip6(self, base, n, stride, ip_len, nh, seed, stream=None):
        """cgck_synth_strided_ip6: the synth_strided byte stream stamped as IPv6
        packets of next header nh (its checksum field zeroed)."""
        _check(load().cgck_synth_strided_ip6(self.ctx, base, n, stride, ip_len, nh, seed, stream),
               "cgck_synth_strided_ip6")

    def synth_imix(self, base, desc, n, seed, stream=None):
        _check(load().cgck_synth_imix(self.ctx, base, desc, n, seed, stream), "cgck_synth_imix")

    def synth_imix_ring(self, base, desc, n, stride, l3_off, seed, stream=None):
        """IMIX frames in ring slots (cgck_synth_imix_ring): n * stride bytes at base."""
        _check(load().cgck_synth_imix_ring(self.ctx, base, desc, n, stride, l3_off, seed, stream),
               "cgck_synth_imix_ring")

    def synth_imix_ip6(self, base, desc, n, nh, seed, stream=None):
        """cgck_synth_imix_ip6: the synth_imix set stamped as IPv6 packets of next
        header nh (its checksum field zeroed)."""
        _check(load().cgck_synth_imix_ip6(self.ctx, base, desc, n, nh, seed, stream), "cgck_synth_imix_ip6")

    def synth_imix_ring_ip6(self, base, desc, n, stride, l3_off, nh, seed, stream=None):
        """cgck_synth_imix_ring_ip6: the synth_imix_ring frames stamped as IPv6."""
        _check(load().cgck_synth_imix_ring_ip6(self.ctx, base, desc, n, stride, l3_off, nh, seed, stream),
               "cgck_synth_imix_ring_ip6")

    def synth_imix_dual(self, base, desc, n, seed, stride=0, l3_off=0, stream=None):
        """cgck_synth_imix_dual: the IMIX set, packed (stride 0) or in ring slots, with
        frame k IPv6 when k % 5 < 2 and its protocol by k % 7 (for MIXED batches)."""
        _check(load().cgck_synth_imix_dual(self.ctx, base, desc, n, stride, l3_off, seed, stream),
               "cgck_synth_imix_dual")

    def toeplitz(self, data, n, stride, cnt, key, out, mask=0xFFFFFFFF, key_size=None, stream=None):
        """cgck_toeplitz: device data/out, host key.  Asynchronous."""
        k = _u8(key)
        _check(load().cgck_toeplitz(self.ctx, data, n, stride, cnt, k.ctypes.data,
                                    len(k) if key_size is None else key_size, mask, out, stream),
               "cgck_toeplitz")

    def rss_pass(self):
        """cgck_test_rss_pass: (records one pass of toeplitz_kernel's grid covers on this
        device, 4-record groups the dense kernel's register ring holds before it wraps)."""
        r, g = _u64(0), _u64(0)
        _check(load().cgck_test_rss_pass(self.ctx, ctypes.byref(r), ctypes.byref(g)), "cgck_test_rss_pass")
        return r.value, g.value

    @staticmethod
    def rss_spec(key, mask=0xFFFFFFFF, hf=RSS_TCP | RSS_UDP, queue_num=0, key_size=None):
        """A cgck_rss_spec_t; the key array is kept alive with it."""
        k = _u8(key)
        s = RssSpec(k.ctypes.data, len(k) if key_size is None else key_size, mask, hf, queue_num)
        s._key_ref = k
        return s

    def rss_strided(self, base, n, stride, l3_off, ip_len, spec, hash=None, kind=None, queue=None,
                    qcount=None, stream=None):
        """cgck_rss_strided: device base and outputs (pointers or None).  Asynchronous."""
        res = RssRes(hash, kind, queue, qcount)
        _check(load().cgck_rss_strided(self.ctx, base, n, stride, l3_off, ip_len, ctypes.byref(spec),
                                       ctypes.byref(res), stream), "cgck_rss_strided")

    def rss_desc(self, base, desc, n, spec, hash=None, kind=None, queue=None, qcount=None, stream=None):
        """cgck_rss_desc: device base, descriptors and outputs.  Asynchronous."""
        res = RssRes(hash, kind, queue, qcount)
        _check(load().cgck_rss_desc(self.ctx, base, desc, n, ctypes.byref(spec), ctypes.byref(res), stream),
               "cgck_rss_desc")

    def rss_desc_host(self, base, desc, spec, hash=None, kind=None, queue=None, qcount=None):
        """cgck_rss_desc_host: a host-resident burst (numpy) hashed on the device;
        the outputs are numpy arrays or None, qcount is incremented.  Synchronous."""
        assert desc.dtype == DESC_DTYPE
        res = RssRes(*(None if a is None else a.ctypes.data for a in (hash, kind, queue, qcount)))
        _check(load().cgck_rss_desc_host(self.ctx, base.ctypes.data, base.nbytes, desc.ctypes.data, len(desc),
                                         ctypes.byref(spec), ctypes.byref(res)), "cgck_rss_desc_host")

    def steer(self, queue, n, queue_num, desc_in=None, qoff=None, perm=None, slot=None, desc_out=None,
              work=None, stream=None):
        """cgck_steer: the stable partition of n frames by their queue bytes; device
        pointers or None (work: at least steer_work_bytes(n, queue_num) bytes).
        Asynchronous."""
        res = SteerRes(qoff, perm, slot, desc_out)
        _check(load().cgck_steer(self.ctx, queue, n, queue_num, desc_in, ctypes.byref(res), work, stream),
               "cgck_steer")

    def rss_steer_desc(self, base, desc, n, spec, queue, hash=None, kind=None, qcount=None, qoff=None,
                       perm=None, slot=None, desc_out=None, work=None, stream=None):
        """cgck_rss_steer_desc: rss_desc into `queue` (required), then steer over
        it with spec.queue_num queues, on one stream.  Asynchronous."""
        rss, res = RssRes(hash, kind, queue, qcount), SteerRes(qoff, perm, slot, desc_out)
        _check(load().cgck_rss_steer_desc(self.ctx, base, desc, n, ctypes.byref(spec), ctypes.byref(rss),
                                          ctypes.byref(res), work, stream), "cgck_rss_steer_desc")

    def l2_desc(self, base, raw, n, desc_out=None, cls=None, count=None, stream=None):
        """cgck_l2_desc: classify n raw Ethernet frames (raw: {frame_off, offset of
        the Ethernet header, bytes delivered}) and write the trimmed descriptors,
        the class bytes and / or the running counters; device pointers or None.
        Asynchronous."""
        res = L2Res(desc_out, cls, count)
        _check(load().cgck_l2_desc(self.ctx, base, raw, n, ctypes.byref(res), stream), "cgck_l2_desc")

    def l2_pass_frames(self):
        """cgck_test_l2_pass: frames one pass of l2d_kernel's grid covers on this device."""
        f = _u64()
        _check(load().cgck_test_l2_pass(self.ctx, ctypes.byref(f)), "cgck_test_l2_pass")
        return f.value

    def l4_desc(self, base, desc, n, seg=None, cls=None, hash=None, count=None, stream=None):
        """cgck_l4_desc: per-frame TCP / UDP segment records of n described frames;
        each output is optional (seg: SEG_DTYPE[n], 16-byte aligned; cls: u8[n];
        hash: u32[n]; count: u32[SEG_NCOUNT], accumulated)."""
        res = L4Res(seg, cls, hash, count)
        _check(load().cgck_l4_desc(self.ctx, base, desc, n, ctypes.byref(res), stream), "cgck_l4_desc")

    def l4_pass_frames(self):
        """cgck_test_l4_pass: frames one pass of l4d_kernel's grid covers on this device."""
        f = _u64()
        _check(load().cgck_test_l4_pass(self.ctx, ctypes.byref(f)), "cgck_test_l4_pass")
        return f.value

    def l4_build(self, base, n, slot, seg, flow, nflow, cls=None, fidx=None, ip_id0=0, ip_off=0, raw_out=None,
                 desc_out=None, cls_out=None, count=None, stream=None):
        """cgck_l4_build: Ethernet + IP + TCP / UDP headers of n frames written into the
        slots `slot` describes, from seg (SEG_DTYPE[n]) and flow (FLOW_DTYPE[nflow])
        records; device pointers or None (cls: every frame TCP; fidx: frame k uses
        flow[k]).  Each output is optional (raw_out, desc_out: DESC_DTYPE[n]; cls_out:
        u8[n]; count: u32[BLD_NCOUNT], accumulated).  Asynchronous."""
        arg = L4BuildIn(slot, seg, cls, flow, fidx, nflow, ip_id0, ip_off)
        res = L4BuildRes(raw_out, desc_out, cls_out, count)
        _check(load().cgck_l4_build(self.ctx, base, n, ctypes.byref(arg), ctypes.byref(res), stream), "cgck_l4_build")

    def l4_build_pass_frames(self):
        """cgck_test_l4_build_pass: frames one pass of l4b_kernel's grid covers on this device."""
        f = _u64()
        _check(load().cgck_test_l4_build_pass(self.ctx, ctypes.byref(f)), "cgck_test_l4_build_pass")
        return f.value

    def pcb_build(self, pcb, stat=None, stream=None):
        """cgck_pcb_build: the device hash table of pcb (a Pcb) from its connection
        records; stat: u32[4], written.  Asynchronous."""
        _check(load().cgck_pcb_build(self.ctx, ctypes.byref(pcb), stat, stream), "cgck_pcb_build")

    def pcb_lookup(self, base, desc, seg, n, pcb, cls=None, idx=None, fidx=None, kind=None, count=None, stream=None):
        """cgck_pcb_lookup: the connection of each of the n frames desc and seg
        (cgck_l4_desc's records) describe, against pcb's table; each output is optional
        (idx, fidx: u32[n]; kind: u8[n]; count: u32[PCB_NCOUNT], accumulated).
        Asynchronous."""
        res = PcbRes(idx, fidx, kind, count)
        _check(load().cgck_pcb_lookup(self.ctx, base, desc, seg, cls, n, ctypes.byref(pcb), ctypes.byref(res), stream),
               "cgck_pcb_lookup")

    def pcb_pass_frames(self):
        """cgck_test_pcb_pass: frames one pass of pcbl_kernel's grid covers on this device."""
        f = _u64(0)
        _check(load().cgck_test_pcb_pass(self.ctx, ctypes.byref(f)), "cgck_test_pcb_pass")
        return f.value

    @staticmethod
    def _l4_reply_args(desc, seg, link, cls, kind, verdict, l2cls, at, vmask, flags, seg_out, flow_out, cls_out,
                       queue, count):
        arg = L4ReplyIn(desc, seg, cls, kind, verdict, l2cls, at, Flow.of(link), vmask, flags)
        return arg, L4ReplyRes(seg_out, flow_out, cls_out, queue, count)

    def l4_reply(self, base, n, desc, seg, link, cls=None, kind=None, verdict=None, l2cls=None, at=None, vmask=0,
                 flags=0, seg_out=None, flow_out=None, cls_out=None, queue=None, count=None, stream=None):
        """cgck_l4_reply: tcp_respond's RST records for the n received frames desc and
        seg (cgck_l4_desc's records) describe; device pointers or None (cls: every
        frame TCP; kind: every frame a MISS; verdict, l2cls: 0; at: frame k's outputs go
        to index k).  link: a FLOW_DTYPE record or Flow, the replies' link header.  Each
        output is optional (seg_out: SEG_DTYPE[n]; flow_out: FLOW_DTYPE[n]; cls_out,
        queue: u8[n]; count: u32[RPL_NCOUNT], accumulated).  Asynchronous."""
        arg, res = self._l4_reply_args(desc, seg, link, cls, kind, verdict, l2cls, at, vmask, flags, seg_out, flow_out,
                                       cls_out, queue, count)
        _check(load().cgck_l4_reply(self.ctx, base, n, ctypes.byref(arg), ctypes.byref(res), stream), "cgck_l4_reply")

    def l4_reply_packed(self, base, n, desc, seg, link, pk_queue, pk_at, pk_qoff, work=None, cls=None, kind=None,
                        verdict=None, l2cls=None, vmask=0, flags=0, seg_out=None, flow_out=None, cls_out=None,
                        queue=None, count=None, stream=None):
        """cgck_l4_reply_packed: the RSTs first and in arrival order (the reference's
        slot and ip_id order).  pk_queue: u8[n], pk_at: u32[n], pk_qoff: u32[3] (qoff[1]
        = the number of RSTs), work: steer_work_bytes(n, 1) bytes or None; the rest as
        l4_reply.  Asynchronous."""
        arg, res = self._l4_reply_args(desc, seg, link, cls, kind, verdict, l2cls, None, vmask, flags, seg_out, flow_out,
                                       cls_out, queue, count)
        pk = L4ReplyPack(pk_queue, pk_at, pk_qoff, work)
        _check(load().cgck_l4_reply_packed(self.ctx, base, n, ctypes.byref(arg), ctypes.byref(res), ctypes.byref(pk),
                                           stream), "cgck_l4_reply_packed")

    def l4_reply_pass_frames(self):
        """cgck_test_l4_reply_pass: frames one pass of l4r_kernel's grid covers on this device."""
        f = _u64(0)
        _check(load().cgck_test_l4_reply_pass(self.ctx, ctypes.byref(f)), "cgck_test_l4_reply_pass")
        return f.value

    def synth_eth(self, base, desc, raw, n, vlan_every, seed, stream=None):
        """cgck_synth_eth: Ethernet headers (a VLAN tag on every vlan_every-th frame)
        in front of a ring set's IP headers, and the transport's descriptors in raw."""
        _check(load().cgck_synth_eth(self.ctx, base, desc, raw, n, vlan_every, seed, stream), "cgck_synth_eth")

    @staticmethod
    def dst_params(laddr, faddr, fport, queue_num, queue_id, key=None, key_size=None):
        """laddr/faddr = (min, max) host order; fport network order.  The key
        array must stay alive while the params are used."""
        k = None if key is None else _u8(key)
        p = DstParams(laddr[0], laddr[1], faddr[0], faddr[1], fport, queue_num, queue_id,
                      None if k is None else k.ctypes.data,
                      0 if k is None else (len(k) if key_size is None else key_size))
        p._key_ref = k
        return p

    def dst_cache(self, params, out, cap, count, stream=None):
        """cgck_dst_cache: device out/count, asynchronous."""
        _check(load().cgck_dst_cache(self.ctx, ctypes.byref(params), out, cap, count, stream),
               "cgck_dst_cache")

    def dst_cache_host(self, params, cap):
        """cgck_dst_cache_host: returns the DST_DTYPE entries written."""
        out = np.zeros(cap, DST_DTYPE)
        got = _u32()
        _check(load().cgck_dst_cache_host(self.ctx, ctypes.byref(params), out.ctypes.data, cap,
                                          ctypes.byref(got)), "cgck_dst_cache_host")
        return out[:got.value]

    def probe_read(self, src, nbytes, sink, stream=None):
        _check(load().cgck_probe_read(self.ctx, src, nbytes, sink, stream), "cgck_probe_read")

    def record(self, ev, stream=None):
        _check(load().cgck_event_record(self.ctx, ev.ptr, stream), "cgck_event_record")

    @staticmethod
    def elapsed_ms(a, b):
        ms = ctypes.c_float()
        _check(load().cgck_event_elapsed_ms(a.ptr, b.ptr, ctypes.byref(ms)), "elapsed")
        return ms.value

    # -- numpy conveniences (tests) --
    def run_host_strided(self, buf, n, stride, l3_off, ip_len, flags, want_verdict=True):
        """Copy a host batch to the device, run cgck_strided, copy results (and,
        with STORE, the bytes) back.  Returns (out, verdict); verdict is None
        when want_verdict is False (no verdict array passed to the library)."""
        d = DeviceBuffer(max(buf.nbytes, 1))
        o = DeviceBuffer(4 * max(n, 1))
        v = DeviceBuffer(max(n, 1))
        d.upload(buf, stream=self.stream)
        self.strided(d.ptr, n, stride, l3_off, ip_len, flags, o.ptr, v.ptr if want_verdict else None, None)
        out = np.zeros(n, np.uint32)
        ver = np.zeros(n, np.uint8) if want_verdict else None
        o.download(out, stream=self.stream)
        if want_verdict:
            v.download(ver, stream=self.stream)
        if flags & STORE:
            d.download(buf, stream=self.stream)
        self.sync()
        return out, ver

    def run_host_desc(self, buf, desc, flags):
        n = len(desc)
        d = DeviceBuffer(max(buf.nbytes, 1))
        dd = DeviceBuffer(max(desc.nbytes, 12))
        o = DeviceBuffer(4 * max(n, 1))
        v = DeviceBuffer(max(n, 1))
        d.upload(buf, stream=self.stream)
        dd.upload(desc, stream=self.stream)
        self.desc(d.ptr, dd.ptr, n, flags, o.ptr, v.ptr, None)
        out = np.zeros(n, np.uint32)
        ver = np.zeros(n, np.uint8)
        o.download(out, stream=self.stream)
        v.download(ver, stream=self.stream)
        if flags & STORE:
            d.download(buf, stream=self.stream)
        self.sync()
        return out, ver
