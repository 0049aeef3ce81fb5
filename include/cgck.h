/*
 * cgck.h — C-ABI of the MI355X (gfx950) Internet-checksum engine that stands in
 * for con-gen's checksum unit (reference: kogdenko/con-gen, subr.c:119-223).
 *
 * Two layers, one shared library (libcgck.so):
 *
 *  1. Drop-in symbols.  `in_cksum` and `udp_cksum` keep the exact prototypes of
 *     subr.h:373-374 (and therefore the `ip_cksum` / `tcp_cksum` macros of
 *     subr.h:176-177 keep working unchanged).  They are synchronous: each call
 *     runs the gfx950 kernel on the calling thread's own context (stream +
 *     pinned staging) and returns the host-order u16 the call sites store
 *     verbatim into the header.  Inside a deferred TX window
 *     (cgck_tx_begin .. cgck_tx_flush) the same symbols queue the packet and
 *     return 0; the flush fills every queued field in one batched launch
 *     (the bsd_flush / toy_flush batch point).
 *
 *  2. Batched API (`cgck_*`).  Packet batches described either by a fixed
 *     stride or by 12-byte descriptors, device-resident (all pointers are
 *     device pointers) or host-resident (pinned staging, H2D + kernel + D2H).
 *     Every entry point returns 0 or a negative errno and never aborts.
 *
 * Semantics (bit-exact with the reference on the same bytes):
 *   S   = sum of the region's little-endian 16-bit words counted from the
 *         region's first byte (odd trailing byte = low byte), plus the
 *         12-byte pseudo-header for L4 (subr.c:119-125, 197-210);
 *   out = (S mod 65535 == 0) ? 0xFFFF : 0xFFFF - (S mod 65535)
 *         (reduce(), subr.c:137-156: a folded sum of 0 maps to 0xFFFF).
 *
 * No HIP or torch types appear in any signature: streams are `void *`
 * (a hipStream_t, or NULL for the context's own stream).
 */
#ifndef CGCK_H
#define CGCK_H

#include <stdint.h>
#include <stddef.h>
#include <netinet/ip.h> /* struct ip, as subr.h:29 uses it */

#ifdef __cplusplus
extern "C" {
#endif

#define CGCK_ABI_VERSION 2

/* ------------------------------------------------------------------------ */
/* 1. Drop-in symbols (subr.h:373-374; bodies subr.c:186-195, 212-223).     */
/* ------------------------------------------------------------------------ */

/* Checksum of [data, data+len).  ip_cksum(ip) == in_cksum(ip, ip->ip_hl<<2)
 * (subr.h:176).  Callers: ip_output.c:63, ip_input.c:51, ip_icmp.c:77,191,
 * gbtcp/inet.c:322, gbtcp/tcp.c:374. */
uint16_t in_cksum(void *data, int len);

/* TCP/UDP checksum: `len` bytes at ip + ip_hl*4 plus the pseudo-header
 * {ip_src, ip_dst, 0, ip_p, htons(len)}.  tcp_cksum == udp_cksum (subr.h:177).
 * Callers: tcp_output.c:417, tcp_input.c:78, tcp_subr.c:122,
 * udp_usrreq.c:89,189, gbtcp/inet.c:145, gbtcp/tcp.c:377. */
uint16_t udp_cksum(struct ip *ip, int len);

/* ------------------------------------------------------------------------ */
/* 2. Batched API.                                                           */
/* ------------------------------------------------------------------------ */

typedef struct cgck_ctx cgck_ctx_t;

/* One packet of a descriptor batch: the IPv4 header sits at
 * base + frame_off + l3_off; ip_len bytes of datagram follow it
 * (ip_hl*4 header bytes + the L4 region).  12 bytes, 4-byte aligned. */
typedef struct cgck_desc {
	uint64_t frame_off; /* byte offset of the frame from the batch base   */
	uint16_t l3_off;    /* IPv4 header offset inside the frame (14: Ethernet) */
	uint16_t ip_len;    /* datagram bytes covered (IPv4 total length)      */
} __attribute__((packed, aligned(4))) cgck_desc_t;

/* Operation flags. */
enum {
	CGCK_RAW         = 1u << 0, /* out.lo = in_cksum(ip, ip_len): whole region, no header semantics */
	CGCK_IP          = 1u << 1, /* out.lo = ip_cksum(ip) = in_cksum(ip, ip_hl<<2) */
	CGCK_L4          = 1u << 2, /* out.hi = udp_cksum(ip, ip_len - ip_hl*4) (pseudo-header) */
	CGCK_L4_NOPSEUDO = 1u << 3, /* with CGCK_L4: out.hi = in_cksum(ip+hl, ip_len-hl) (ICMP, ip_icmp.c:77,191) */
	CGCK_ZERO_FIELDS = 1u << 4, /* read the checksum fields as zero: ip+10 and the L4 field by ip_p
	                               (TCP +16, UDP +6, ICMP +2 after the header) — the "field = 0,
	                               recompute" step every call site performs */
	CGCK_STORE       = 1u << 5, /* write out.lo to ip+10 and out.hi to the L4 field (TX fill).  The
	                               frames of a CGCK_STORE batch must not overlap: the order
	                               between packets is unspecified */
	CGCK_VERIFY      = 1u << 6, /* compare with the stored fields (implies ZERO_FIELDS), verdict bits */
	CGCK_V_IP_ZERO_IS_FFFF = 1u << 7, /* bsd44 ip_input.c:46-48: a received ip_sum of 0 counts as 0xFFFF */
	CGCK_V_UDP_ZERO_SKIP   = 1u << 8, /* udp_usrreq.c:86: uh_sum == 0 means "not checksummed" */
	CGCK_IP6         = 1u << 9, /* the record at l3_off is an IPv6 header (40 bytes); see below */
	CGCK_MIXED       = 1u << 10, /* each record is IPv4 or IPv6 by its own version nibble; see below */
};
/* CGCK_IP6.  ip_len (descriptor or strided argument) is the bytes covered from
 * the first header byte, 40 + payload, at most 65535 (no jumbograms); the
 * header's own payload-length field is not consulted.  The other flags keep
 * their meaning:
 *   CGCK_RAW   unchanged (in_cksum of the whole region).
 *   CGCK_IP    accepted and inert: IPv6 has no header checksum, so out.lo = 0,
 *              CGCK_BAD_IP is never set and nothing is stored at +10
 *              (CGCK_V_IP_ZERO_IS_FFFF is inert too).  The GEN_BOTH / FILL_BOTH
 *              / VERIFY_* sets therefore work with `| CGCK_IP6`.
 *   CGCK_L4    out.hi = the upper-layer checksum.  The L4 header is found from
 *              l4_off = 40, nh = byte 6: Hop-by-Hop (0), Routing (43) and
 *              Destination Options (60) advance by (b[1] + 1) * 8, AH (51) by
 *              (b[1] + 2) * 4, at most 8 extension headers.  A Fragment header
 *              (44) means the packet has no L4 result: out.hi = 0, nothing
 *              stored or compared, no bad bit.  Any other value is the
 *              terminal nh.  The sum covers the ip_len - l4_off bytes at l4_off
 *              plus the 40-byte pseudo-header {src, dst (header bytes 8..39),
 *              the upper-layer length as 32 bits big-endian, three zero bytes,
 *              nh} (RFC 8200 §8.1).  Checksum fields: TCP (6) +16, UDP (17) +6,
 *              ICMPv6 (58) +2 after l4_off; any other terminal nh (59 and
 *              unknown ones included) has no field: its sum is still returned
 *              in out.hi, nothing is zeroed, stored or compared.
 *   CGCK_ZERO_FIELDS, CGCK_STORE, CGCK_VERIFY, CGCK_V_UDP_ZERO_SKIP
 *              as for IPv4, on the field found above (V_UDP_ZERO_SKIP is
 *              honoured as given: an IPv6 caller leaves it out, RFC 8200 §8.1).
 *   CGCK_L4_NOPSEUDO | CGCK_IP6 is -EINVAL.
 * CGCK_BAD_LEN: ip_len < 40, or, with CGCK_L4, an extension header (its first
 * two bytes), the start of the L4 region or the checksum field the chain names
 * lies past ip_len, or there is a ninth extension header; out = 0, nothing
 * stored, not counted as bad.
 * Accepted by cgck_strided, cgck_desc and cgck_desc_host (with a burst server
 * open such a batch takes the launch path); cgck_burst_request refuses it with
 * -EINVAL.  The RX / TX windows and the drop-in symbols remain IPv4.
 * Native kernels (every other batch runs in the group kernel's IPv6 variant,
 * cksum6, which has the full semantics): dense strided frames of 1 KiB and more
 * and aligned strided 40..64 B frames with CGCK_IP / CGCK_L4 only (dstr6; lpd6,
 * lpa6); and, through cgck_desc, cgck_desc_host or cgck_strided, mixed-length
 * or mid-size batches (a length hint or ip_len of 256..1023 B: a receive burst
 * copied back to back or left in ring slots) with any flags but CGCK_STORE and
 * no `bad` counters (lpw6, streamed through LDS like IPv4's lpw). */
/* CGCK_MIXED.  A receive burst as it comes off a ring: IPv4 and IPv6 frames,
 * TCP, UDP, ICMP / ICMPv6 and the odd ARP frame in one batch and one call, with
 * no host-side sort by family.  Each packet is judged by v, the high nibble of
 * its first byte; ip_len is the bytes covered from the first header byte, as for
 * either family (at most 65535 for a strided batch).
 *   ip_len == 0   verdict CGCK_BAD_LEN, out = 0.
 *   v == 4        the IPv4 semantics of the other flags, exactly as without
 *                 CGCK_MIXED, except that the L4 result follows the packet's own
 *                 ip_p: ip_p == 1 (ICMP) is computed as under CGCK_L4_NOPSEUDO,
 *                 in_cksum(ip + hl, ip_len - hl) with its field at +2; every
 *                 other protocol with the pseudo-header.  IPv4's BAD_LEN rules.
 *   v == 6        the CGCK_IP6 semantics above for that packet: CGCK_IP inert
 *                 (out.lo = 0, never CGCK_BAD_IP), the extension-header walk,
 *                 the Fragment rule, the field by the terminal nh and the
 *                 BAD_LEN rules unchanged.
 *   any other v   out = 0, verdict CGCK_NOT_IP; nothing compared or counted.
 * CGCK_V_IP_ZERO_IS_FFFF applies to the IPv4 packets (inert for IPv6 anyway).
 * CGCK_V_UDP_ZERO_SKIP applies to the IPv4 packets only: RFC 8200 §8.1 forbids
 * a zero UDP checksum over IPv6, so such a packet is compared and comes out
 * CGCK_BAD_L4 (under CGCK_IP6 alone the flag is honoured as given).
 * `bad` counters: [0] += bad IPv4 header sums, [1] += bad L4 sums of either
 * family.
 * -EINVAL: CGCK_MIXED with CGCK_RAW, CGCK_IP6, CGCK_L4_NOPSEUDO or CGCK_STORE,
 * or a strided ip_len > 65535.  CGCK_STORE is out of scope on purpose: a
 * transmit path knows what it built, and sorts its fills by family for free.
 * Accepted by cgck_strided, cgck_desc (any 4-byte aligned descriptor array) and
 * cgck_desc_host (with a burst server open such a batch takes the launch path);
 * cgck_burst_request refuses it with -EINVAL.  The RX / TX windows and the
 * drop-in symbols are untouched.  One kernel serves every such batch
 * (lpwx_kernel: lpw's pipeline with the finish chosen per lane), whatever its
 * lengths and whatever family is pinned; any length is exact.  Measured on 16M
 * IMIX frames, two in five IPv6, against two calls over host-sorted descriptor
 * arrays (lpw + lpw6, the sort itself not timed): 0.83 of their time on frames
 * copied back to back, but 1.05 on frames left in 2048-byte ring slots, where
 * the one call is the slower route by more than the run's 1.2 % margin (its
 * second finish costs 4 % over lpw).  The two-call route needs
 * every packet's first bytes on the host. */
#define CGCK_GEN_BOTH   (CGCK_IP | CGCK_L4)
#define CGCK_FILL_BOTH   (CGCK_IP | CGCK_L4 | CGCK_ZERO_FIELDS | CGCK_STORE)
#define CGCK_VERIFY_BSD  (CGCK_IP | CGCK_L4 | CGCK_VERIFY | CGCK_V_IP_ZERO_IS_FFFF | CGCK_V_UDP_ZERO_SKIP)
#define CGCK_VERIFY_TOY  (CGCK_IP | CGCK_L4 | CGCK_VERIFY)

/* Verdict bits (one byte per packet). */
enum {
	CGCK_BAD_IP  = 1u << 0, /* -> ips_badsum    (netstat.h:40)  */
	CGCK_BAD_L4  = 1u << 1, /* -> tcps_rcvbadsum / udps_badsum (netstat.h:103,129) */
	CGCK_BAD_LEN = 1u << 2, /* header modes only: ip_len < 20 or ip_len < ip_hl*4
	                           (ip_input.c:24-37 drops these before any checksum):
	                           out = 0, nothing stored, not counted as bad
	                           (CGCK_IP6: see that flag) */
	CGCK_NOT_IP  = 1u << 3, /* CGCK_MIXED only: the record's version nibble is neither 4 nor 6
	                           (an ARP frame, say): out = 0, nothing compared or counted */
};

/* Error codes are negative errno values; this gives a thread-local message. */
const char *cgck_last_error(void);
int cgck_abi_version(void);

/* Contexts: one per calling thread (a HIP stream, pinned staging, scratch).
 * A context is never shared between threads without external locking. */
int cgck_ctx_create(int device, cgck_ctx_t **out);
int cgck_ctx_destroy(cgck_ctx_t *ctx);
void *cgck_ctx_stream(cgck_ctx_t *ctx);
int cgck_ctx_sync(cgck_ctx_t *ctx);
/* Pin the context's kernel family instead of the dispatcher's choice (parity
 * tests of every family, A/B runs): "auto" (the default), "group", "lpp",
 * "lpa", "slot2", "dstr", "lpd", "lpw" ("lpw" covers its fill / counter
 * variant for IPv4, lpf_kernel, which takes the batches with CGCK_STORE or a
 * `bad` pointer).  A family that cannot take a batch
 * (alignment, flags, lengths) still falls back to one that can, so results
 * stay exact; a CGCK_IP6 batch runs in the family's IPv6 variant ("dstr",
 * "lpd", "lpa", "lpw", "group") or, where there is none or it cannot take the
 * batch, in the group kernel's.  A CGCK_MIXED batch ignores the pin: one
 * kernel, lpwx_kernel, serves all of them.  -EINVAL for an unknown name. */
int cgck_ctx_set_kernel(cgck_ctx_t *ctx, const char *family);

/* Device-resident batches.  `out` (u32 per packet: lo16 = IP/RAW result,
 * hi16 = L4 result), `verdict` (u8 per packet) and `bad` (u32[2] running
 * counters: [0] += bad IP, [1] += bad L4) are optional (NULL).  `stream`
 * NULL = the context's stream.  Asynchronous: returns after the launch. */
int cgck_strided(cgck_ctx_t *ctx, void *base, uint64_t n, uint64_t stride,
		 uint32_t l3_off, uint32_t ip_len, uint32_t flags,
		 uint32_t *out, uint8_t *verdict, uint32_t *bad, void *stream);
int cgck_desc(cgck_ctx_t *ctx, void *base, const cgck_desc_t *desc, uint64_t n,
	      uint32_t flags, uint32_t *out, uint8_t *verdict, uint32_t *bad,
	      void *stream);

/* Shape hint for descriptor batches: their typical (mean) ip_len, default
 * 1500.  Below 1 KiB the lane-per-packet kernel is used (mixed/small packets,
 * e.g. IMIX = 354), from 1 KiB the lane-group kernel.  From 256 B to 1 KiB
 * the batch streams through LDS (lpw); so does an IPv4 transmit fill
 * (CGCK_STORE) or a verify with `bad` counters (lpf, the same pipeline with
 * those side effects), except a CGCK_STORE batch under CGCK_LAYOUT_PACKED,
 * which gathers in registers (slot2), the faster of the two on packed frames.
 * Any length is still handled correctly; the hint only picks the faster
 * kernel. */
int cgck_set_desc_len_hint(cgck_ctx_t *ctx, uint32_t max_ip_len);

/* Layout hint for descriptor batches.  CGCK_LAYOUT_PACKED: the frames of a
 * batch lie back to back in descriptor order (a receive burst copied into
 * one buffer, the IMIX set of BASELINE configs[3]); the dispatcher then
 * streams the buffer itself (contiguous DMA through LDS) instead of gathering
 * each frame, for mixed lengths below 1 KiB.  Results are exact for any
 * layout: 64-frame steps that are not back to back are computed frame by
 * frame, only slower.  Default CGCK_LAYOUT_ANY. */
enum { CGCK_LAYOUT_ANY = 0, CGCK_LAYOUT_PACKED = 1 };
int cgck_set_desc_layout(cgck_ctx_t *ctx, uint32_t layout);

/* Host-resident batch (ring memory), synchronous.  Registered memory
 * (cgck_host_register) is read where it lies and in-place stores land there;
 * a small pageable burst (packet bytes <= 512 KiB) is copied packet by packet
 * into pinned staging that the kernel reads; a larger pageable batch goes by
 * DMA of [base, base+bytes).  Results come back to out/verdict (and, with
 * CGCK_STORE, the filled fields into `base`).  -EINVAL when a descriptor
 * reaches past `bytes`. */
int cgck_desc_host(cgck_ctx_t *ctx, void *base, size_t bytes,
		   const cgck_desc_t *desc, uint64_t n, uint32_t flags,
		   uint32_t *out, uint8_t *verdict);

/* Zero-copy ring memory: page-lock a transport's
 * buffer pool (netmap slots, XDP UMEM, DPDK mempool) so H2D copies read it
 * directly.  Thin wrappers of hipHostRegister / hipHostUnregister. */
int cgck_host_register(void *ptr, size_t bytes);
int cgck_host_unregister(void *ptr);
/* The device view of [ptr, ptr + bytes) inside a range registered with
 * cgck_host_register (for cgck_burst_request); -ENOENT otherwise. */
int cgck_host_device_ptr(const void *ptr, size_t bytes, void **dev);

/* The drop-in symbols run on a per-thread context created on first use
 * (device from $CGCK_DEVICE, default 0).  cgck_thread_ctx returns that
 * context (creating it), so a worker's batched calls (cgck_desc_host,
 * cgck_dst_cache_host, ...) share its stream and staging with the drop-ins;
 * NULL on failure (cgck_last_error says why).  A worker thread that exits
 * calls cgck_thread_release to free it. */
cgck_ctx_t *cgck_thread_ctx(void);
int cgck_thread_release(void);

/* Per-thread device binding (one host thread per device).  A
 * worker calls cgck_thread_bind(queue_id % cgck_device_count()) in its
 * thread_init (con-gen.c:1062-1100 starts one worker per RSS queue, up to
 * N_THREADS_MAX = 32, subr.h:58) before its first checksum call; its
 * drop-in context, windows and burst server then live on that device.  The
 * binding outlives cgck_thread_release.  -EINVAL: no such device; -EBUSY:
 * the thread's context already exists on another device (release it first).
 * cgck_thread_device returns the device the thread's context is (or will be)
 * on. */
int cgck_thread_bind(int device);
int cgck_thread_device(void);

/* The drop-in symbols have no error channel (their prototypes are the
 * reference's).  When one cannot produce a result (no device, a launch or
 * synchronisation failure) it calls the handler set here with what failed
 * and cgck_last_error()'s text — con-gen passes a function that ends in its
 * panic3() (subr.c:238-261), which prints the stats and exits.  If the
 * handler returns, or none is set, the library prints the message and
 * aborts.  Process-wide; NULL restores the default. */
typedef void (*cgck_error_fn)(const char *what, const char *msg, void *arg);
void cgck_set_error_handler(cgck_error_fn fn, void *arg);

/* RX window at the transport's receive burst.
 * cgck_rx_begin computes, for every frame of the burst in one launch, the
 * values the stack's own verifiers are about to ask for — ip_cksum of the
 * header with ip_sum read as zero (ip_input.c:49-51, gbtcp/inet.c:319-322)
 * and the L4 checksum with its field read as zero: tcp_cksum / udp_cksum of
 * the segment (tcp_input.c:75-78, udp_usrreq.c:86-89, gbtcp/inet.c:142-145)
 * or, for ICMP, in_cksum of the message (ip_icmp.c:187-189).  Until
 * cgck_rx_end, this thread's drop-in in_cksum / udp_cksum calls on those
 * headers and segments (same pointer, same length) return the precomputed
 * value without touching the GPU; any other call is computed synchronously
 * as outside the window.  The stack's verify, count and drop code
 * (t_*_do_incksum 0/1/2) therefore runs unchanged.
 *
 * desc[i] = {frame offset from base, l3_off (14 for Ethernet), bytes
 * received after l3_off (ip_input's `len`)}; [base, base + bytes) must hold
 * every frame and stay unchanged (apart from the checksum fields the stack
 * zeroes and rewrites) until cgck_rx_end.  The L4 value covers
 * ntohs(ip_len) - ip_hl*4 bytes when the frame holds them.  Registered
 * memory (cgck_host_register) is read in place.  Returns the number of
 * frames precomputed, or a negative errno (-EBUSY: a window is already
 * open).  cgck_rx_end returns how many calls the window answered. */
int cgck_rx_begin(void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n);
int cgck_rx_end(void);

/* Pipelined RX window: bursts in flight while the stack works.  The
 * transport posts burst k as it arrives (cgck_rx_post returns at once, the
 * burst server computing it meanwhile), then opens the window over the
 * oldest posted burst — k - 1, whose values are in by then — with
 * cgck_rx_begin_posted, runs the stack over it and closes it with
 * cgck_rx_end as above.  The ring keeps a posted burst's frames unchanged
 * until its window closes (netmap's head and DPDK's mbuf free come after
 * the stack's processing: netmap.c:116-126, dpdk.c:255-263).  Up to 64
 * bursts may be posted and not yet opened (-EBUSY beyond).  One request per
 * thread is on the burst server at a time: the bursts posted while it is
 * there go out together, as one request, when it is back, so a loop that
 * posts small bursts faster than one request's round trip pays one round
 * trip per round trip, not per burst.  Without an open burst server, or
 * when a burst does not fit it, cgck_rx_post computes the burst at once.
 * cgck_rx_post returns the frames posted (-EINVAL: a descriptor reaches
 * past `bytes`); cgck_rx_begin_posted the frames the window answers for
 * (as cgck_rx_begin), -ENOENT when nothing is posted.  Posted fills
 * (cgck_tx_post) coalesce the same way, and bursts and fills waiting
 * together over the same registered range go out as one request. */
int cgck_rx_post(void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n);
int cgck_rx_begin_posted(void);

/* The drain rule.  con-gen's loop calls io_rx only on POLLIN
 * (con-gen.c:508-517), so the burst posted last before a quiet spell would
 * otherwise wait for the next frame to arrive.  Every thread_process
 * iteration that posts no burst drains: while cgck_rx_pending() > 0, the
 * transport opens the oldest posted burst (cgck_rx_begin_posted, which
 * waits for its values if the GPU is not done), runs the stack over it,
 * closes it and releases its slots.  A burst therefore
 * never waits longer than one loop iteration after its post.
 * cgck_rx_pending returns the bursts posted and not yet opened (0..64);
 * cgck_rx_ready, without waiting, 1 when the oldest one's values are in
 * (opening it will not wait), 0 while the GPU still computes it, -ENOENT
 * when nothing is posted.  A transport may also drain a ready burst early,
 * in the iteration that posted it (after check_timers, con-gen.c:524). */
int cgck_rx_pending(void);
int cgck_rx_ready(void);

/* Deferred TX fill.  Between begin and flush, the
 * drop-in in_cksum/udp_cksum calls of THIS thread that target an IPv4
 * header (len == ip_hl*4), a TCP/UDP segment, or an ICMP message right
 * after a 20-byte header of protocol 1 (icmp_send, ip_icmp.c:68-80) lying
 * inside memory registered with cgck_host_register (the transport's ring or
 * mempool, whose slots stay owned by the stack until the kick) return 0 and
 * are queued; a second call for the same header or segment replaces the
 * first.  Calls on any other memory (a stack-local struct packet, pkt_body)
 * are computed synchronously, as outside the window.  The flush computes the
 * queue in one launch and writes each result into its field (ip+10; TCP +16
 * / UDP +6 / ICMP +2 after the header); it must run before the transport
 * hands the slots to the NIC.  Returns the number of fields written, or a
 * negative errno.
 *
 * The window may stay open for the whole loop iteration,
 * so the replies the stack builds while it processes a burst (tcp_respond,
 * icmp_error, echo replies) and check_timers' keepalives are queued too.
 * A call about a frame of the open RX window is never queued (it is the
 * stack verifying what it received).  A received frame must therefore be
 * processed inside an RX window whenever the TX window is open: its verify
 * calls outside one would look like a transmit call and be queued.
 * cgck_window_stats_n's counter [4] counts queued calls on a header of the
 * last closed RX window's frames, so an integration that misses that rule
 * shows up there. */
int cgck_tx_begin(void);
int cgck_tx_flush(void);

/* Pipelined TX fill: cgck_tx_post closes the window like cgck_tx_flush but
 * returns once the fill is posted (the number of fields queued); the fields
 * are final once cgck_tx_complete, which waits for the oldest posted fill,
 * returns how many it wrote (0: none posted).  The kernel returns the
 * values and the completion writes the fields from the host, so the ring
 * lines stay in the worker's caches for the stack's next writes to those
 * slots.  The transport calls
 * it before it hands those slots to the NIC — at the next loop's kick
 * (con-gen.c:493), so the GPU computes burst k while the stack builds burst
 * k + 1.  Up to 64 fills may be posted and not yet completed: one more
 * cgck_tx_post completes the oldest first (its fields are written then); if
 * that completion fails, the new window is still posted and the oldest
 * fill's error is returned (its fields stay unwritten: the transport drops
 * or recomputes those packets). */
int cgck_tx_post(void);
int cgck_tx_complete(void);

/* Without waiting: fills posted and not yet completed (cgck_tx_pending),
 * and whether the oldest one's values are in (cgck_tx_ready: 1, so
 * cgck_tx_complete will not wait; 0 while the GPU computes it; -ENOENT
 * when none is posted).  A transport that holds each fill's slots back from
 * the NIC until its completion (netmap: `head` stops at the fill's first
 * slot; DPDK: its mbufs stay out of rte_eth_tx_burst) can complete fills as
 * they come back instead of waiting at every kick. */
int cgck_tx_pending(void);
int cgck_tx_ready(void);

/* Per-thread window counters since the thread's first call:
 * [0] drop-in calls answered by an RX window, [1] calls inside an RX window
 * computed synchronously (no match), [2] calls queued by a TX window, [3]
 * calls inside a TX window computed synchronously (memory not registered). */
int cgck_window_stats(uint64_t stats[4]);
/* The same counters and more: writes min(n, 5) of them and returns how many
 * the library keeps (5).  [4]: TX-window calls queued on the IPv4 header of a
 * frame of the last closed RX window (a received frame verified outside an RX
 * window, see cgck_tx_begin; or a received frame reused for a reply). */
int cgck_window_stats_n(uint64_t *stats, int n);

/* Burst server (latency).  Keeps up to 32 workgroups
 * (one per 64 packets of max_pkts) resident on `ctx` (NULL: this thread's
 * drop-in context) that serve host-resident batches through a mailbox (a
 * doorbell in device memory the host writes through the large BAR, or
 * host-coherent memory): cgck_desc_host, the RX window, the TX window's flush (its queue
 * read in place when it lies in one registered range, as cgck_desc_host of
 * that range) and the synchronous drop-in calls then skip the kernel launch
 * and the stream synchronisation whenever a batch fits (at most max_pkts packets and max_bytes of packet bytes; a
 * batch of more than 64 packets is split over the workgroups).  Batches
 * above the caps take the launch path, whose many workgroups read host
 * memory faster for hundreds of frames of >= 576 B: max_bytes ~96 KiB routes
 * a mixed workload best.  Each server holds a hardware
 * queue of its own, so a device takes at most 12 from a process (-EBUSY
 * beyond: that context runs its requests through launches).  The server exits after idle_ms
 * without a request (0: 200 ms) and is relaunched by the next one; close
 * stops it.  cgck_ctx_destroy and cgck_thread_release close it too. */
int cgck_burst_open(cgck_ctx_t *ctx, uint32_t max_pkts, size_t max_bytes, uint32_t idle_ms);
int cgck_burst_close(cgck_ctx_t *ctx);

/* One request to ctx's open burst server (NULL: this thread's context) over
 * memory the device already sees — [dev_base, dev_base + range), e.g. the
 * device view of a ring registered elsewhere.  The host does not check the
 * descriptors: the server checks every one against `range` on the device
 * before any load or store, and a descriptor that reaches past it fails the
 * request with -EIO: the workgroup whose slice holds it reads and stores
 * nothing (the other slices of a wide request may have been served).  Every request the library posts
 * to a server for registered memory (cgck_desc_host, the RX/TX windows)
 * carries its range the same way.  -ENOSPC: no server open, or n above its
 * max_pkts.  cgck_host_register / cgck_host_unregister drain every open
 * server before the mapping changes (the next request relaunches it), so no
 * server kernel runs across a mapping change. */
int cgck_burst_request(cgck_ctx_t *ctx, const void *dev_base, uint64_t range,
		       const cgck_desc_t *desc, uint64_t n, uint32_t flags,
		       uint32_t *out, uint8_t *verdict);

/* Synthetic batches generated on the device.  Byte j of the
 * stream is byte (j & 7) of splitmix64(seed, j >> 3); each packet then gets
 * ver/ihl 0x45, tos 0, total length, ip_p = 6 and zeroed IP/TCP checksum
 * fields.  IMIX: 64/576/1500 at 7:4:1 in a fixed 12-packet cycle, packed
 * densely, with the descriptors written to `desc`. */
int cgck_synth_strided(cgck_ctx_t *ctx, void *base, uint64_t n, uint64_t stride,
		       uint32_t ip_len, uint64_t seed, void *stream);
/* The same byte stream stamped as IPv6 packets (40 <= ip_len <= stride,
 * ip_len <= 65535): bytes 0-3 = 60 00 00 00, bytes 4-5 = ip_len - 40
 * big-endian, byte 6 = nh, and the checksum field of nh (TCP +16, UDP +6,
 * ICMPv6 +2 after the 40-byte header) zeroed when the packet holds it. */
int cgck_synth_strided_ip6(cgck_ctx_t *ctx, void *base, uint64_t n, uint64_t stride,
			   uint32_t ip_len, uint32_t nh, uint64_t seed, void *stream);
int cgck_synth_imix(cgck_ctx_t *ctx, void *base, cgck_desc_t *desc, uint64_t n,
		    uint64_t seed, void *stream);
uint64_t cgck_imix_bytes(uint64_t n); /* bytes an n-packet IMIX batch occupies */
/* The same IMIX frames in ring slots: frame k at k * stride + l3_off (the
 * netmap layout: 2048-byte slots, IPv4 at +14), n * stride bytes of buffer. */
int cgck_synth_imix_ring(cgck_ctx_t *ctx, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
			 uint32_t l3_off, uint64_t seed, void *stream);
/* The two IMIX sets stamped as IPv6: the byte stream, the 12-frame cycle, the
 * offsets and the descriptors of cgck_synth_imix / cgck_synth_imix_ring, each
 * frame stamped as cgck_synth_strided_ip6 stamps one (nh <= 255). */
int cgck_synth_imix_ip6(cgck_ctx_t *ctx, void *base, cgck_desc_t *desc, uint64_t n,
			uint32_t nh, uint64_t seed, void *stream);
int cgck_synth_imix_ring_ip6(cgck_ctx_t *ctx, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
			     uint32_t l3_off, uint32_t nh, uint64_t seed, void *stream);
/* A dual-stack IMIX set (for CGCK_MIXED): the byte stream, the 12-frame cycle,
 * the offsets and the descriptors of cgck_synth_imix (stride == 0: packed,
 * l3_off must be 0, cgck_imix_bytes(n) bytes) or of cgck_synth_imix_ring
 * (stride != 0: n * stride bytes).  Frame k is stamped IPv6 when k % 5 < 2 (5 is
 * coprime to 12: every cycle position sees both families), as
 * cgck_synth_strided_ip6 stamps one, otherwise IPv4 as cgck_synth_strided does.
 * Its protocol follows k % 7: 0-3 TCP (6), 4-5 UDP (17), 6 ICMP (1 for IPv4, 58
 * for IPv6); that protocol's checksum field is zeroed when the frame holds it. */
int cgck_synth_imix_dual(cgck_ctx_t *ctx, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
			 uint32_t l3_off, uint64_t seed, void *stream);
/* Ethernet framing for the ring form (stride != 0) of a cgck_synth_imix* set, for
 * cgck_l2_desc: `desc` is the set's descriptor array, `raw` receives the
 * transport's view.  For frame k, t = (vlan_every && k % vlan_every == 0) ? 1 : 0
 * and h = 14 + 4t; the h bytes before the IP header, at frame_off + l3_off - h,
 * become: twelve address bytes from splitmix64(seed, 2k) and splitmix64(seed, 2k +
 * 1) (eight and four, low byte first) with bit 0 of byte 0 cleared; when t, TPID
 * 0x8100 and TCI k & 0x0FFF; the ethertype by the version nibble at l3_off (4:
 * 0x0800, 6: 0x86DD, anything else 0x0806).  raw[k] = {frame_off, l3_off - h,
 * max(ip_len + h, 60)}: the padding of a short frame is the ring's own stream
 * bytes after the packet (non-zero garbage).  The slots must hold l3_off + 1500
 * bytes, as for cgck_synth_imix_dual.  -EINVAL: a NULL or misaligned argument, or
 * any l3_off < 18 (no room for the header and a tag); that is checked on the
 * device before anything is written, so the call waits for `stream` once, and it
 * uses the context's dst-cache scratch (one such call at a time per context). */
int cgck_synth_eth(cgck_ctx_t *ctx, void *base, const cgck_desc_t *desc, cgck_desc_t *raw,
		   uint64_t n, uint32_t vlan_every, uint64_t seed, void *stream);

/* ------------------------------------------------------------------------ */
/* 3. Toeplitz RSS hash (subr.c:482-530, subr.h:370-371) */
/*    and the dst-cache build that calls it (con-gen.c:291-360).             */
/* ------------------------------------------------------------------------ */

/* Drop-in symbols, prototypes of subr.h:370-371.  Synchronous, on the calling
 * thread's context (like in_cksum).  toeplitz_hash: subr.c:482-502 over
 * `cnt` bytes (cnt <= 65536; reads key[0..3] and key[4..key_size-1] as the
 * reference does).  rss_hash4: subr.c:506-530, the hash of the 12 bytes
 * {faddr, laddr, fport, lport} masked to 7 bits.  Caller: con-gen.c:338. */
uint32_t toeplitz_hash(const unsigned char *data, int cnt, const unsigned char *key, int key_size);
uint32_t rss_hash4(uint32_t laddr, uint32_t faddr, uint16_t lport, uint16_t fport,
		   unsigned char *key, int key_size);

/* Batched hash, device-resident: out[k] = toeplitz_hash(data + k*stride, cnt,
 * key, key_size) & mask (mask 0x7F = rss_hash4 on {faddr, laddr, fport,
 * lport} records of 12 bytes).  `key` is host memory (the context derives
 * and caches its byte tables).  Asynchronous. */
int cgck_toeplitz(cgck_ctx_t *ctx, const void *data, uint64_t n, uint64_t stride, uint32_t cnt,
		  const unsigned char *key, int key_size, uint32_t mask, uint32_t *out, void *stream);

/* Per-frame hash of a receive burst: the software RSS steer for transports
 * without hardware RSS (veth, memif, pcap deliver every frame on one queue) and
 * the audit of an "RSS is invalid" panic (con-gen.c:358).  The kernel finds the
 * tuple in each frame itself; nothing is parsed, cut out or uploaded by the host.
 *
 * Each frame is ip_len bytes at base + frame_off + l3_off (descriptor or strided
 * argument, as for the checksum calls) and is judged by v, the high nibble of
 * its first byte b[0], as under CGCK_MIXED.  The header's own length fields
 * (IPv4 total length, IPv6 payload length) are not consulted: ip_len bounds
 * every read.
 *   ip_len == 0   kind = CGCK_BAD_LEN.
 *   v == 4        hl = (b[0] & 15) * 4.  ip_len < 20, hl < 20 or ip_len < hl:
 *                 CGCK_BAD_LEN.  The frame is a fragment when
 *                 ((b[6] << 8 | b[7]) & 0x3FFF) != 0 (MF set or a non-zero
 *                 offset; DF alone is not a fragment).  A non-fragment with
 *                 ip_len >= hl + 4 and ip_p == 6 under CGCK_RSS_TCP, or ip_p ==
 *                 17 under CGCK_RSS_UDP, hashes the 12 bytes b[12..20) ++
 *                 b[hl..hl+4): kind = CGCK_RSS_L4.  Every other frame hashes the
 *                 8 bytes b[12..20): kind = 0.  The byte order is rss_hash4's
 *                 {faddr, laddr, fport, lport} as the receiver sees them
 *                 (subr.c:506-530): hash & 0x7F of a CGCK_RSS_L4 frame is
 *                 rss_hash4(ip_dst, ip_src, dport, sport).
 *   v == 6        the extension-header walk of CGCK_IP6 without its last clause:
 *                 l4_off = 40, nh = b[6]; Hop-by-Hop (0), Routing (43) and
 *                 Destination Options (60) advance by (b[1] + 1) * 8, AH (51) by
 *                 (b[1] + 2) * 4, at most 8 extension headers.  ip_len < 40, an
 *                 extension header's first two bytes past ip_len, an l4_off past
 *                 ip_len or a ninth header: CGCK_BAD_LEN.  The checksum-field
 *                 clause does not apply: a TCP frame cut after its ports still
 *                 hashes them.  A Fragment header (44) hashes the 32 bytes
 *                 b[8..40): kind = CGCK_RSS_IP6.  A terminal nh of 6 under
 *                 CGCK_RSS_TCP, or 17 under CGCK_RSS_UDP, with ip_len >= l4_off
 *                 + 4 hashes the 36 bytes b[8..40) ++ b[l4_off..l4_off+4): kind =
 *                 CGCK_RSS_IP6 | CGCK_RSS_L4.  Everything else hashes b[8..40):
 *                 kind = CGCK_RSS_IP6.  The addresses always come from the fixed
 *                 header: there is no home-address or routing-header
 *                 substitution.
 *   any other v   kind = CGCK_NOT_IP.
 * A CGCK_BAD_LEN or CGCK_NOT_IP frame has no hash: hash = 0, queue = 0xFF, no
 * other kind bit, and it is not counted in qcount.
 * The key follows cgck_toeplitz's rule (key[0..3] always read, zeros after
 * max(4, key_size) bytes); these calls share the context's table cache, and its
 * wait on a key change, with cgck_toeplitz and cgck_dst_cache. */
enum { CGCK_RSS_TCP = 1u << 0, CGCK_RSS_UDP = 1u << 1 };      /* hf: which protocols hash their ports */
enum { CGCK_RSS_L4 = 1u << 4, CGCK_RSS_IP6 = 1u << 5 };       /* kind bits, beside CGCK_BAD_LEN / CGCK_NOT_IP */

typedef struct cgck_rss_spec {
	const unsigned char *key; /* host memory, as cgck_toeplitz */
	int key_size;
	uint32_t mask;            /* hash[k] = toeplitz & mask (0x7F = rss_hash4's) */
	uint32_t hf;              /* CGCK_RSS_TCP | CGCK_RSS_UDP; addresses are always hashed */
	uint32_t queue_num;       /* 0: no queue ids; else 1..128 (RSS_QUEUE_ID_MAX) */
} cgck_rss_spec_t;

typedef struct cgck_rss_res {   /* each optional (NULL); at least one non-NULL */
	uint32_t *hash;   /* per frame */
	uint8_t *kind;    /* per frame */
	uint8_t *queue;   /* per frame: hash[k] % queue_num, 0xFF for a frame without a hash */
	uint32_t *qcount; /* u32[queue_num] running counters: [q] += frames steered to q */
} cgck_rss_res_t;

/* Device-resident bursts (`base`, `desc` and the arrays of `res` are device
 * memory; `desc` any 4-byte aligned array), asynchronous on `stream` (NULL: the
 * context's).  One kernel, rssf_kernel, serves both forms.  n == 0 returns 0 and
 * launches nothing.  -EINVAL: a NULL ctx, spec, res, key or base (with n > 0 a
 * NULL desc too); every output NULL; unknown hf bits; queue_num > 128; queue or
 * qcount given with queue_num == 0; a strided ip_len > 65535. */
int cgck_rss_strided(cgck_ctx_t *ctx, const void *base, uint64_t n, uint64_t stride, uint32_t l3_off,
		     uint32_t ip_len, const cgck_rss_spec_t *spec, const cgck_rss_res_t *res, void *stream);
int cgck_rss_desc(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *desc, uint64_t n,
		  const cgck_rss_spec_t *spec, const cgck_rss_res_t *res, void *stream);
/* Host-resident burst, synchronous: registered memory is read in place, a
 * pageable range [base, base + bytes) is copied to the device and hashed there;
 * the arrays of `res` are host memory (qcount is incremented).  The frame bytes
 * are not written.  It never goes through the burst server.  -EINVAL as above,
 * and when a descriptor reaches past `bytes`. */
int cgck_rss_desc_host(cgck_ctx_t *ctx, const void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n,
		       const cgck_rss_spec_t *spec, const cgck_rss_res_t *res);

/* Software steer: a stable counting partition of a device-resident burst by
 * queue id, the step from cgck_rss_desc's one byte per frame to "worker q
 * verifies queue q's frames" without a host pass (INTEGRATION.md has the
 * recipe; DESIGN.md §5.10 the kernels and the measurements).
 *
 * Bins.   bin(k) = queue[k] when queue[k] < queue_num, else queue_num: that last
 *         bin is the unsteered bucket, which takes the 0xFF of a frame without a
 *         hash and any other byte not below queue_num.  The call is total over
 *         all 256 byte values: no input byte makes it fail on the device.
 * Order.  Slots are filled by ascending bin and, within a bin, by ascending
 *         arrival index k: the partition is stable (a flow's frames keep their
 *         order) and the output is fully determined.
 * qoff    qoff[q] = the first slot of bin q, q in 0..queue_num (qoff[queue_num]:
 *         the first unsteered slot); qoff[queue_num + 1] = n.  Written, not
 *         accumulated.
 * perm    perm[s] = the arrival index k of the frame in slot s.
 * slot    slot[k] = s, the inverse of perm (carries per-slot results back to
 *         arrival order).
 * desc_out  desc_out[s] = desc_in[perm[s]]: queue q's descriptors are
 *         desc_out[qoff[q] .. qoff[q + 1]).
 * Arguments.  queue_num is 1..128, as in cgck_rss_spec_t; n <= 0xFFFFFFFF.
 *         desc_in may be NULL when desc_out is NULL (a strided caller uses perm).
 *         desc_in and desc_out are 4-byte aligned, as for CGCK_MIXED, and must
 *         not be the same array.
 * Workspace.  `work` is caller-owned device memory of at least
 *         cgck_steer_work_bytes(n, queue_num) bytes, 4-byte aligned.  It need not
 *         be zeroed and holds nothing between calls.  The library keeps no hidden
 *         scratch for this call: two calls in flight on two streams of one context
 *         are independent (unlike the table cache).  cgck_steer_work_bytes is pure
 *         (no device, no context) and returns 0 for every n that fits one tile (n
 *         <= 4096 frames: any receive burst), and `work` may then be NULL.
 * Execution.  Asynchronous on `stream` (NULL: the context's).  n == 0 returns 0,
 *         launches nothing and writes nothing (cgck_rss_desc's rule).  The inputs
 *         (queue, desc_in, the frames) are never written.  One tile takes one
 *         launch (steer_one_kernel); more take three (count, scan, scatter), and
 *         no workgroup ever waits for another.
 * Measured (DESIGN.md §5.10, 16M dual-stack IMIX frames on one MI355X): all four
 *         outputs take 0.27 ms with 8 queues and 0.55 ms with 128, against 0.48 ms
 *         for the cgck_rss_desc that feeds them and 210 / 920 ms for the host
 *         route (queue[] down, a stable numpy bucket, the descriptors up); perm
 *         alone takes 0.09 / 0.27 ms.  On a burst the one launch takes 6 us at 256
 *         frames and 17 us at 4096, the three launches 11 and 22 us: keep device
 *         bursts within one tile.
 * There is no host form: a host burst's queue[] already lies on the host after
 * cgck_rss_desc_host, and a bucket loop over a few hundred bytes there costs less
 * than one launch.
 * -EINVAL: a NULL ctx, queue or res; every output NULL; queue_num 0 or above
 * 128; n above 0xFFFFFFFF; desc_out without desc_in; desc_out == desc_in; a
 * misaligned descriptor array or workspace; work NULL while
 * cgck_steer_work_bytes(n, queue_num) != 0. */
typedef struct cgck_steer_res { /* device memory; each optional (NULL); at least one non-NULL */
	uint32_t *qoff;        /* u32[queue_num + 2], written (not accumulated) */
	uint32_t *perm;        /* u32[n]: perm[s] = arrival index k of the frame in slot s */
	uint32_t *slot;        /* u32[n]: slot[k] = s, the inverse of perm */
	cgck_desc_t *desc_out; /* cgck_desc_t[n]: desc_out[s] = desc_in[perm[s]] */
} cgck_steer_res_t;

size_t cgck_steer_work_bytes(uint64_t n, uint32_t queue_num);
int cgck_steer(cgck_ctx_t *ctx, const uint8_t *queue, uint64_t n, uint32_t queue_num,
	       const cgck_desc_t *desc_in, const cgck_steer_res_t *res, void *work, void *stream);
/* Hash and steer: cgck_rss_desc with `spec` and `rss`, then cgck_steer over
 * rss->queue with queue_num = spec->queue_num and desc_in = desc, on one stream.
 * rss->queue is required (it is the steer's input; the library allocates none)
 * and so is spec->queue_num >= 1; rss's other arrays stay optional, and qcount
 * keeps its running-counter meaning.  -EINVAL: cgck_rss_desc's list, cgck_steer's
 * list, a NULL rss->queue, queue_num 0. */
int cgck_rss_steer_desc(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *desc, uint64_t n,
			const cgck_rss_spec_t *spec, const cgck_rss_res_t *rss, const cgck_steer_res_t *res,
			void *work, void *stream);

/* Classify and trim a raw Ethernet burst: the stage before every call above.
 * Those calls start from a cgck_desc_t that already names l3_off and ip_len; a
 * transport knows only where a frame starts and how many bytes the NIC
 * delivered.  cgck_l2_desc is ether_input's demultiplex (bsd44/if_ether.c:152-183)
 * and ip_input's length rules (ip_input.c:28-44, 63-79) as one kernel over a
 * device-resident burst: it finds the IP header behind up to two VLAN tags, names
 * the frame's class, and cuts Ethernet padding off by the header's own length
 * field.  (A 40-byte TCP ACK arrives in a 60-byte frame; with ip_len = 60 - 14 the
 * pseudo-header length is wrong and a good segment verifies as CGCK_BAD_L4.)
 *
 * Input.  raw[k] is a cgck_desc_t read as: frame_off as usual; l3_off the offset
 * of the Ethernet header inside the slot (0 for most rings); ip_len the bytes
 * delivered from that offset, L below.  `raw` is any 4-byte aligned array.
 *
 * Contract.  With e the L bytes at base + frame_off + l3_off, for every frame:
 *  1. L < 14: class RUNT.
 *  2. et = e[12] << 8 | e[13], off = 14, tags = 0.  While et is 0x8100 or 0x88A8
 *     and tags < 2: if L < off + 4 the class is RUNT (and the walk ends);
 *     otherwise et = e[off+2] << 8 | e[off+3], off += 4, ++tags.  tags > 0 when the
 *     walk ends sets CGCK_L2_VLAN, whatever the class.  An et that is still one of
 *     the two TPIDs after two tags: class OTHER.
 *  3. Flags, on every frame with L >= 14, whatever its class (if_ether.c:163-168):
 *     CGCK_L2_BCAST when e[0..5] are all 0xFF, otherwise CGCK_L2_MCAST when
 *     e[0] & 1.
 *  4. avail = L - off; b = the bytes from off on.
 *  5. et == 0x0800, in ip_input's order: avail < 20: TOOSMALL.  b[0] >> 4 != 4:
 *     BADVERS.  hl = (b[0] & 15) * 4; hl < 20 or hl > avail: BADHLEN.  total =
 *     b[2] << 8 | b[3]; total < hl: BADLEN.  avail < total: TOOSHORT.  Otherwise
 *     IP4 with ip_len_out = total.
 *  6. et == 0x86DD: avail < 40: TOOSMALL.  b[0] >> 4 != 6: BADVERS.  total = 40 +
 *     (b[4] << 8 | b[5]); avail < total: TOOSHORT.  Otherwise IP6 with ip_len_out
 *     = total.  There is no jumbogram rule: a jumbogram carries payload length 0
 *     and comes out as IP6 with ip_len_out = 40 (its fixed header, and a
 *     Hop-by-Hop header cut off: CGCK_BAD_LEN to every later call); L is 16 bits,
 *     so a total above 65535 is always TOOSHORT.
 *  7. et == 0x0806: ARP.  Any other et, an 802.3 length field included: OTHER.
 *  8. raw.l3_off + off > 65535 (the output field has 16 bits), for a frame that
 *     rules 1-2 did not already make a RUNT: class RUNT, flags as above.
 * The result is fully determined for every byte string.
 *
 * Outputs.  desc_out[k].frame_off = raw[k].frame_off, always.  IP4 / IP6: l3_off =
 * raw.l3_off + off, ip_len = ip_len_out.  ARP / OTHER and the drop classes 5-9:
 * l3_off = raw.l3_off + off, ip_len = 0.  RUNT: l3_off = raw.l3_off, ip_len = 0.
 * ip_len == 0 is the existing "no frame" value (CGCK_MIXED and cgck_rss_desc
 * answer CGCK_BAD_LEN, queue 0xFF; cgck_steer bins it as unsteered), so the three
 * calls compose after this one with no special case.  cls[k] = class | flags.
 * count[] are running counters (+=, like `bad` and qcount): [c] frames of class c
 * for the ten classes, [10] frames with CGCK_L2_BCAST or CGCK_L2_MCAST
 * (if_imcasts), [11] frames with CGCK_L2_VLAN.  count[5..9] are what
 * ipstat.ips_toosmall / ips_badvers / ips_badhlen / ips_badlen / ips_tooshort
 * would have counted, with one difference: ip_input verifies the header sum
 * before it looks at ip_len (ip_input.c:45-67), so a frame with both a bad sum and
 * a bad length is counted there as ips_badsum and here by its length class only
 * (this call sums nothing; CGCK_VERIFY does, afterwards).
 *
 * Execution.  Asynchronous on `stream` (NULL: the context's).  n == 0 returns 0,
 * launches nothing and writes nothing.  The frames and `raw` are never written.
 * The library keeps no scratch for this call.  One kernel, l2d_kernel; every rule
 * consults only the frame's first 28 bytes, and every read lies inside the 16-byte
 * granules that hold a byte of [frame, frame + L) (cgck_rss_desc's rule).
 * desc_out must not be raw.
 * Measured (DESIGN.md §5.11, 16M Ethernet-framed dual-stack IMIX frames in
 * 2048-byte slots on one MI355X): 0.50 ms with all three outputs, the same as the
 * cgck_rss_desc that follows it on the same burst.
 * There is no host form and no strided form: a host burst's bytes are in the
 * host's caches for the RX window anyway, where these few compares per frame cost
 * less than a launch; and a ring's delivered lengths differ per slot, so its caller
 * writes an array either way.
 * -EINVAL: a NULL ctx, res or base, or (with n > 0) a NULL raw; every output
 * NULL; a misaligned raw or desc_out; desc_out == raw. */
enum { /* class: low nibble of cls[k] */
	CGCK_L2_IP4 = 0, CGCK_L2_IP6 = 1, CGCK_L2_ARP = 2, CGCK_L2_OTHER = 3, CGCK_L2_RUNT = 4,
	CGCK_L2_TOOSMALL = 5, CGCK_L2_BADVERS = 6, CGCK_L2_BADHLEN = 7, CGCK_L2_BADLEN = 8,
	CGCK_L2_TOOSHORT = 9, CGCK_L2_NCLASS = 10,
};
enum { CGCK_L2_VLAN = 1u << 4, CGCK_L2_BCAST = 1u << 6, CGCK_L2_MCAST = 1u << 7 }; /* flag bits of cls[k] */
#define CGCK_L2_NCOUNT 12 /* counters: [class] for the ten classes, [10] BCAST or MCAST frames (if_imcasts), [11] tagged frames */

typedef struct cgck_l2_res {   /* device memory; each optional (NULL); at least one non-NULL */
	cgck_desc_t *desc_out; /* [n] */
	uint8_t *cls;          /* [n] */
	uint32_t *count;       /* u32[CGCK_L2_NCOUNT], running counters (+=), like `bad` and qcount */
} cgck_l2_res_t;

int cgck_l2_desc(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *raw, uint64_t n,
		 const cgck_l2_res_t *res, void *stream);

/* Per-frame TCP / UDP segment records: the stage after the verify.  What either
 * stack does next with a verified frame is the front half of tcp_input / tcp_in /
 * udp_input: the segment length rules (tcps_rcvshort, tcps_rcvbadoff, udps_hdrops,
 * udps_badlen: bsd44/tcp_input.c:67,91-95, gbtcp/inet.c:123-131,154-156,
 * bsd44/udp_usrreq.c:65-79), the header fields in host order (tcp_input.c:107-110;
 * gbtcp's struct tcb, gbtcp/inet.h:128-134), the option walk (tcp_dooptions,
 * tcp_input.c:925-996) and the PCB hash SO_HASH(faddr, lport, fport) that
 * in_pcblookup starts from (subr.h:179-180, in_pcb.c:175).  cgck_l4_desc produces
 * them on the device, one kernel over the burst's descriptors, so a worker reads
 * verdict[s], cls[s] and seg[s], goes to its hash bucket, and touches a frame only
 * when the segment carries payload.  This is header demultiplexing: the parsing
 * ends where tcp_input.c:115 (findpcb) begins, and there is no TCP state machine
 * here.
 *
 * Contract, total over every byte string.  A frame is the ip_len bytes b at base +
 * frame_off + l3_off; ip_len bounds every read; the IP header's own length fields
 * are not consulted (cgck_l2_desc has applied them).
 *  1. The IP layer, by cgck_rss_desc's rules word for word, so that both calls
 *     judge a frame alike.  ip_len == 0: NONE.  v = b[0] >> 4; CGCK_SEG_IP6 is set
 *     whenever ip_len > 0 and v == 6, whatever the class.
 *     v == 4: hl = (b[0] & 15) * 4; ip_len < 20, hl < 20 or ip_len < hl: NONE.
 *       ((b[6] << 8 | b[7]) & 0x3FFF) != 0: FRAG with l4_off = hl.  That is
 *       cgck_rss_desc's definition of a fragment, so the library has one notion of
 *       it; ip_input.c:94 also drops a datagram with the reserved bit set, which is
 *       not a fragment here.  Otherwise proto = b[9], l4_off = hl, F = b[12..16)
 *       loaded little-endian.
 *     v == 6: cgck_rss_desc's extension-header walk (no checksum-field clause).  Its
 *       CGCK_BAD_LEN cases: NONE.  A Fragment header: FRAG with l4_off at that
 *       header.  Otherwise proto = the terminal next-header value, l4_off where the
 *       walk stopped, F = the XOR of the four little-endian dwords of b[8..24).
 *     Any other v: NONE.
 *  2. m = ip_len - l4_off; t = the bytes from l4_off on.  Every class but NONE
 *     carries l4_off and pay_len; pay_len = m unless stated otherwise.
 *  3. proto 6.  m < 20: TCP_SHORT.  off = (t[12] >> 4) * 4; off < 20: TCP_BADOFF;
 *     off > m: TCP_OFFLONG (bsd44 counts both as tcps_rcvbadoff, gbtcp counts
 *     OFFLONG as tcps_rcvshort: hence two classes).  Otherwise TCP: sport = t[0] |
 *     t[1] << 8 and dport likewise, as stored; seq, ack and win read big-endian;
 *     th_flags = t[13]; hdr_len = off; pay_len = m - off; and the options, with cnt
 *     = off - 20, o = t[20..off), i = 0, while i < cnt: o[i] == 0 stops; o[i] == 1:
 *     ++i; otherwise i + 1 >= cnt stops with OPT_BAD, len = o[i+1], len == 0 stops
 *     with OPT_BAD, i + len > cnt stops with OPT_BAD; kind 2 with len 4 on a SYN:
 *     mss (big-endian) and CGCK_SEG_MSS; kind 3 with len 3 on a SYN: wscale =
 *     min(o[i+2], 14) and CGCK_SEG_WS; kind 8 with len 10: ts_val, ts_ecr and
 *     CGCK_SEG_TS; a later occurrence overwrites an earlier one; i += len (a len of
 *     1 advances one byte, as the reference does).  On every well-formed segment
 *     this is tcp_dooptions.  It differs where the reference reads cp[1] or option
 *     data past the option area, for which it has no bound (tcp_input.c:937-948):
 *     here no byte at or past `off` is ever consulted.
 *  4. proto 17.  m < 8: UDP_SHORT.  ulen = t[4] << 8 | t[5]; ulen > m or ulen < 8:
 *     UDP_BADLEN.  The first condition is udps_badlen; the second has no
 *     counterpart: the reference goes on with a datagram shorter than its header.
 *     Otherwise UDP: the ports, hdr_len = 8, pay_len = ulen - 8.
 *  5. proto 1 under v4, or 58 under v6: ICMP.  Anything else: OTHER.  Both carry
 *     only l4_off and pay_len.
 *  6. hash[k] = F ^ (F >> 16) ^ bswap16(dport ^ sport) for TCP and UDP: SO_HASH(ip_src,
 *     dport, sport) as the receiver's in_pcblookup computes it; for IPv4 it equals
 *     the `hash` of the cgck_dst_entry_t the frame answers.  0 for every other class.
 *  7. count[class] += 1 per frame; count[11] += 1 per frame with CGCK_SEG_IP6.
 *
 * Execution.  Asynchronous on `stream` (NULL: the context's).  n == 0 returns 0,
 * launches nothing and writes nothing.  The frames and `desc` are never written.
 * The library keeps no scratch for this call.  One kernel, l4d_kernel; `desc` is
 * any 4-byte aligned array, and every read lies inside the 16-byte granules that
 * hold a byte of [frame, frame + ip_len) (cgck_rss_desc's rule).
 * Measured (DESIGN.md §5.12, 16M dual-stack IMIX frames in 2048-byte slots on one
 * MI355X, random TCP header bytes: a worst case for the option walk): 0.62 ms
 * with all four outputs, 0.61 ms with seg alone and 0.53 ms with cls and count,
 * against 0.50 ms for cgck_rss_desc (hash only) on the same descriptors in the
 * same run: 1.23, 1.21 and 1.05 times the hash, with margins of 5 to 14 % between
 * allocations; the excess is the 37 bytes written per frame.
 * There is no host form and no strided form: a host burst's header lines are in
 * the host's caches for the RX window anyway, where this parse costs less than a
 * launch; and the call follows cgck_l2_desc or cgck_steer, which both leave a
 * descriptor array.
 * -EINVAL: a NULL ctx, res or base, or (with n > 0) a NULL desc; every output
 * NULL; a misaligned desc; a seg that is not 16-byte aligned. */
typedef struct cgck_seg {      /* 32 bytes; fields a class does not name are 0 */
	uint32_t seq, ack;         /* host order (tcp_input.c:107-108) */
	uint32_t ts_val, ts_ecr;   /* host order; valid with CGCK_SEG_TS */
	uint16_t sport, dport;     /* as stored: the u16 a little-endian load of the two bytes gives
	                              (be16_t, as in_pcb.c:178-182 compares them) */
	uint16_t win;              /* host order, unscaled */
	uint16_t mss;              /* host order; valid with CGCK_SEG_MSS */
	uint16_t l4_off;           /* from the IP header's first byte */
	uint16_t pay_len;
	uint8_t th_flags;
	uint8_t hdr_len;           /* TCP: th_off * 4 (20..60); UDP: 8; else 0 */
	uint8_t wscale;            /* min(value, 14) (TCP_MAX_WINSHIFT); valid with CGCK_SEG_WS */
	uint8_t opt;               /* CGCK_SEG_MSS | _WS | _TS | _OPT_BAD */
} cgck_seg_t;
enum { CGCK_SEG_TCP = 0, CGCK_SEG_UDP = 1, CGCK_SEG_ICMP = 2, CGCK_SEG_OTHER = 3, CGCK_SEG_FRAG = 4,
       CGCK_SEG_NONE = 5, CGCK_SEG_TCP_SHORT = 6, CGCK_SEG_TCP_BADOFF = 7, CGCK_SEG_TCP_OFFLONG = 8,
       CGCK_SEG_UDP_SHORT = 9, CGCK_SEG_UDP_BADLEN = 10, CGCK_SEG_NCLASS = 11 };   /* low nibble of cls[k] */
enum { CGCK_SEG_IP6 = 1u << 4 };                                                  /* flag bit of cls[k] */
enum { CGCK_SEG_MSS = 1, CGCK_SEG_WS = 2, CGCK_SEG_TS = 4, CGCK_SEG_OPT_BAD = 0x80 };
#define CGCK_SEG_NCOUNT 12     /* [class] for the eleven classes, [11] frames with CGCK_SEG_IP6 */

typedef struct cgck_l4_res {   /* device memory; each optional (NULL); at least one non-NULL */
	cgck_seg_t *seg;           /* [n], 16-byte aligned */
	uint8_t *cls;              /* [n] */
	uint32_t *hash;            /* [n] */
	uint32_t *count;           /* u32[CGCK_SEG_NCOUNT], running counters (+=) */
} cgck_l4_res_t;

int cgck_l4_desc(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *desc, uint64_t n,
		 const cgck_l4_res_t *res, void *stream);

/* Frames from segment records: the inverse of cgck_l2_desc + cgck_l4_desc, and the
 * transmit side's first step.  con-gen's product is header-only segments (SYNs,
 * ACKs, FINs, RSTs, keepalives: tcp_output.c:253-304,359-418, tcp_subr.c:52-123,
 * ip_output.c:42-68, gbtcp/tcp.c:381-450) whose every byte follows from a tuple and
 * a handful of numbers.  cgck_l4_build writes Ethernet + IPv4 / IPv6 + TCP / UDP
 * headers into ring slots from flow records (the tuple and the link header) and
 * segment records (cgck_seg_t: the numbers), one kernel over the burst, with both
 * checksums final for a segment without payload.  The tuples may come from
 * cgck_dst_cache, or be cgck_l4_desc's records edited into replies (tcp_respond's
 * swap of addresses and ports is the caller's edit: there is no TCP state here).
 *
 * Contract, total over every input byte string.  For frame k, F is the bytes at
 * base + slot[k].frame_off + slot[k].l3_off, cap = slot[k].ip_len the bytes the
 * slot has from there, s = seg[k].  The class, by these rules in order:
 *  1. c = cls ? cls[k] & 15 : CGCK_SEG_TCP.  c neither CGCK_SEG_TCP nor
 *     CGCK_SEG_UDP: SKIP (a caller may pass cgck_l4_desc's own class array and
 *     build only what it parsed).
 *  2. f = fidx ? fidx[k] : k.  f >= nflow, or flow[f].flags with a bit outside
 *     CGCK_FLOW_IP6 | CGCK_FLOW_VLAN: BADFLOW.  Otherwise CGCK_BLD_IP6 is set
 *     whenever the flow is IPv6, whatever class follows.
 *  3. BADSEG.  TCP: s.opt & ~(CGCK_SEG_MSS | CGCK_SEG_WS | CGCK_SEG_TS) (which
 *     includes CGCK_SEG_OPT_BAD), or CGCK_SEG_WS with s.wscale > 14.  UDP:
 *     s.pay_len > 65527.
 *  4. h = 14, or 18 with CGCK_FLOW_VLAN; iph = 20, or 40 for IPv6; l4h = 8 for
 *     UDP, for TCP 20 + 4 [MSS] + 4 [WS] + 12 [TS]; total = iph + l4h + s.pay_len;
 *     L = h + total.  L > cap, or slot[k].l3_off + h > 65535: NOROOM.
 *  5. Otherwise the frame is built, class TCP or UDP, with CGCK_BLD_PAYLOAD when
 *     s.pay_len > 0.
 * Of s the call consults sport, dport, seq, ack, win, th_flags, opt, mss, wscale,
 * ts_val, ts_ecr and pay_len; l4_off and hdr_len are ignored, so a record of
 * cgck_l4_desc can come back edited.
 * Bytes of a built frame:
 *   Ethernet.  F[0..6) = eth_dst, F[6..12) = eth_src; with VLAN 81 00 and the TCI
 *     big-endian; the ethertype 08 00 or 86 DD at F[h-2..h).
 *   IPv4.  45 00, total big-endian, the id (ip_id0 + k) & 0xFFFF big-endian
 *     (ip_output.c:40,53), ip_off big-endian, ttl, proto (6 / 17), the header sum,
 *     laddr[0..4), faddr[0..4).
 *   IPv6.  60 00 00 00, the payload length l4h + pay_len big-endian, next header =
 *     proto, hop limit = ttl, laddr, faddr (16 bytes each).  No extension headers.
 *   TCP.  sport and dport as stored (the two bytes a little-endian store of the
 *     u16 gives: the inverse of cgck_seg_t's rule), seq and ack big-endian, the
 *     data offset (l4h / 4) << 4 with a zero low nibble, th_flags, win big-endian,
 *     the sum, urgent pointer 0; then, each whenever its bit is set, in
 *     tcp_output.c:255-302's layout and order, 02 04 mss, 01 03 03 wscale, and
 *     01 01 08 0A ts_val ts_ecr.  The builder writes what it is told: MSS on a
 *     segment without SYN is the caller's business.
 *   UDP.  The ports, ulen = 8 + pay_len big-endian, the sum.
 *   Sums follow this header's `out` rule.  The IPv4 header sum is always final.
 *     With pay_len == 0 the L4 sum is final, over the 12-byte pseudo-header for
 *     IPv4 and the 40-byte one for IPv6, as under CGCK_L4 / CGCK_IP6.  With
 *     pay_len > 0 the L4 field is written as zero and CGCK_BLD_PAYLOAD says so;
 *     desc_out is then the descriptor array for cgck_desc(CGCK_L4 |
 *     CGCK_ZERO_FIELDS | CGCK_STORE [| CGCK_IP6]).  The builder never reads or
 *     sums payload: a streamed fill does that at its own rate.
 * What is written: exactly the bytes F[0, h + iph + l4h) of a built frame.
 * Payload already in the slot behind them and every byte before F stay untouched;
 * nothing of a slot whose frame is not built is written.  The kernel never reads
 * a slot's bytes and does no read-modify-write at a wider granularity, so frames
 * packed back to back may share dwords and 16-byte granules.  The slots of one
 * call must not overlap; the order between frames is unspecified, as for
 * CGCK_STORE.
 * Outputs.  raw_out[k] = {frame_off, slot.l3_off, L}: what a transport sends and
 * what cgck_l2_desc takes.  desc_out[k] = {frame_off, slot.l3_off + h, total}: what
 * cgck_desc and cgck_l4_desc take.  A frame that is not built gets {frame_off,
 * slot.l3_off, 0} in both (ip_len == 0 is the library's "no frame").  cls[k] =
 * class | flags.  count[class] += 1 per frame, count[6] += 1 per built IPv6 frame,
 * count[7] += 1 per built frame with CGCK_BLD_PAYLOAD.
 *
 * Execution.  Asynchronous on `stream` (NULL: the context's).  n == 0 returns 0,
 * launches nothing and writes nothing.  The inputs are never written.  The library
 * keeps no scratch for this call.  One kernel, l4b_kernel; DESIGN.md §5.14 has its
 * measurements.
 * -EINVAL: a NULL ctx, base or in; with n > 0 a NULL slot, seg or flow; a slot,
 * raw_out or desc_out that is not 4-byte aligned, a seg or flow that is not
 * 16-byte aligned; raw_out or desc_out equal to slot or to each other.  Every
 * 16-bit value is a legal ip_off, so none is refused.
 * Out of scope: payload sums in the builder; ICMP, IP options and
 * IPv6 extension headers; a host form (a host burst's headers are cheaper to
 * write on the host, as for cgck_l2_desc and cgck_l4_desc); any TCP state. */
typedef struct cgck_flow {       /* 48 bytes; arrays 16-byte aligned */
	uint8_t  eth_dst[6], eth_src[6];
	uint16_t vlan_tci;           /* host order; written with CGCK_FLOW_VLAN */
	uint8_t  flags;              /* CGCK_FLOW_IP6 | CGCK_FLOW_VLAN */
	uint8_t  ttl;                /* ip_ttl / hop limit */
	uint8_t  laddr[16];          /* source address as on the wire; IPv4: bytes 0..3, the rest ignored */
	uint8_t  faddr[16];          /* destination address, likewise */
} cgck_flow_t;
enum { CGCK_FLOW_IP6 = 1, CGCK_FLOW_VLAN = 2 };

typedef struct cgck_l4_build_in {   /* pointers are device memory */
	const cgck_desc_t *slot;  /* [n] where frame k goes: frame_off; l3_off = the Ethernet header's offset
	                             in the slot; ip_len = cap, the bytes the slot has from there */
	const cgck_seg_t  *seg;   /* [n], 16-byte aligned */
	const uint8_t     *cls;   /* [n] or NULL (every frame TCP): low nibble CGCK_SEG_TCP / CGCK_SEG_UDP */
	const cgck_flow_t *flow;  /* [nflow], 16-byte aligned */
	const uint32_t    *fidx;  /* [n] or NULL (frame k uses flow[k]) */
	uint32_t nflow;
	uint16_t ip_id0;          /* IPv4 frame k carries id (ip_id0 + k) & 0xFFFF (ip_output.c:40,53) */
	uint16_t ip_off;          /* host order: 0x4000 as bsd44's ip_output, 0 as gbtcp's tcp_fill */
} cgck_l4_build_in_t;

typedef struct cgck_l4_build_res {  /* device memory; each optional; res itself may be NULL */
	cgck_desc_t *raw_out;   /* [n] {frame_off, slot.l3_off, L}: what a transport sends, what cgck_l2_desc takes */
	cgck_desc_t *desc_out;  /* [n] {frame_off, slot.l3_off + h, total}: what cgck_desc / cgck_l4_desc take */
	uint8_t     *cls;       /* [n] class | flags */
	uint32_t    *count;     /* u32[CGCK_BLD_NCOUNT] running counters (+=) */
} cgck_l4_build_res_t;

enum { CGCK_BLD_TCP = 0, CGCK_BLD_UDP = 1, CGCK_BLD_SKIP = 2, CGCK_BLD_BADFLOW = 3,
       CGCK_BLD_BADSEG = 4, CGCK_BLD_NOROOM = 5, CGCK_BLD_NCLASS = 6 };   /* low nibble */
enum { CGCK_BLD_IP6 = 1u << 4, CGCK_BLD_PAYLOAD = 1u << 5 };              /* flag bits  */
#define CGCK_BLD_NCOUNT 8  /* [class] for the six classes, [6] built IPv6 frames, [7] built frames with PAYLOAD */

int cgck_l4_build(cgck_ctx_t *ctx, void *base, uint64_t n, const cgck_l4_build_in_t *in,
		  const cgck_l4_build_res_t *res, void *stream);
/* Bytes in front of the payload (h + IP header + transport header) for a flow's flags, a class byte and
 * a seg's opt; 0 when rule 1 or 3 above would refuse it (or rule 2 the flags).  Pure: no device, no
 * context. */
uint32_t cgck_l4_build_hdr_bytes(uint8_t flow_flags, uint8_t cls, uint8_t opt);

/* Per-frame connection lookup: the first thing both stacks do with a parsed
 * segment, in_pcblookup (bsd44/in_pcb.c:167-192, called from tcp_input.c:118 and
 * udp_usrreq.c:97; ip_socket_get, subr.c:580-596), over a tuple table the caller
 * owns.  cgck_l4_desc's records go in, and the index cgck_l4_build takes as fidx
 * comes out, with no host pass between the receive side and the transmit side.
 * The tuple set of a con-gen worker is fixed for the worker's life (the dst cache,
 * con-gen.c:291-360), so cgck_pcb_build makes a device hash table once per
 * dst-cache build and cgck_pcb_lookup resolves every burst against it.  This is a
 * lookup and holds no TCP state: which socket is open at an index, and what to
 * answer, stay the caller's.
 *
 * Keys.  The key of connection j is (family, proto, laddr, faddr, lport, fport)
 * with f = flow[conn[j].flow]: the family is f.flags & CGCK_FLOW_IP6; IPv4 uses
 * bytes 0..3 of f.laddr and f.faddr and ignores the rest, IPv6 all 16; f's MACs,
 * TCI, TTL and CGCK_FLOW_VLAN bit are not part of the key.  Connection j is valid
 * when proto != 0, flow < nflow and f.flags has no bit outside IP6 | VLAN.
 * The key of frame k uses b, the ip_len bytes at base + frame_off + l3_off, and
 * v = b[0] >> 4, as in_pcblookup(proto, ip_dst, dport, ip_src, sport): family
 * v == 6; proto 6 or 17 from cls[k] & 15; laddr = ip_dst (v4 b[16..20), v6
 * b[24..40)); faddr = ip_src (v4 b[12..16), v6 b[8..24)); lport = seg[k].dport,
 * fport = seg[k].sport.
 *
 * Lookup rules, in order, total over every input byte string:
 *  1. c = cls ? cls[k] & 15 : CGCK_SEG_TCP.  c neither CGCK_SEG_TCP nor
 *     CGCK_SEG_UDP: SKIP (cgck_l4_desc's own class array may come in, as in
 *     cgck_l4_build).
 *  2. NONE when ip_len == 0, when v == 4 with ip_len < 20, when v == 6 with
 *     ip_len < 40, and for any other v.  The header's own length fields and cls's
 *     IP6 flag are not consulted; ip_len bounds every read.
 *  3. The lowest valid j whose key equals the frame's: HIT, idx = j, fidx =
 *     conn[j].flow.
 *  4. BOUND with idx = bound[p] when bound != NULL, p = bswap16(seg[k].dport) <
 *     CGCK_PCB_NBOUND and bound[p] != 0xFFFFFFFF.  Proto and family are not
 *     compared, as in_pcb.c:186-188 (the reference has no IPv6; the same rule
 *     applies to it here).
 *  5. MISS.
 * Every kind but HIT and BOUND writes idx = 0xFFFFFFFF; every kind but HIT writes
 * fidx = 0xFFFFFFFF (for cgck_l4_build: BADFLOW, nothing built).  count[kind] += 1
 * per frame and count[5] += 1 per HIT with v == 6.
 *
 * Build.  cgck_pcb_build initialises the table itself (the caller need not zero
 * it) and inserts every valid connection.  stat, when given, is written, not
 * accumulated: [0] distinct keys, [1] valid entries whose key equals a lower-index
 * valid entry's, [2] entries with proto == 0, [3] entries with proto != 0 and a
 * bad flow (flow >= nflow or a refused flag bit).  The four sum to nconn and each
 * is determined whatever the order of execution.  The table's layout is private.
 * It is valid while conn, flow and table stay unchanged.  nconn == 0 is legal:
 * every frame is then MISS, BOUND, SKIP or NONE.
 * cgck_pcb_table_bytes(nconn) = 8 * S, S the power of two at or above 2 * nconn
 * and at least 2; 0 for nconn > 1 << 30.  Pure: no device, no context.
 *
 * Execution.  Both calls are asynchronous on `stream` (NULL: the context's).
 * A lookup with n == 0 launches nothing and writes nothing.  The inputs are never
 * written.  The library keeps no scratch.  Kernels: pcbb_kernel (a lane per
 * connection; no lane or workgroup ever waits for another) and pcbl_kernel (a lane
 * per frame); DESIGN.md §5.15 has the design and the measurements.
 * -EINVAL: a NULL ctx, pcb, res or base; with n > 0 a NULL desc or seg; every
 * output NULL; a desc, conn, bound, idx, fidx, count or stat that is not 4-byte
 * aligned, a seg, flow or table that is not 16-byte aligned; nconn > 1 << 30;
 * nconn > 0 with a NULL conn; nflow > 0 with a NULL flow; a NULL table;
 * table_bytes below cgck_pcb_table_bytes(nconn).  The argument checks come before
 * any device work.
 *
 * Safety, part of the contract.  A table that cgck_pcb_build did not produce for
 * these arrays can cost hits but can never fault: every index read from the table
 * is compared with nconn, and every conn[j].flow with nflow, before it is used,
 * and a probe ends after at most the table's slot count.  A reported HIT is always
 * a true key match, because the compare reads conn and flow.
 * Out of scope: the socket layer and which socket is open at an
 * index; incremental insert and delete; in_pcbnotify's quoted-header lookup; a
 * host form. */
typedef struct cgck_conn {      /* 12 bytes, arrays 4-byte aligned */
	uint32_t flow;              /* index into flow[]: the addresses and the family */
	uint16_t lport, fport;      /* as stored (be16_t), cgck_seg_t's rule */
	uint8_t  proto;             /* 6, 17, ...; 0: unused entry */
	uint8_t  rsv[3];            /* ignored */
} cgck_conn_t;

#define CGCK_PCB_NBOUND 5000    /* EPHEMERAL_MIN (subr.h:62): the ports a listening socket binds */

typedef struct cgck_pcb {       /* pointers are device memory */
	const cgck_conn_t *conn;    /* [nconn] */
	uint32_t nconn;             /* <= 1 << 30 */
	const cgck_flow_t *flow;    /* [nflow], 16-byte aligned: cgck_l4_build's table */
	uint32_t nflow;
	void *table;                /* caller-owned, 16-byte aligned */
	size_t table_bytes;         /* >= cgck_pcb_table_bytes(nconn) */
	const uint32_t *bound;      /* NULL, or u32[CGCK_PCB_NBOUND]: the index of the socket bound to port p, or 0xFFFFFFFF */
} cgck_pcb_t;

size_t cgck_pcb_table_bytes(uint32_t nconn);
int cgck_pcb_build(cgck_ctx_t *ctx, const cgck_pcb_t *pcb, uint32_t *stat /* device u32[4] or NULL */, void *stream);

typedef struct cgck_pcb_res {   /* device memory; each optional; at least one non-NULL */
	uint32_t *idx;              /* [n] connection index, 0xFFFFFFFF when there is none */
	uint32_t *fidx;             /* [n] conn[idx].flow for a HIT, else 0xFFFFFFFF */
	uint8_t  *kind;             /* [n] */
	uint32_t *count;            /* u32[CGCK_PCB_NCOUNT] running counters (+=) */
} cgck_pcb_res_t;
enum { CGCK_PCB_HIT = 0, CGCK_PCB_BOUND = 1, CGCK_PCB_MISS = 2, CGCK_PCB_SKIP = 3, CGCK_PCB_NONE = 4, CGCK_PCB_NCLASS = 5 };
#define CGCK_PCB_NCOUNT 6       /* [kind] for the five kinds, [5] HITs on IPv6 frames */

int cgck_pcb_lookup(cgck_ctx_t *ctx, const void *base, const cgck_desc_t *desc, const cgck_seg_t *seg,
		    const uint8_t *cls /* or NULL: every frame TCP */, uint64_t n,
		    const cgck_pcb_t *pcb, const cgck_pcb_res_t *res, void *stream);

/* The first reply either stack sends: tcp_respond's RST for a TCP segment that
 * found no PCB (bsd44/tcp_input.c:128-129, 881-899; tcp_subr.c:93-123), for a whole
 * burst on the device.  cgck_l4_desc's records, cgck_pcb_lookup's kinds and the
 * verify's verdicts go in; the segment records and the flow records that
 * cgck_l4_build takes come out, so no host pass over frame bytes lies between the
 * receive burst and the transmit burst.  A MISS frame has fidx = 0xFFFFFFFF: no
 * entry of the caller's flow[] fits it, and its reply's addresses are the received
 * frame's, swapped, which is why this call reads the frames.  The rule is stateless:
 * with tp == NULL tcp_respond reads nothing but the received segment.  Everything
 * with tp != NULL (keepalives, ACKs, which segment to send) stays the caller's
 * (DESIGN.md §6).
 *
 * Contract, total over every input byte string.  For frame k: s = seg[k]; c = cls ?
 * cls[k] & 15 : CGCK_SEG_TCP; kd = kind ? kind[k] : CGCK_PCB_MISS; vd = verdict ?
 * verdict[k] : 0; lc = l2cls ? l2cls[k] : 0; b the ip_len bytes at base + frame_off +
 * l3_off; v = b[0] >> 4.  The class, by these rules in order:
 *  1. c != CGCK_SEG_TCP: SKIP.  (A UDP miss draws icmp_error's port unreachable,
 *     which cgck_l4_build cannot build: it stays the caller's.)
 *  2. kd != CGCK_PCB_MISS: NOTMISS.
 *  3. vd & vmask: DROPPED.  vmask is the caller's checksum policy: CGCK_BAD_LEN,
 *     with CGCK_BAD_IP when t_ip_do_incksum != 0 (ip_input.c:50-57 returns on a bad
 *     sum) and CGCK_BAD_L4 when t_tcp_do_incksum > 1 (tcp_input.c:77-85 drops only
 *     then; at 1 it counts the bad sum and goes on).
 *  4. cgck_pcb_lookup's rule 2, word for word: NONE when ip_len == 0, when v == 4
 *     with ip_len < 20, when v == 6 with ip_len < 40, and for any other v.  ip_len
 *     bounds every read; the header's own length fields are not consulted.
 *  5. QUIET with flags & CGCK_RPL_NO_RST and s.th_flags & 0x04; and with flags &
 *     CGCK_RPL_NO_MCAST when lc & (CGCK_L2_BCAST | CGCK_L2_MCAST), or v == 4 with
 *     (b[16] >> 4) == 14, or v == 6 with b[24] == 0xFF.  This is 4.4BSD's test, which
 *     the reference has commented out (tcp_input.c:887-890): with flags == 0 the call
 *     is the reference's behaviour and answers an RST with an RST.
 *  6. RST.
 * The reply record r of an RST is zero except: r.sport = s.dport and r.dport =
 * s.sport, as stored; with s.th_flags & 0x10, r.seq = s.ack and r.th_flags = 0x04;
 * otherwise r.ack = s.seq + s.pay_len + (s.th_flags & 0x02 ? 1 : 0) modulo 2^32 and
 * r.th_flags = 0x14.  win, opt and pay_len are 0 (tcp_subr.c:115-116).
 * The reply flow f of an RST: eth_dst, eth_src, vlan_tci and ttl are link's (the
 * reference sends from its configured MACs, ip_output.c:67-68, not the frame's
 * swapped ones); flags = (link.flags & CGCK_FLOW_VLAN) | (v == 6 ? CGCK_FLOW_IP6 :
 * 0); laddr = the frame's destination (v4: b[16..20) and twelve zero bytes, v6:
 * b[24..40)); faddr = its source (b[12..16) or b[8..24)).
 * Every other class yields an all-zero r and f.
 * The class byte is class | CGCK_RPL_IP6, the flag set whenever ip_len > 0 and v ==
 * 6.  It is cgck_l4_build's in.cls: CGCK_RPL_RST == CGCK_SEG_TCP, every other class
 * is one its rule 1 skips, and the flag is CGCK_SEG_IP6.
 *
 * Outputs.  seg, flow and cls are indexed by a = at ? at[k] : k; a frame with a >= n
 * writes none of the three and is still counted.  Two frames with one `at` value
 * are the caller's error: which of them lands is unspecified, as for overlapping
 * slots in cgck_l4_build.  queue[k] (always at k) = 0 for an RST and 0xFF otherwise:
 * cgck_steer's input with queue_num 1.  count[class] += 1 per frame and count[7] +=
 * 1 per RST on an IPv6 frame (count[1] stays: no class has that value).
 *
 * cgck_l4_reply_packed: the replies in the reference's slot and id order.  The
 * reference hands out one transmit slot and one ip_id per packet sent (tx_alloc,
 * ip_output.c:40,52), not per packet received.  On one stream: cgck_l4_reply with
 * queue = pk->queue alone; cgck_steer(pk->queue, n, 1, NULL, {qoff = pk->qoff, slot =
 * pk->at}, pk->work); cgck_l4_reply with in.at = pk->at and the caller's res, whose
 * counters are therefore counted once.  Afterwards qoff[1] = R, the number of RSTs;
 * seg[0..R) and flow[0..R) are the RSTs in arrival order; cls[R..n) holds the other
 * classes, and seg and flow there are zero.  A cgck_l4_build over n with fidx = NULL,
 * in.cls = cls and ip_id0 fills slots 0..R-1 with ids ip_id0 + r, as tcp_respond
 * would, and skips the rest; a caller that has read qoff[1] builds over R.  The
 * caller owns pk's arrays: queue u8[n], at u32[n], qoff u32[3], work of
 * cgck_steer_work_bytes(n, 1) bytes (0 up to 4096 frames: work may then be NULL).
 * in->at must be NULL.
 *
 * cgck_l4_reply_rule: the rule for one frame in host memory; the same source text
 * as the kernel's.  Returns the class byte and fills *r and *f.  Pure: no device,
 * no context.  It is what a host-resident burst uses.  -EINVAL: a NULL s, link, r
 * or f, a NULL ip with ip_len > 0, and the flags and link.flags cgck_l4_reply
 * refuses.
 *
 * Execution.  Asynchronous on `stream` (NULL: the context's).  n == 0 returns 0,
 * launches nothing and writes nothing.  The inputs and the frames are never
 * written.  The library keeps no scratch.  One kernel, l4r_kernel, a lane per
 * frame; every read of a frame lies inside the 16-byte granules that hold a byte
 * of [frame, frame + ip_len) (cgck_rss_desc's rule); plain vector stores; no lane
 * or workgroup waits for another.  DESIGN.md §5.16 has the design.
 * -EINVAL: a NULL ctx, base, in or res; with n > 0 a NULL desc or seg; every output
 * NULL; a desc, at or count that is not 4-byte aligned, a seg or flow (on either
 * side) that is not 16-byte aligned; link.flags with a bit outside CGCK_FLOW_IP6 |
 * CGCK_FLOW_VLAN (the template's IP6 bit is ignored); flags with an unknown bit; an
 * output seg equal to the input seg.  The packed form adds: a NULL pk, queue, at or
 * qoff; a non-NULL in->at; a misaligned at, qoff or work; n above 0xFFFFFFFF; a NULL
 * work while cgck_steer_work_bytes(n, 1) != 0.  The argument checks come before any
 * device work.
 * Out of scope: ICMP unreachables for UDP misses and echo replies
 * (the builder has no ICMP); replies on a live connection; a strided form. */
enum { CGCK_RPL_RST = 0, CGCK_RPL_SKIP = 2, CGCK_RPL_NOTMISS = 3, CGCK_RPL_DROPPED = 4, CGCK_RPL_NONE = 5,
       CGCK_RPL_QUIET = 6, CGCK_RPL_NCLASS = 7 };              /* low nibble of cls[k]; 1 is no class */
enum { CGCK_RPL_IP6 = 1u << 4 };                               /* flag bit of cls[k] */
enum { CGCK_RPL_NO_RST = 1, CGCK_RPL_NO_MCAST = 2 };           /* flags */
#define CGCK_RPL_NCOUNT 8       /* [class] for the seven class values, [7] RSTs on IPv6 frames */

typedef struct cgck_l4_reply_in {       /* pointers are device memory */
	const cgck_desc_t *desc;            /* [n] the received frames */
	const cgck_seg_t  *seg;             /* [n] cgck_l4_desc's records, 16-byte aligned */
	const uint8_t *cls, *kind, *verdict, *l2cls;   /* [n] each, or NULL (see the rule) */
	const uint32_t *at;                 /* [n] or NULL: frame k's outputs go to index at[k] (NULL: k) */
	cgck_flow_t link;                   /* by value, host memory: MACs, vlan_tci, flags & VLAN, ttl */
	uint8_t vmask;
	uint32_t flags;                     /* CGCK_RPL_NO_RST | CGCK_RPL_NO_MCAST */
} cgck_l4_reply_in_t;

typedef struct cgck_l4_reply_res {      /* device memory; each optional; at least one non-NULL */
	cgck_seg_t  *seg;                   /* [n], 16-byte aligned */
	cgck_flow_t *flow;                  /* [n], 16-byte aligned: cgck_l4_build's flow with fidx NULL */
	uint8_t     *cls;                   /* [n] class | CGCK_RPL_IP6: cgck_l4_build's in.cls */
	uint8_t     *queue;                 /* [n] 0 for an RST, 0xFF otherwise: cgck_steer's input, queue_num 1 */
	uint32_t    *count;                 /* u32[CGCK_RPL_NCOUNT] running counters (+=) */
} cgck_l4_reply_res_t;

typedef struct cgck_l4_reply_pack {     /* device memory, the caller's; cgck_l4_reply_packed's intermediates */
	uint8_t  *queue;                    /* [n] */
	uint32_t *at;                       /* [n] the slot of frame k: RSTs first, in arrival order */
	uint32_t *qoff;                     /* u32[3], written: {0, R, n} */
	void     *work;                     /* cgck_steer_work_bytes(n, 1) bytes, or NULL when that is 0 */
} cgck_l4_reply_pack_t;

int cgck_l4_reply(cgck_ctx_t *ctx, const void *base, uint64_t n, const cgck_l4_reply_in_t *in,
		  const cgck_l4_reply_res_t *res, void *stream);
int cgck_l4_reply_packed(cgck_ctx_t *ctx, const void *base, uint64_t n, const cgck_l4_reply_in_t *in,
			 const cgck_l4_reply_res_t *res, const cgck_l4_reply_pack_t *pk, void *stream);
int cgck_l4_reply_rule(const cgck_seg_t *s, uint8_t cls, uint8_t kind, uint8_t verdict, uint8_t vmask,
		       uint8_t l2cls, uint32_t flags, const uint8_t *ip, uint32_t ip_len, const cgck_flow_t *link,
		       cgck_seg_t *r, cgck_flow_t *f);

/* One dst-cache entry: the fields thread_init_dst_cache fills in struct
 * ip_socket (con-gen.c:344-349; subr.h:218-228).  16 bytes. */
typedef struct cgck_dst_entry {
	uint32_t laddr; /* ipso_laddr, network order */
	uint32_t faddr; /* ipso_faddr, network order */
	uint16_t lport; /* ipso_lport, network order */
	uint16_t fport; /* ipso_fport, network order */
	uint32_t hash;  /* ipso_hash = SO_HASH(faddr, lport, fport) (subr.h:179-180) */
} cgck_dst_entry_t;

/* The struct thread fields the loop reads (subr.h:274-279, 325-328). */
typedef struct cgck_dst_params {
	uint32_t laddr_min, laddr_max; /* t_ip_laddr_min/max, host order */
	uint32_t faddr_min, faddr_max; /* t_ip_faddr_min/max, host order */
	uint16_t fport;                /* t_port, network order */
	uint8_t rss_queue_num;         /* t_rss_queue_num */
	uint8_t rss_queue_id;          /* t_rss_queue_id; the filter runs only when
	                                  id < 128 (RSS_QUEUE_ID_MAX) and num > 1 */
	const unsigned char *rss_key;  /* t_rss_key (host memory; unused without the filter) */
	int rss_key_size;              /* t_rss_key_size */
} cgck_dst_params_t;

/* Enumerate the candidate tuples in the reference's loop order (faddr
 * fastest, then the ephemeral lport 5000..65535, then laddr; the tuple count
 * is computed in 32-bit arithmetic as con-gen.c:314-315 does), keep those
 * whose rss_hash4 % queue_num == queue_id, and write the first `cap`
 * (t_dst_cache_size, >= 1) in order.  `*count` = entries written
 * (con-gen.c:356; the caller panics below t_concurrency, :357-358).
 * cgck_dst_cache: `out` and `count` are device memory, asynchronous.
 * cgck_dst_cache_host: host memory, synchronous. */
int cgck_dst_cache(cgck_ctx_t *ctx, const cgck_dst_params_t *prm, cgck_dst_entry_t *out, uint32_t cap,
		   uint32_t *count, void *stream);
int cgck_dst_cache_host(cgck_ctx_t *ctx, const cgck_dst_params_t *prm, cgck_dst_entry_t *out,
			uint32_t cap, uint32_t *count);

/* Plumbing for callers without their own runtime (tests, bench, C users).
 * A free while any burst server is resident is deferred until the last one
 * closes: hipFree / hipHostFree synchronise the device, which would wait for
 * the resident servers to idle out (the library's own buffers are handled
 * the same way). */
int cgck_device_count(void);
int cgck_dev_alloc(size_t bytes, void **ptr);
int cgck_dev_free(void *ptr);
int cgck_host_alloc(size_t bytes, void **ptr); /* pinned */
int cgck_host_free(void *ptr);
int cgck_memcpy(void *dst, const void *src, size_t bytes, void *stream); /* async, any direction */
int cgck_memset(void *dst, int value, size_t bytes, void *stream);

/* Name of the last checksum / hash kernel the context's dispatcher launched,
 * as rocprofv3 reports it (e.g. "cksum_kernel<16, 6, 1, false, true>");
 * "" before the first launch. */
const char *cgck_ctx_last_kernel(cgck_ctx_t *ctx);

/* HIP-event timing on a given stream (NULL = context stream). */
typedef struct cgck_event cgck_event_t;
int cgck_event_create(cgck_event_t **ev);
int cgck_event_destroy(cgck_event_t *ev);
int cgck_event_record(cgck_ctx_t *ctx, cgck_event_t *ev, void *stream);
int cgck_event_elapsed_ms(cgck_event_t *start, cgck_event_t *stop, float *ms);

/* Diagnostics: a plain coalesced streaming read of [src, src+bytes) (device
 * memory, 16-byte aligned) with minimal arithmetic — the practical HBM-read
 * ceiling the checksum kernels are compared with.  `sink` is a device u32. */
int cgck_probe_read(cgck_ctx_t *ctx, const void *src, uint64_t bytes, uint32_t *sink, void *stream);

/* Test hooks (tests/test_gpu_burst_seq.py; not for production callers).
 * cgck_test_burst_seq restarts ctx's open, idle burst server as if `seq` were
 * the last request served (the 32-bit seq wrap test); cgck_test_burst_stale
 * sets the done words of workgroups >= from half the seq space ahead (a word
 * untouched for 2^31 requests), which the next request must refresh.
 * -EINVAL: no server open, or a posted request not yet collected. */
int cgck_test_burst_seq(cgck_ctx_t *ctx, uint32_t seq);
int cgck_test_burst_stale(cgck_ctx_t *ctx, uint32_t from);
/* The route a host-resident request would take on a burst server opened with
 * (max_pkts, max_bytes), written into name[cap]: "launch", "refused"
 * (cgck_burst_request fails), or which of the server's compiled bodies serves
 * it, e.g. "one/lds/sys/g16u1/fl" or "wide32/slice/inplace/g4u4+u1/rt/2passes"
 * ("Burst server", has the table).  mem: 0 cgck_desc_host on pageable memory,
 * 1 on registered memory, 2 cgck_burst_request; posted: a window's posted
 * request; max_len: the longest ip_len; pkt_bytes: the packets' bytes, each
 * padded to 16; flags: as posted; n1: a two-part request's split, or 0.
 * Needs no device and no context.  cgck_test_burst_route_kind writes the i-th
 * kind of body a name can stand for and returns 1 when a request to this
 * library can reach it, 0 when only the lab build's options do, -ENOENT past
 * the last. */
int cgck_test_burst_route(uint32_t max_pkts, size_t max_bytes, int mem, int posted, uint64_t n, uint32_t max_len,
                          uint64_t pkt_bytes, uint32_t flags, uint32_t n1, char *name, size_t cap);
int cgck_test_burst_route_kind(uint32_t i, char *kind, size_t cap);
/* The geometry cgck_steer uses for (n, queue_num): frames per tile (a multiple of
 * 256, doubling from 4096 so that tiles x (queue_num + 1) stays within 262144
 * words), tiles = ceil(n / tile), and cgck_steer_work_bytes' value.  Each output
 * pointer may be NULL.  Needs no device and no context.  -EINVAL: queue_num
 * outside 1..128 or n above 0xFFFFFFFF. */
int cgck_test_steer_plan(uint64_t n, uint32_t queue_num, uint32_t *tile, uint32_t *tiles, size_t *work_bytes);
/* Frames one pass of cgck_l2_desc's grid covers on ctx's device: the launcher's
 * workgroup cap (four per compute unit) x 256.  A burst above twice that makes
 * every wave run three steps.  -EINVAL: a NULL ctx or frames. */
int cgck_test_l2_pass(cgck_ctx_t *ctx, uint64_t *frames);
/* The same for cgck_l4_desc's grid. */
int cgck_test_l4_pass(cgck_ctx_t *ctx, uint64_t *frames);
/* The same for cgck_l4_build's grid. */
int cgck_test_l4_build_pass(cgck_ctx_t *ctx, uint64_t *frames);
/* Pin the store shape of l4b_kernel for every later cgck_l4_build of the process (the tests of both
 * shapes and the A/B of tools/l4b_ab.py): 0 the product's choice, 1 every dword from
 * its own lane (l4b_kernel<.., false>), 2 whole 16-byte granules turned through LDS (<.., true>).
 * Returns the previous value; -EINVAL for any other. */
int cgck_test_l4_build_store(int shape);
/* The same as cgck_test_l4_pass for cgck_pcb_lookup's grid. */
int cgck_test_pcb_pass(cgck_ctx_t *ctx, uint64_t *frames);
/* Pin how every later cgck_pcb_build and cgck_pcb_lookup of the process work (the tests and the A/B of
 * tools/pcb_ab.py); a table is looked up under the mode it was built under.  Bit 0:
 * every key's home slot is the table's last slot, which forces the longest chain and the wrap-around.
 * Bit 1: the A/B's other table shape, 4-byte slots that hold the index alone (pcbb_kernel<false>,
 * pcbl_kernel<.., false>).  Returns the previous value; -EINVAL outside 0..3. */
int cgck_test_pcb_mode(int mode);
/* The same as cgck_test_l4_pass for cgck_l4_reply's grid. */
int cgck_test_l4_reply_pass(cgck_ctx_t *ctx, uint64_t *frames);
/* Pin how l4r_kernel stores seg and flow under `at` for every later cgck_l4_reply of the process (the
 * tests of both shapes and the A/B of tools/l4r_ab.py): 0 the product's choice, 1 a lane
 * stores its own 16-byte pieces (l4r_kernel<.., 1>), 2 the pieces and their targets are turned through
 * LDS so that one store instruction covers whole records of consecutive frames (l4r_kernel<.., 2>).
 * Without `at` the records always leave turned, as consecutive pieces.  Returns the previous value;
 * -EINVAL for any other. */
int cgck_test_l4_reply_store(int shape);
/* cgck_toeplitz's launch geometry on ctx's device.  records: what one pass of the
 * per-record kernel's grid covers (its workgroup cap, eight per compute unit, x 256);
 * a batch above twice that makes every lane run three passes.  groups: the 4-record
 * groups the dense kernel's register ring holds before it wraps (its workgroups x 256
 * lanes x the ring depth).  -EINVAL: a NULL ctx, records or groups. */
int cgck_test_rss_pass(cgck_ctx_t *ctx, uint64_t *records, uint64_t *groups);

#ifdef __cplusplus
}
#endif
#endif /* CGCK_H */
