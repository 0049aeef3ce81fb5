// cgck_api.cpp — host side of libcgck.so: the C-ABI declared in
// include/cgck.h.  Contexts (stream + staging), device-resident and
// host-resident batches, registered rings, the Toeplitz RSS batch and
// dst-cache entry points, synthetic generation and timing.  The burst
// server's host side is in cgck_burst.cpp, the drop-in symbols and the
// per-thread RX / TX windows are in cgck_dropin.cpp.
//
// Every checksum this library returns is computed by the gfx950 kernels
// (cgck_group.hip, cgck_lane.hip); there is no host arithmetic path.  Without
// a usable device every entry point fails with -ENODEV.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <shared_mutex>
#include <vector>

#include "cgck_host.h"
#include "cgck_pcb_probe.h"
#include "cgck_reply_rule.h"
#include "cgck_steer_plan.h"

using namespace cgck;

// --------------------------------------------------------------------------
// Errors
// --------------------------------------------------------------------------

static thread_local char t_err[256];

int cgck::set_err(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(t_err, sizeof(t_err), fmt, ap);
	va_end(ap);
	return code;
}

const char *cgck::err_text() { return t_err; }

extern "C" const char *cgck_last_error(void) { return t_err; }
extern "C" int cgck_abi_version(void) { return CGCK_ABI_VERSION; }

// --------------------------------------------------------------------------
// Context
// --------------------------------------------------------------------------

static void rss_users_free(cgck_ctx *c);

struct cgck_event {
	hipEvent_t ev;
};

int cgck::grow_host(void **p, size_t *cap, size_t need)
{
	if (need <= *cap)
		return 0;
	size_t n = need < 4096 ? 4096 : need + need / 2;
	if (*p)
		free_or_park(*p, true);
	*p = nullptr;
	*cap = 0;
	HIP_TRY(hipHostMalloc(p, n, hipHostMallocDefault));
	*cap = n;
	return 0;
}

int cgck::grow_dev(void **p, size_t *cap, size_t need)
{
	if (need <= *cap)
		return 0;
	size_t n = need < 65536 ? 65536 : need + need / 4;
	if (*p)
		free_or_park(*p, false);
	*p = nullptr;
	*cap = 0;
	HIP_TRY(hipMalloc(p, n));
	*cap = n;
	return 0;
}

extern "C" int cgck_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

// Kernel family by name (cgck_ctx_set_kernel, kFamilyNames).  The product
// library knows its own families; the lab build also the A/B-only ones and
// raw numbers (tools/sweep.py, $CGCK_KERNEL).  -1: unknown.
static int family_of(const char *kf)
{
	for (const auto &f : kFamilyNames)
		if (!strcmp(kf, f.name) && (CGCK_LAB || !f.lab_only))
			return f.family;
#if CGCK_LAB
	if (!strncmp(kf, "lpp", 3))
		return atoi(kf + 3);
	if (*kf >= '0' && *kf <= '9')
		return atoi(kf);
#endif
	return -1;
}

extern "C" int cgck_ctx_create(int device, cgck_ctx_t **out)
{
	if (!out)
		return set_err(-EINVAL, "cgck_ctx_create: out is NULL");
	*out = nullptr;
	int n = cgck_device_count();
	if (n <= 0)
		return set_err(-ENODEV, "cgck: no HIP device visible (gfx950 required)");
	if (device < 0 || device >= n)
		return set_err(-ENODEV, "cgck: device %d out of range (%d visible)", device, n);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return set_err(-ENODEV, "cgck: device %d is %s, this build targets gfx950", device,
			       prop.gcnArchName);
	cgck_ctx *c = (cgck_ctx *)calloc(1, sizeof(*c));
	if (!c)
		return set_err(-ENOMEM, "cgck_ctx_create: out of memory");
	c->device = device;
	c->num_cus = prop.multiProcessorCount;
	c->last_kernel = "";
	c->desc_len_hint = 1500;
	if (const char *kf = CGCK_ENV("CGCK_KERNEL")) // lab build only
		c->family = family_of(kf);
	hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
	if (e != hipSuccess) {
		free(c);
		return set_err(-EIO, "hipStreamCreate: %s", hipGetErrorString(e));
	}
	if ((e = hipMalloc(&c->d_zero, kZeroBytes)) != hipSuccess ||
	    (e = hipMemset(c->d_zero, 0, kZeroBytes)) != hipSuccess) {
		(void)hipStreamDestroy(c->stream);
		free(c);
		return set_err(-EIO, "zero chunk: %s", hipGetErrorString(e));
	}
	*out = c;
	return 0;
}

extern "C" int cgck_ctx_set_kernel(cgck_ctx_t *c, const char *name)
{
	if (!c || !name)
		return set_err(-EINVAL, "cgck_ctx_set_kernel: NULL argument");
	const int f = family_of(name);
	if (f < 0)
		return set_err(-EINVAL, "cgck_ctx_set_kernel: unknown kernel family \"%s\"", name);
	c->family = f;
	return 0;
}

extern "C" int cgck_ctx_destroy(cgck_ctx_t *c)
{
	if (!c)
		return 0;
	(void)hipSetDevice(c->device);
	if (c->srv.box)
		(void)cgck_burst_close(c);
	(void)CGCK_SYNC(c->stream);
	(void)hipStreamDestroy(c->stream);
	for (void *h : {(void *)c->h_stage, (void *)c->h_out})
		if (h)
			free_or_park(h, true);
	for (void *d : {(void *)c->d_bytes, (void *)c->d_aux, c->d_zero, (void *)c->d_rss_tab, (void *)c->d_dst})
		if (d)
			free_or_park(d, false);
	rss_users_free(c);
	free(c->h_rss_tab);
	free(c->rss_key);
	free(c);
	return 0;
}

extern "C" void *cgck_ctx_stream(cgck_ctx_t *c) { return c ? (void *)c->stream : nullptr; }

extern "C" const char *cgck_ctx_last_kernel(cgck_ctx_t *c) { return c && c->last_kernel ? c->last_kernel : ""; }

extern "C" int cgck_ctx_sync(cgck_ctx_t *c)
{
	if (!c)
		return set_err(-EINVAL, "cgck_ctx_sync: NULL context");
	HIP_TRY(CGCK_SYNC(c->stream));
	return 0;
}

extern "C" int cgck_set_desc_len_hint(cgck_ctx_t *c, uint32_t max_ip_len)
{
	if (!c)
		return set_err(-EINVAL, "cgck_set_desc_len_hint: NULL context");
	c->desc_len_hint = max_ip_len ? max_ip_len : 1500;
	return 0;
}

extern "C" int cgck_set_desc_layout(cgck_ctx_t *c, uint32_t layout)
{
	if (!c)
		return set_err(-EINVAL, "cgck_set_desc_layout: NULL context");
	if (layout > CGCK_LAYOUT_PACKED)
		return set_err(-EINVAL, "cgck_set_desc_layout: unknown layout %u", layout);
	c->desc_layout = layout;
	return 0;
}

static inline hipStream_t pick(cgck_ctx *c, void *stream)
{
	return stream ? (hipStream_t)stream : c->stream;
}

// --------------------------------------------------------------------------
// Device-resident batches
// --------------------------------------------------------------------------

// *flags comes back as the kernels take it: RAW | IP6 is RAW (a raw region
// has no header semantics of either family).
static int check_flags(uint32_t *flagsp)
{
	const uint32_t flags = *flagsp;
	const uint32_t known = CGCK_RAW | CGCK_IP | CGCK_L4 | CGCK_L4_NOPSEUDO | CGCK_ZERO_FIELDS |
			       CGCK_STORE | CGCK_VERIFY | CGCK_V_IP_ZERO_IS_FFFF | CGCK_V_UDP_ZERO_SKIP | CGCK_IP6 |
			       CGCK_MIXED;
	if (flags & ~known)
		return set_err(-EINVAL, "cgck: unknown flag bits 0x%x", flags & ~known);
	if ((flags & CGCK_MIXED) && (flags & (CGCK_RAW | CGCK_IP6 | CGCK_L4_NOPSEUDO | CGCK_STORE)))
		return set_err(-EINVAL, "cgck: CGCK_MIXED decides the family and the ICMP rule per packet and stores "
					"nothing: it excludes CGCK_RAW, CGCK_IP6, CGCK_L4_NOPSEUDO and CGCK_STORE");
	if ((flags & CGCK_RAW) && (flags & ~(CGCK_RAW | CGCK_IP6)))
		return set_err(-EINVAL, "cgck: the RAW flag excludes every other flag");
	if ((flags & CGCK_IP6) && (flags & CGCK_L4_NOPSEUDO))
		return set_err(-EINVAL, "cgck: CGCK_L4_NOPSEUDO has no meaning with CGCK_IP6 (every IPv6 upper-layer "
					"checksum covers the pseudo-header)");
	if (flags & CGCK_RAW)
		*flagsp = CGCK_RAW;
	if (!(flags & (CGCK_RAW | CGCK_IP | CGCK_L4)))
		return set_err(-EINVAL, "cgck: flags select no checksum (RAW, IP or L4)");
	return 0;
}

int cgck::run(cgck_ctx *c, const KParams &p0, uint32_t len_hint, hipStream_t st)
{
	HIP_TRY(hipSetDevice(c->device));
	KParams p = p0;
	p.zero = c->d_zero;
	hipError_t e = launch_cksum(p, len_hint, c->num_cus, c->family | (c->desc_layout ? kPacked : 0), st);
	if (e != hipSuccess)
		return set_err(-EIO, "cksum launch: %s", hipGetErrorString(e));
	if (p.n)
		c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_strided(cgck_ctx_t *c, void *base, uint64_t n, uint64_t stride, uint32_t l3_off,
			    uint32_t ip_len, uint32_t flags, uint32_t *out, uint8_t *verdict,
			    uint32_t *bad, void *stream)
{
	if (!c)
		return set_err(-EINVAL, "cgck_strided: NULL context");
	int rc = check_flags(&flags);
	if (rc)
		return rc;
	if ((flags & (CGCK_IP6 | CGCK_MIXED)) && ip_len > 65535)
		return set_err(-EINVAL, "cgck_strided: CGCK_IP6 and CGCK_MIXED take ip_len <= 65535 (no jumbograms)");
	if (n && !base)
		return set_err(-EINVAL, "cgck_strided: NULL base");
	if (ip_len > 0x7fffffffu)
		return set_err(-EINVAL, "cgck_strided: ip_len too large");
	KParams p = {(const uint8_t *)base, nullptr, n, stride, l3_off, ip_len, flags, out, verdict, bad, 0, nullptr};
	return run(c, p, ip_len, pick(c, stream));
}

extern "C" int cgck_desc(cgck_ctx_t *c, void *base, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
			 uint32_t *out, uint8_t *verdict, uint32_t *bad, void *stream)
{
	if (!c)
		return set_err(-EINVAL, "cgck_desc: NULL context");
	int rc = check_flags(&flags);
	if (rc)
		return rc;
	if (n && (!base || !desc))
		return set_err(-EINVAL, "cgck_desc: NULL base or descriptors");
	if (((uintptr_t)desc & 3) != 0)
		return set_err(-EINVAL, "cgck_desc: descriptors must be 4-byte aligned");
	KParams p = {(const uint8_t *)base, desc, n, 0, 0, 0, flags, out, verdict, bad, 0, nullptr};
	return run(c, p, c->desc_len_hint, pick(c, stream));
}

// --------------------------------------------------------------------------
// Host-resident batch
// --------------------------------------------------------------------------
//
// Three ways in, by what the caller's memory is:
//  * registered ring memory (cgck_host_register: the netmap pool, XDP UMEM,
//    DPDK mempool): the kernel reads the packets over the fabric where they
//    lie and in-place stores land there — no copy of the packet bytes;
//  * a small pageable burst (packet bytes <= kStageBytes): the CPU copies
//    each packet into this context's pinned staging and the kernel reads the
//    staging — one launch and one synchronisation, the RX-burst latency path
//    (a DMA from pageable memory costs more than the copy at these sizes);
//  * a large pageable batch: DMA of [base, base + bytes) into device scratch.
// Descriptors and per-packet outputs pass through pinned staging in the first
// two cases.

static constexpr size_t kStageBytes = 512 << 10;

// [p, p + bytes) inside one registered host allocation: its device pointer
static void *registered_ptr(void *p, size_t bytes)
{
	hipPointerAttribute_t a, b;
	if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost || !a.devicePointer) {
		(void)hipGetLastError();
		return nullptr;
	}
	void *end = (uint8_t *)p + bytes - 1;
	if (hipPointerGetAttributes(&b, end) != hipSuccess || b.type != hipMemoryTypeHost ||
	    (uint8_t *)b.devicePointer - (uint8_t *)a.devicePointer != (ptrdiff_t)(bytes - 1)) {
		(void)hipGetLastError();
		return nullptr;
	}
	return a.devicePointer;
}

// Does every descriptor lie inside the `bytes` given?  -EINVAL in `who`'s name
// otherwise.  sum (optional): the longest ip_len and the packets' bytes, each
// padded to 16.
static int desc_range_check(const char *who, const cgck_desc_t *desc, uint64_t n, size_t bytes, DescSummary *sum = nullptr)
{
	DescSummary s = {0, 0};
	for (uint64_t i = 0; i < n; i++) {
		s.max_len = desc[i].ip_len > s.max_len ? desc[i].ip_len : s.max_len;
		const uint64_t end = desc[i].frame_off + desc[i].l3_off + desc[i].ip_len;
		if (end > bytes || end < desc[i].frame_off)
			return set_err(-EINVAL, "%s: descriptor %llu reaches past the %zu bytes given", who,
				       (unsigned long long)i, bytes);
		s.pkt_bytes += ((size_t)desc[i].ip_len + 15) & ~(size_t)15;
	}
	if (sum)
		*sum = s;
	return 0;
}

// Copy each packet of [base, ...) to a 16-byte-padded offset of `dst` and
// describe it there: d[i] is desc[i]'s packet relative to dst.
static void gather_packets(uint8_t *dst, cgck_desc_t *d, const void *base, const cgck_desc_t *desc, uint64_t n)
{
	size_t at = 0;
	for (uint64_t i = 0; i < n; i++) {
		memcpy(dst + at, (const uint8_t *)base + desc[i].frame_off + desc[i].l3_off, desc[i].ip_len);
		d[i].frame_off = at;
		d[i].l3_off = 0;
		d[i].ip_len = desc[i].ip_len;
		at += ((size_t)desc[i].ip_len + 15) & ~(size_t)15;
	}
}

// desc_host, or (pend != nullptr) its posted form: when the request goes to
// the burst server it is left posted and *pend records where its outputs go
// (1 is returned; burst_collect finishes it), otherwise it is computed at
// once (0).
// sum: a summary the library computed itself while building the
// descriptors (they lie inside [base, base + bytes) by construction): the
// per-descriptor pass is skipped.
static int desc_host_impl(cgck_ctx *c, void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
			  uint32_t *out, uint8_t *verdict, uint32_t *meta, BurstPending *pend,
			  const DescSummary *sum = nullptr, const DescSplit *split = nullptr)
{
	if (n == 0)
		return 0;
	if (split && (split->n1 == 0 || split->n1 >= n))
		split = nullptr;
	if (!base || !desc)
		return set_err(-EINVAL, "cgck_desc_host: NULL base or descriptors");
	int rc;
	DescSummary own;
	if (!sum && (rc = desc_range_check("cgck_desc_host", desc, n, bytes, &own)))
		return rc;
	const size_t pkt_bytes = (sum ? sum : &own)->pkt_bytes;
	const uint32_t max_len = (sum ? sum : &own)->max_len;
	// Kernel shape from the context's length hint (default 1500: the group
	// kernel's 16 packets per block), not from the batch: a host-resident
	// burst is bound by PCIe round trips, which many small blocks overlap —
	// 256 x 64 B RX-window frames took 31 us at 256 packets per block (G4)
	// against 19 us at 16 (tools/txburst).
	const uint32_t hint = c->desc_len_hint;
	hipStream_t st = c->stream;
	// registered through cgck_host_register (the per-thread cached lookup),
	// else whatever HIP knows of the memory (a caller's hipHostMalloc)
	RegRange rr;
	void *dev_base = reg_find(base, bytes, &rr) ? (void *)(rr.dev + ((uint8_t *)base - rr.lo))
						    : registered_ptr(base, bytes);
	// Server requests copy the packet bytes into the request block (one wide
	// read) unless they are registered and either larger than that read or
	// stored to in place; a pageable batch with in-place stores takes the
	// launch path (the server's copy of the bytes is not written back).
	// A posted request (pend) reads registered memory in place whatever its
	// size: its latency is hidden, and copying the bytes would put them back
	// on the poster's thread.
	const bool store = flags & CGCK_STORE;
	const bool in_place = burst_in_place(dev_base != nullptr, store, pend != nullptr, pkt_bytes, n, kServerCopy);
	// (an IPv6 or mixed batch takes the launch path: the server's bodies are IPv4)
	if (burst_flags_ok(flags, in_place) &&
	    burst_fits(c, n, in_place ? 0 : pkt_bytes, pkt_bytes)) {
		// the resident server: no launch, no stream sync
		const BurstLayout L = burst_layout(in_place ? 0 : pkt_bytes, n);
		const BurstBlock blk = burst_next_block(c, L, pend != nullptr);
		uint8_t *h = blk.p;
		cgck_desc_t *d = (cgck_desc_t *)(h + L.d_off);
		if (in_place)
			memcpy(d, desc, 12 * n);
		else
			gather_packets(h + L.p_off, d, base, desc, n);
		uint32_t seq;
		if ((rc = burst_post(c, blk, in_place ? (const uint8_t *)dev_base : nullptr, bytes, n, flags, max_len, L,
				     &seq, split)))
			return rc;
		BurstPending now;
		BurstPending *q = pend ? pend : &now;
		*q = BurstPending{seq, (uint32_t)n, bytes, out, meta, verdict, 0};
		if (pend) {
			burst_hold(c, pend);
			return 1;
		}
		return burst_collect(c, &now);
	}
	// the launch paths below (the server's needs no current device: its
	// calls name their stream, and a relaunch sets it)
	HIP_TRY(hipSetDevice(c->device));
	if (split) {
		// a two-part request the server cannot take: each part computed at
		// once on its own (the launch path takes one flag set)
		const uint32_t n1 = split->n1;
		if ((rc = desc_host_impl(c, base, bytes, desc, n1, flags, out, verdict, meta, nullptr)))
			return rc;
		return desc_host_impl(c, base, bytes, desc + n1, n - n1, split->flags2, out ? out + n1 : nullptr,
				      verdict ? verdict + n1 : nullptr, nullptr, nullptr);
	}
	if (dev_base || pkt_bytes <= kStageBytes) {
		// pinned staging: [packets (staged case)] | descriptors | out | meta | verdict
		const size_t sbytes = dev_base ? 0 : pkt_bytes;
		const size_t d_off = sbytes, o_off = (d_off + 12 * n + 15) & ~(size_t)15, m_off = o_off + 4 * n,
			     v_off = m_off + (meta ? 4 * n : 0);
		if ((rc = grow_host((void **)&c->h_stage, &c->h_stage_cap, v_off + n)))
			return rc;
		uint8_t *h = c->h_stage;
		cgck_desc_t *d = (cgck_desc_t *)(h + d_off);
		if (dev_base)
			memcpy(d, desc, 12 * n);
		else
			gather_packets(h, d, base, desc, n);
		uint32_t *o = (uint32_t *)(h + o_off);
		uint32_t *m = meta ? (uint32_t *)(h + m_off) : nullptr;
		uint8_t *v = h + v_off;
		KParams p = {dev_base ? (const uint8_t *)dev_base : h, d, n, 0, 0, 0, flags, o, v, nullptr, 0, nullptr, m};
		if ((rc = run(c, p, hint, st)))
			return rc;
		HIP_TRY(CGCK_SYNC(st));
		if (out)
			memcpy(out, o, 4 * n);
		if (meta)
			memcpy(meta, m, 4 * n);
		if (verdict)
			memcpy(verdict, v, n);
		if ((flags & CGCK_STORE) && !dev_base)
			for (uint64_t i = 0; i < n; i++)
				memcpy((uint8_t *)base + desc[i].frame_off + desc[i].l3_off, h + d[i].frame_off,
				       desc[i].ip_len);
		return 0;
	}
	// a large pageable batch: DMA of [base, base + bytes) into device scratch
	const size_t dbytes = 12 * n, obytes = 4 * n, vbytes = n, mbytes = meta ? 4 * n : 0;
	if ((rc = grow_dev((void **)&c->d_bytes, &c->d_bytes_cap, bytes)))
		return rc;
	if ((rc = grow_dev((void **)&c->d_aux, &c->d_aux_cap, dbytes + obytes + mbytes + vbytes + 64)))
		return rc;
	uint8_t *d_desc = c->d_aux;
	uint32_t *d_out = (uint32_t *)(c->d_aux + ((dbytes + 15) & ~(size_t)15));
	uint32_t *d_meta = meta ? d_out + n : nullptr;
	uint8_t *d_ver = (uint8_t *)(d_out + n + (meta ? n : 0));
	HIP_TRY(hipMemcpyAsync(c->d_bytes, base, bytes, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_desc, desc, dbytes, hipMemcpyHostToDevice, st));
	KParams p = {c->d_bytes, (const cgck_desc_t *)d_desc, n, 0, 0, 0, flags, d_out, d_ver, nullptr, 0, nullptr, d_meta};
	if ((rc = run(c, p, hint, st)))
		return rc;
	if (out)
		HIP_TRY(hipMemcpyAsync(out, d_out, obytes, hipMemcpyDeviceToHost, st));
	if (meta)
		HIP_TRY(hipMemcpyAsync(meta, d_meta, mbytes, hipMemcpyDeviceToHost, st));
	if (verdict)
		HIP_TRY(hipMemcpyAsync(verdict, d_ver, vbytes, hipMemcpyDeviceToHost, st));
	uint8_t *back = nullptr;
	if (flags & CGCK_STORE) {
		// Only the packets' own spans go back: every other byte of [base,
		// base + bytes) may have changed since the H2D snapshot (the NIC or
		// the caller writing other slots of the ring).
		if ((rc = grow_host((void **)&c->h_stage, &c->h_stage_cap, bytes)))
			return rc;
		back = c->h_stage;
		HIP_TRY(hipMemcpyAsync(back, c->d_bytes, bytes, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(CGCK_SYNC(st));
	if (back)
		for (uint64_t i = 0; i < n; i++) {
			const size_t o = desc[i].frame_off + desc[i].l3_off;
			memcpy((uint8_t *)base + o, back + o, desc[i].ip_len);
		}
	return 0;
}

int cgck::desc_host(cgck_ctx *c, void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
		    uint32_t *out, uint8_t *verdict, uint32_t *meta)
{
	return desc_host_impl(c, base, bytes, desc, n, flags, out, verdict, meta, nullptr);
}

int cgck::desc_host_post(cgck_ctx *c, void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
			 uint32_t *out, uint8_t *verdict, uint32_t *meta, BurstPending *pend, const DescSummary *sum,
			 const DescSplit *split)
{
	pend->seq = 0;
	pend->rc = 0;
	return desc_host_impl(c, base, bytes, desc, n, flags, out, verdict, meta, pend, sum, split);
}

extern "C" int cgck_desc_host(cgck_ctx_t *c, void *base, size_t bytes, const cgck_desc_t *desc,
			      uint64_t n, uint32_t flags, uint32_t *out, uint8_t *verdict)
{
	if (!c)
		return set_err(-EINVAL, "cgck_desc_host: NULL context");
	int rc = check_flags(&flags);
	if (rc)
		return rc;
	return desc_host(c, base, bytes, desc, n, flags, out, verdict);
}

// One request to the context's burst server over device-visible memory the
// caller already holds (a registered ring's device view): no host-side check
// of the descriptors — the server checks each against `range` on the device
// before any load or store, and refuses the request (-EIO) otherwise.
extern "C" int cgck_burst_request(cgck_ctx_t *c, const void *dev_base, uint64_t range, const cgck_desc_t *desc,
				  uint64_t n, uint32_t flags, uint32_t *out, uint8_t *verdict)
{
	if (!c && !(c = thread_ctx()))
		return -ENODEV; // thread_ctx set the message
	const bool ip6 = flags & (CGCK_IP6 | CGCK_MIXED);
	int rc = check_flags(&flags);
	if (rc)
		return rc;
	if (ip6)
		return set_err(-EINVAL, "cgck_burst_request: the burst server has no IPv6 bodies (CGCK_IP6, CGCK_MIXED): "
					"use cgck_desc_host, which launches such a batch");
	if (!dev_base || !range || (n && !desc))
		return set_err(-EINVAL, "cgck_burst_request: NULL base, zero range or NULL descriptors");
	if (n == 0)
		return 0;
	uint32_t max_len = 0;
	for (uint64_t i = 0; i < n; i++)
		max_len = desc[i].ip_len > max_len ? desc[i].ip_len : max_len;
	if (!burst_fits(c, n, 0, 0))
		return set_err(-ENOSPC, "cgck_burst_request: no burst server open on the context, or %llu packets "
					"exceed its capacity", (unsigned long long)n);
	const BurstLayout L = burst_layout(0, n);
	const BurstBlock blk = burst_next_block(c, L);
	memcpy(blk.p + L.d_off, desc, 12 * n);
	uint32_t seq;
	if ((rc = burst_serve(c, blk, (const uint8_t *)dev_base, range, n, flags, max_len, L, &seq)))
		return rc;
	const uint8_t *o = burst_resp(c, seq);
	if (out)
		memcpy(out, o, 4 * n);
	if (verdict)
		memcpy(verdict, o + burst_ver_off((uint32_t)n), n);
	return 0;
}

// Ranges registered through cgck_host_register, so the deferred TX window
// can tell ring memory from a caller's stack or heap, and its flush read the
// queued packets where they lie.  Written only by register/unregister
// (set-up time); lookups take the reader side.
std::atomic<uint64_t> cgck::g_reg_gen{1}; // bumped by every register / unregister
namespace {
std::shared_mutex g_reg_mu;
std::vector<RegRange> g_reg;
// per thread: the range of the last hit, valid while the generation holds
__attribute__((tls_model("initial-exec"))) thread_local uint64_t t_reg_gen = 0;
__attribute__((tls_model("initial-exec"))) thread_local RegRange t_reg_last{nullptr, nullptr, nullptr};
} // namespace

bool cgck::reg_find(const void *p, size_t bytes, RegRange *r)
{
	const uint8_t *b = (const uint8_t *)p;
	if (t_reg_gen == g_reg_gen.load(std::memory_order_acquire) && b >= t_reg_last.lo && b < t_reg_last.hi &&
	    bytes <= (size_t)(t_reg_last.hi - b)) {
		*r = t_reg_last; // the TX window's per-call check: no lock on the hot path
		return true;
	}
	std::shared_lock<std::shared_mutex> lk(g_reg_mu);
	for (const RegRange &x : g_reg)
		if (b >= x.lo && b < x.hi && bytes <= (size_t)(x.hi - b)) {
			*r = x;
			t_reg_last = x;
			t_reg_gen = g_reg_gen.load(std::memory_order_acquire);
			return true;
		}
	return false;
}

// Memory of the brk heap is refused.  Rings carved out of the heap (numpy
// buffers in the tests, round 3's failing test among them) were read and
// written by the GPU at an address 64 KiB or 128 KiB away from the right one
// for a run of pages, intermittently: the allocator returns the heap's pages
// to the kernel and faults fresh ones in at the same addresses, and pages
// that moved under a registration stayed mapped to the GPU where they had
// been (the failing values are the frames'
// own at the shifted address; the same rings in mappings of their own were
// exact in every run).  A ring belongs in a mapping of its own — mmap, a
// hugetlbfs segment, a transport's pool — which nothing else in the process
// unmaps or re-faults while it is registered.
static bool in_brk_heap(const void *ptr, size_t bytes)
{
	FILE *f = fopen("/proc/self/maps", "r");
	if (!f)
		return false;
	char line[512];
	bool hit = false;
	const uintptr_t a = (uintptr_t)ptr, e = a + bytes;
	while (!hit && fgets(line, sizeof(line), f)) {
		unsigned long lo, hi;
		if (sscanf(line, "%lx-%lx", &lo, &hi) == 2 && strstr(line, "[heap]") && a < hi && e > lo)
			hit = true;
	}
	fclose(f);
	return hit;
}

extern "C" int cgck_host_register(void *ptr, size_t bytes)
{
	if (!ptr || !bytes)
		return set_err(-EINVAL, "cgck_host_register: NULL or empty range");
	if (in_brk_heap(ptr, bytes))
		return set_err(-EINVAL,
			       "cgck_host_register: [%p, +%zu) lies in the brk heap, whose pages the allocator returns "
			       "and re-faults under a registration; register a mapping of its own (mmap, hugetlbfs, the "
			       "transport's pool)",
			       ptr, bytes);
	MapChange map_c; // no request in flight, every server drained
	HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
	void *dev = nullptr;
	if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess || !dev) {
		(void)hipGetLastError();
		return 0; // registered; the TX flush just keeps staging for it
	}
	std::unique_lock<std::shared_mutex> lk(g_reg_mu);
	g_reg.push_back({(uint8_t *)ptr, (uint8_t *)ptr + bytes, (uint8_t *)dev});
	g_reg_gen.fetch_add(1, std::memory_order_acq_rel);
	return 0;
}

extern "C" int cgck_host_device_ptr(const void *ptr, size_t bytes, void **dev)
{
	if (!dev)
		return set_err(-EINVAL, "cgck_host_device_ptr: dev is NULL");
	*dev = nullptr;
	RegRange rr;
	if (!ptr || !reg_find(ptr, bytes, &rr))
		return set_err(-ENOENT, "cgck_host_device_ptr: [%p, +%zu) is not inside a registered range", ptr, bytes);
	*dev = rr.dev + ((const uint8_t *)ptr - rr.lo);
	return 0;
}

extern "C" int cgck_host_unregister(void *ptr)
{
	MapChange map_c; // no request in flight, every server drained
	{
		std::unique_lock<std::shared_mutex> lk(g_reg_mu);
		for (size_t i = 0; i < g_reg.size(); i++)
			if (g_reg[i].lo == (uint8_t *)ptr) {
				g_reg.erase(g_reg.begin() + i);
				break;
			}
		g_reg_gen.fetch_add(1, std::memory_order_acq_rel);
	}
	HIP_TRY(hipHostUnregister(ptr));
	return 0;
}

// --------------------------------------------------------------------------
// One region for the drop-in symbols (cgck_dropin.cpp): staged into pinned
// memory that the kernel reads over the fabric (or served by the resident
// burst server when one is open)
// --------------------------------------------------------------------------

int cgck::one_region(cgck_ctx *c, const void *src, uint32_t span, uint32_t ip_len, uint32_t flags, uint32_t *out)
{
	int rc;
	if (ip_len <= 0xffff && !(flags & CGCK_STORE) && burst_fits(c, 1, span, span)) {
		// the resident server: one descriptor, no launch, no stream sync
		const BurstLayout L = burst_layout(span, 1);
		const BurstBlock blk = burst_next_block(c, L);
		uint8_t *h = blk.p;
		if (span)
			memcpy(h + L.p_off, src, span);
		cgck_desc_t *d = (cgck_desc_t *)(h + L.d_off);
		d->frame_off = 0;
		d->l3_off = 0;
		d->ip_len = (uint16_t)ip_len;
		uint32_t seq;
		if ((rc = burst_serve(c, blk, nullptr, 0, 1, flags, ip_len, L, &seq)))
			return rc;
		*out = *(const uint32_t *)burst_resp(c, seq);
		return 0;
	}
	if ((rc = grow_host((void **)&c->h_stage, &c->h_stage_cap, span + 16)) ||
	    (rc = grow_host((void **)&c->h_out, &c->h_out_cap, 64)))
		return rc;
	if (span)
		memcpy(c->h_stage, src, span);
	KParams p = {c->h_stage, nullptr, 1, 0, 0, ip_len, flags | kFlagGroup, c->h_out, nullptr, nullptr, 0, nullptr};
	if ((rc = run(c, p, ip_len, c->stream)))
		return rc;
	HIP_TRY(CGCK_SYNC(c->stream));
	*out = c->h_out[0];
	return 0;
}

// --------------------------------------------------------------------------
// Toeplitz RSS hash and the dst-cache build
// --------------------------------------------------------------------------

// Byte tables of a key: T[i][v] = XOR of W(8i+b) over the set bits b of v
// (MSB first), where W(p) is the 32-bit window of the key bit stream at bit
// p.  toeplitz_hash (subr.c:482-502) starts its window at key[0..3]
// unconditionally (:489) and shifts in key[i+4] only while i+4 < key_size
// (:496), so stream byte b is key[b] for b < max(4, key_size), else 0.
static void rss_tables(const uint8_t *key, int key_size, uint32_t cnt, uint32_t *T)
{
	const uint64_t kb = key_size > 4 ? (uint64_t)key_size : 4;
	auto kbyte = [&](uint64_t b) -> uint64_t { return b < kb ? key[b] : 0; };
	for (uint32_t i = 0; i < cnt; i++) {
		uint32_t W[8];
		const uint64_t b = i;
		const uint64_t x = kbyte(b) << 32 | kbyte(b + 1) << 24 | kbyte(b + 2) << 16 | kbyte(b + 3) << 8 |
				   kbyte(b + 4);
		for (int s = 0; s < 8; s++)
			W[s] = (uint32_t)(x >> (8 - s));
		for (uint32_t v = 0; v < 256; v++) {
			uint32_t h = 0;
			for (int s = 0; s < 8; s++)
				if (v & (0x80u >> s))
					h ^= W[s];
			T[i * 256 + v] = h;
		}
	}
}

// Streams that launched kernels reading d_rss_tab, each with an event
// recorded after its last such launch: a key change waits for all of them
// before the tables are rewritten (a caller may hash on several streams).
namespace {
struct RssUsers {
	std::vector<std::pair<hipStream_t, hipEvent_t>> ev;
};
} // namespace

int cgck::rss_note_use(cgck_ctx *c, hipStream_t st)
{
	if (!c->rss_users)
		c->rss_users = new RssUsers;
	RssUsers *u = (RssUsers *)c->rss_users;
	hipEvent_t e = nullptr;
	for (auto &x : u->ev)
		if (x.first == st)
			e = x.second;
	if (!e) {
		HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		u->ev.push_back({st, e});
	}
	HIP_TRY(hipEventRecord(e, st));
	return 0;
}

static int rss_wait_users(cgck_ctx *c)
{
	RssUsers *u = (RssUsers *)c->rss_users;
	if (!u)
		return 0;
	// every read of the old tables has finished: the list starts over, so it
	// holds only the streams used since the last key change (an event
	// recorded on a stream the caller has destroyed since still completes)
	while (!u->ev.empty()) {
		HIP_TRY(hipEventSynchronize(u->ev.back().second));
		(void)hipEventDestroy(u->ev.back().second);
		u->ev.pop_back();
	}
	return 0;
}

static void rss_users_free(cgck_ctx *c)
{
	RssUsers *u = (RssUsers *)c->rss_users;
	if (!u)
		return;
	for (auto &x : u->ev)
		(void)hipEventDestroy(x.second);
	delete u;
	c->rss_users = nullptr;
}

// Make d_rss_tab hold the tables of (key, key_size) for `cnt` bytes.  A key
// change first waits for every launch that read the old tables, on any stream.
int cgck::rss_prepare(cgck_ctx *c, const uint8_t *key, int key_size, uint32_t cnt, hipStream_t st)
{
	const int klen = key_size > 4 ? key_size : 4;
	if (c->rss_valid && c->rss_key_len == klen && c->rss_cnt >= cnt && !memcmp(c->rss_key, key, klen))
		return 0;
	const uint32_t tcnt = cnt < 12 ? 12 : cnt; // rss_hash4's 12 bytes are always there
	const size_t tbytes = (size_t)tcnt * 256 * 4;
	int rc;
	if (c->rss_valid && (rc = rss_wait_users(c)))
		return rc;
	c->rss_valid = false;
	if (tbytes > c->h_rss_tab_cap) {
		free(c->h_rss_tab);
		c->h_rss_tab = (uint32_t *)malloc(tbytes);
		c->h_rss_tab_cap = c->h_rss_tab ? tbytes : 0;
		if (!c->h_rss_tab)
			return set_err(-ENOMEM, "rss tables: out of memory");
	}
	if ((rc = grow_dev((void **)&c->d_rss_tab, &c->d_rss_tab_cap, tbytes)))
		return rc;
	uint8_t *nk = (uint8_t *)realloc(c->rss_key, klen);
	if (!nk)
		return set_err(-ENOMEM, "rss key: out of memory");
	c->rss_key = nk;
	memcpy(c->rss_key, key, klen);
	c->rss_key_len = klen;
	rss_tables(key, key_size, tcnt, c->h_rss_tab);
	HIP_TRY(hipMemcpyAsync(c->d_rss_tab, c->h_rss_tab, tbytes, hipMemcpyHostToDevice, st));
	HIP_TRY(CGCK_SYNC(st)); // h_rss_tab is pageable and reused
	c->rss_cnt = tcnt;
	c->rss_valid = true;
	return 0;
}

extern "C" int cgck_toeplitz(cgck_ctx_t *c, const void *data, uint64_t n, uint64_t stride, uint32_t cnt,
			     const unsigned char *key, int key_size, uint32_t mask, uint32_t *out, void *stream)
{
	if (!c)
		return set_err(-EINVAL, "cgck_toeplitz: NULL context");
	if (n && (!data || !out))
		return set_err(-EINVAL, "cgck_toeplitz: NULL data or out");
	if (!key)
		return set_err(-EINVAL, "cgck_toeplitz: NULL key");
	if (cnt > kRssMaxCnt)
		return set_err(-EINVAL, "cgck_toeplitz: cnt %u above %u", cnt, kRssMaxCnt);
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	int rc = rss_prepare(c, key, key_size, cnt, st);
	if (rc)
		return rc;
	RssParams p = {(const uint8_t *)data, n, stride, cnt, mask, c->d_rss_tab, out};
	HIP_TRY(launch_toeplitz(p, c->num_cus, st));
	c->last_kernel = t_kernel;
	return rss_note_use(c, st);
}

// launch_toeplitz's geometry on c's device, from the constants it launches with.
extern "C" int cgck_test_rss_pass(cgck_ctx_t *c, uint64_t *records, uint64_t *groups)
{
	if (!c || !records || !groups)
		return set_err(-EINVAL, "cgck_test_rss_pass: NULL argument");
	*records = (uint64_t)c->num_cus * kRssPassBlocksPerCu * 256;
	*groups = (uint64_t)c->num_cus * kRssX4BlocksPerCu * 256 * kRssX4Depth;
	return 0;
}

// Per-frame hash of a receive burst (cgck_rssf.hip).  The argument rules the
// three entry points share; `what` names the caller in the message.
static int rss_frames_check(const char *what, const cgck_ctx *c, const void *base, const cgck_desc_t *desc,
			    bool by_desc, uint64_t n, const cgck_rss_spec_t *spec, const cgck_rss_res_t *res)
{
	if (!c || !spec || !res || !base)
		return set_err(-EINVAL, "%s: NULL context, spec, res or base", what);
	if (!spec->key)
		return set_err(-EINVAL, "%s: NULL key", what);
	if (by_desc && n && !desc)
		return set_err(-EINVAL, "%s: NULL descriptors", what);
	if (by_desc && ((uintptr_t)desc & 3) != 0)
		return set_err(-EINVAL, "%s: descriptors must be 4-byte aligned", what);
	if (!res->hash && !res->kind && !res->queue && !res->qcount)
		return set_err(-EINVAL, "%s: every output is NULL", what);
	if (spec->hf & ~(uint32_t)(CGCK_RSS_TCP | CGCK_RSS_UDP))
		return set_err(-EINVAL, "%s: unknown hf bits 0x%x", what, spec->hf & ~(uint32_t)(CGCK_RSS_TCP | CGCK_RSS_UDP));
	if (spec->queue_num > 128)
		return set_err(-EINVAL, "%s: queue_num %u above 128 (RSS_QUEUE_ID_MAX)", what, spec->queue_num);
	if (spec->queue_num == 0 && (res->queue || res->qcount))
		return set_err(-EINVAL, "%s: queue or qcount given with queue_num 0", what);
	return 0;
}

// One launch over device-visible frames; the arrays of `res` are device memory.
static int rss_frames_run(cgck_ctx *c, RssfParams p, const cgck_rss_spec_t *spec, const cgck_rss_res_t *res,
			  hipStream_t st)
{
	int rc = rss_prepare(c, spec->key, spec->key_size, kRssLdsMaxCnt, st);
	if (rc)
		return rc;
	p.mask = spec->mask;
	p.hf = spec->hf;
	p.queue_num = spec->queue_num;
	p.tab = c->d_rss_tab;
	p.zero = c->d_zero;
	p.hash = res->hash;
	p.kind = res->kind;
	p.queue = res->queue;
	p.qcount = res->qcount;
	HIP_TRY(launch_rssf(p, c->num_cus, st));
	c->last_kernel = t_kernel;
	return rss_note_use(c, st);
}

extern "C" int cgck_rss_strided(cgck_ctx_t *c, const void *base, uint64_t n, uint64_t stride, uint32_t l3_off,
				uint32_t ip_len, const cgck_rss_spec_t *spec, const cgck_rss_res_t *res, void *stream)
{
	int rc = rss_frames_check("cgck_rss_strided", c, base, nullptr, false, n, spec, res);
	if (rc)
		return rc;
	if (ip_len > 65535)
		return set_err(-EINVAL, "cgck_rss_strided: ip_len %u above 65535 (no jumbograms)", ip_len);
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	RssfParams p = {};
	p.base = (const uint8_t *)base;
	p.n = n;
	p.stride = stride;
	p.l3_off = l3_off;
	p.ip_len = ip_len;
	return rss_frames_run(c, p, spec, res, pick(c, stream));
}

extern "C" int cgck_rss_desc(cgck_ctx_t *c, const void *base, const cgck_desc_t *desc, uint64_t n,
			     const cgck_rss_spec_t *spec, const cgck_rss_res_t *res, void *stream)
{
	int rc = rss_frames_check("cgck_rss_desc", c, base, desc, true, n, spec, res);
	if (rc)
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	RssfParams p = {};
	p.base = (const uint8_t *)base;
	p.desc = desc;
	p.n = n;
	return rss_frames_run(c, p, spec, res, pick(c, stream));
}

// Host-resident burst: registered memory read in place, a pageable range copied
// whole into device scratch; descriptors and outputs through d_aux.  Always a
// launch on the context's stream (the burst server has no such body).
extern "C" int cgck_rss_desc_host(cgck_ctx_t *c, const void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n,
				  const cgck_rss_spec_t *spec, const cgck_rss_res_t *res)
{
	int rc = rss_frames_check("cgck_rss_desc_host", c, base, desc, true, n, spec, res);
	if (rc)
		return rc;
	if ((rc = desc_range_check("cgck_rss_desc_host", desc, n, bytes)))
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const uint8_t *dev_base = nullptr;
	if (bytes) {
		RegRange rr;
		dev_base = reg_find(base, bytes, &rr) ? rr.dev + ((const uint8_t *)base - rr.lo)
						      : (const uint8_t *)registered_ptr(const_cast<void *>(base), bytes);
	}
	if (!dev_base) {
		if ((rc = grow_dev((void **)&c->d_bytes, &c->d_bytes_cap, bytes ? bytes : 16)))
			return rc;
		if (bytes)
			HIP_TRY(hipMemcpyAsync(c->d_bytes, base, bytes, hipMemcpyHostToDevice, st));
		dev_base = c->d_bytes;
	}
	// d_aux: descriptors | hash | qcount | kind | queue
	const uint32_t qn = spec->queue_num;
	const size_t h_off = (12 * n + 15) & ~(size_t)15, c_off = h_off + 4 * n, k_off = c_off + 4 * 128,
		     q_off = k_off + ((n + 15) & ~(size_t)15);
	if ((rc = grow_dev((void **)&c->d_aux, &c->d_aux_cap, q_off + n)))
		return rc;
	if (res->qcount && (rc = grow_host((void **)&c->h_out, &c->h_out_cap, 4 * 128)))
		return rc;
	HIP_TRY(hipMemcpyAsync(c->d_aux, desc, 12 * n, hipMemcpyHostToDevice, st));
	cgck_rss_res_t dres = {};
	dres.hash = res->hash ? (uint32_t *)(c->d_aux + h_off) : nullptr;
	dres.qcount = res->qcount ? (uint32_t *)(c->d_aux + c_off) : nullptr;
	dres.kind = res->kind ? c->d_aux + k_off : nullptr;
	dres.queue = res->queue ? c->d_aux + q_off : nullptr;
	if (dres.qcount)
		HIP_TRY(hipMemsetAsync(dres.qcount, 0, 4 * 128, st));
	RssfParams p = {};
	p.base = dev_base;
	p.desc = c->d_aux;
	p.n = n;
	if ((rc = rss_frames_run(c, p, spec, &dres, st)))
		return rc;
	if (res->hash)
		HIP_TRY(hipMemcpyAsync(res->hash, dres.hash, 4 * n, hipMemcpyDeviceToHost, st));
	if (res->kind)
		HIP_TRY(hipMemcpyAsync(res->kind, dres.kind, n, hipMemcpyDeviceToHost, st));
	if (res->queue)
		HIP_TRY(hipMemcpyAsync(res->queue, dres.queue, n, hipMemcpyDeviceToHost, st));
	if (res->qcount)
		HIP_TRY(hipMemcpyAsync(c->h_out, dres.qcount, 4 * qn, hipMemcpyDeviceToHost, st));
	HIP_TRY(CGCK_SYNC(st));
	for (uint32_t q = 0; res->qcount && q < qn; q++)
		res->qcount[q] += c->h_out[q];
	return 0;
}

// Stable partition by queue id (cgck_steer.hip).  The argument rules cgck_steer
// and cgck_rss_steer_desc share; `what` names the caller in the message.
static int steer_check(const char *what, const cgck_ctx *c, const uint8_t *queue, uint64_t n, uint32_t queue_num,
		       const cgck_desc_t *desc_in, const cgck_steer_res_t *res, const void *work)
{
	if (!c || !queue || !res)
		return set_err(-EINVAL, "%s: NULL context, queue or res", what);
	if (!res->qoff && !res->perm && !res->slot && !res->desc_out)
		return set_err(-EINVAL, "%s: every output is NULL", what);
	if (queue_num == 0 || queue_num > kSteerMaxQueues)
		return set_err(-EINVAL, "%s: queue_num %u outside 1..128 (RSS_QUEUE_ID_MAX)", what, queue_num);
	if (n > 0xFFFFFFFFull)
		return set_err(-EINVAL, "%s: n %llu above 0xFFFFFFFF", what, (unsigned long long)n);
	if (res->desc_out && !desc_in)
		return set_err(-EINVAL, "%s: desc_out given without desc_in", what);
	if (res->desc_out && res->desc_out == desc_in)
		return set_err(-EINVAL, "%s: desc_out must not be desc_in", what);
	if (((uintptr_t)desc_in & 3) != 0 || ((uintptr_t)res->desc_out & 3) != 0)
		return set_err(-EINVAL, "%s: descriptors must be 4-byte aligned", what);
	if (!work && steer_plan(n, queue_num).work_bytes != 0)
		return set_err(-EINVAL, "%s: NULL work for %llu frames (cgck_steer_work_bytes)", what,
			       (unsigned long long)n);
	if (((uintptr_t)work & 3) != 0)
		return set_err(-EINVAL, "%s: work must be 4-byte aligned", what);
	return 0;
}

static int steer_run(cgck_ctx *c, const uint8_t *queue, uint64_t n, uint32_t queue_num, const cgck_desc_t *desc_in,
		     const cgck_steer_res_t *res, void *work, hipStream_t st)
{
	const SteerPlan plan = steer_plan(n, queue_num);
	SteerParams p = {};
	p.queue = queue;
	p.n = n;
	p.queue_num = queue_num;
	p.tile = plan.tile;
	p.tiles = plan.tiles;
	p.desc_in = desc_in;
	p.qoff = res->qoff;
	p.perm = res->perm;
	p.slot = res->slot;
	p.desc_out = res->desc_out;
	p.hist = (uint32_t *)work;
	HIP_TRY(launch_steer(p, st));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_steer(cgck_ctx_t *c, const uint8_t *queue, uint64_t n, uint32_t queue_num,
			  const cgck_desc_t *desc_in, const cgck_steer_res_t *res, void *work, void *stream)
{
	int rc = steer_check("cgck_steer", c, queue, n, queue_num, desc_in, res, work);
	if (rc)
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	return steer_run(c, queue, n, queue_num, desc_in, res, work, pick(c, stream));
}

// cgck_rss_desc, then cgck_steer over the queue ids it wrote, on one stream.
extern "C" int cgck_rss_steer_desc(cgck_ctx_t *c, const void *base, const cgck_desc_t *desc, uint64_t n,
				   const cgck_rss_spec_t *spec, const cgck_rss_res_t *rss, const cgck_steer_res_t *res,
				   void *work, void *stream)
{
	int rc = rss_frames_check("cgck_rss_steer_desc", c, base, desc, true, n, spec, rss);
	if (rc)
		return rc;
	if (!rss->queue)
		return set_err(-EINVAL, "cgck_rss_steer_desc: rss->queue is NULL (the steer's input)");
	if ((rc = steer_check("cgck_rss_steer_desc", c, rss->queue, n, spec->queue_num, desc, res, work)))
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	RssfParams p = {};
	p.base = (const uint8_t *)base;
	p.desc = desc;
	p.n = n;
	if ((rc = rss_frames_run(c, p, spec, rss, st)))
		return rc;
	return steer_run(c, rss->queue, n, spec->queue_num, desc, res, work, st);
}

// Classify and trim a raw Ethernet burst (cgck_l2d.hip): one launch, no scratch.
extern "C" int cgck_l2_desc(cgck_ctx_t *c, const void *base, const cgck_desc_t *raw, uint64_t n,
			    const cgck_l2_res_t *res, void *stream)
{
	if (!c || !res || !base)
		return set_err(-EINVAL, "cgck_l2_desc: NULL context, res or base");
	if (n && !raw)
		return set_err(-EINVAL, "cgck_l2_desc: NULL descriptors");
	if (!res->desc_out && !res->cls && !res->count)
		return set_err(-EINVAL, "cgck_l2_desc: every output is NULL");
	if (((uintptr_t)raw & 3) != 0 || ((uintptr_t)res->desc_out & 3) != 0)
		return set_err(-EINVAL, "cgck_l2_desc: descriptors must be 4-byte aligned");
	if (res->desc_out && res->desc_out == raw)
		return set_err(-EINVAL, "cgck_l2_desc: desc_out must not be raw");
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	L2dParams p = {};
	p.base = (const uint8_t *)base;
	p.raw = raw;
	p.n = n;
	p.zero = c->d_zero;
	p.desc_out = res->desc_out;
	p.cls = res->cls;
	p.count = res->count;
	HIP_TRY(launch_l2d(p, c->num_cus, pick(c, stream)));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_test_l2_pass(cgck_ctx_t *c, uint64_t *frames)
{
	if (!c || !frames)
		return set_err(-EINVAL, "cgck_test_l2_pass: NULL argument");
	*frames = frame_pass_frames(c->num_cus);
	return 0;
}

// Per-frame TCP / UDP segment records (cgck_l4d.hip): one launch, no scratch.
extern "C" int cgck_l4_desc(cgck_ctx_t *c, const void *base, const cgck_desc_t *desc, uint64_t n,
			    const cgck_l4_res_t *res, void *stream)
{
	if (!c || !res || !base)
		return set_err(-EINVAL, "cgck_l4_desc: NULL context, res or base");
	if (n && !desc)
		return set_err(-EINVAL, "cgck_l4_desc: NULL descriptors");
	if (!res->seg && !res->cls && !res->hash && !res->count)
		return set_err(-EINVAL, "cgck_l4_desc: every output is NULL");
	if (((uintptr_t)desc & 3) != 0)
		return set_err(-EINVAL, "cgck_l4_desc: descriptors must be 4-byte aligned");
	if (((uintptr_t)res->seg & 15) != 0)
		return set_err(-EINVAL, "cgck_l4_desc: seg must be 16-byte aligned");
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	L4dParams p = {};
	p.base = (const uint8_t *)base;
	p.desc = desc;
	p.n = n;
	p.zero = c->d_zero;
	p.seg = res->seg;
	p.cls = res->cls;
	p.hash = res->hash;
	p.count = res->count;
	HIP_TRY(launch_l4d(p, c->num_cus, pick(c, stream)));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_test_l4_pass(cgck_ctx_t *c, uint64_t *frames)
{
	if (!c || !frames)
		return set_err(-EINVAL, "cgck_test_l4_pass: NULL argument");
	*frames = frame_pass_frames(c->num_cus);
	return 0;
}

// Frames from segment records (cgck_l4b.hip): one launch, no scratch.  The store
// shape is the product's (kL4bTurned) unless cgck_test_l4_build_store pinned one.
static constexpr bool kL4bTurned = false; // the A/B of DESIGN.md §5.14: turned is no faster
static std::atomic<int> g_l4b_store{0};

extern "C" int cgck_l4_build(cgck_ctx_t *c, void *base, uint64_t n, const cgck_l4_build_in_t *in,
			     const cgck_l4_build_res_t *res, void *stream)
{
	static const cgck_l4_build_res_t none = {};
	if (!c || !base || !in)
		return set_err(-EINVAL, "cgck_l4_build: NULL context, base or in");
	if (!res)
		res = &none;
	if (n && (!in->slot || !in->seg || !in->flow))
		return set_err(-EINVAL, "cgck_l4_build: NULL slot, seg or flow");
	if (((uintptr_t)in->slot & 3) != 0 || ((uintptr_t)res->raw_out & 3) != 0 || ((uintptr_t)res->desc_out & 3) != 0)
		return set_err(-EINVAL, "cgck_l4_build: descriptors must be 4-byte aligned");
	if (((uintptr_t)in->seg & 15) != 0 || ((uintptr_t)in->flow & 15) != 0)
		return set_err(-EINVAL, "cgck_l4_build: seg and flow must be 16-byte aligned");
	if ((res->raw_out && res->raw_out == in->slot) || (res->desc_out && res->desc_out == in->slot) ||
	    (res->raw_out && res->raw_out == res->desc_out))
		return set_err(-EINVAL, "cgck_l4_build: raw_out and desc_out must be neither slot nor each other");
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	L4bParams p = {};
	p.base = (uint8_t *)base;
	p.slot = in->slot;
	p.seg = in->seg;
	p.cls = in->cls;
	p.flow = in->flow;
	p.fidx = in->fidx;
	p.n = n;
	p.nflow = in->nflow;
	p.ip_id0 = in->ip_id0;
	p.ip_off = in->ip_off;
	p.raw_out = res->raw_out;
	p.desc_out = res->desc_out;
	p.cls_out = res->cls;
	p.count = res->count;
	const int shape = g_l4b_store.load(std::memory_order_relaxed);
	HIP_TRY(launch_l4b(p, shape == 0 ? kL4bTurned : shape == 2, c->num_cus, pick(c, stream)));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" uint32_t cgck_l4_build_hdr_bytes(uint8_t flow_flags, uint8_t cls, uint8_t opt)
{
	const uint32_t l = l4b_lengths(flow_flags, cls, opt);
	return (l & 255u) + ((l >> 8) & 255u) + (l >> 16);
}

extern "C" int cgck_test_l4_build_store(int shape)
{
	if (shape < 0 || shape > 2)
		return set_err(-EINVAL, "cgck_test_l4_build_store: shape must be 0 (the product's), 1 (direct) or 2 (turned)");
	return g_l4b_store.exchange(shape, std::memory_order_relaxed);
}

extern "C" int cgck_test_l4_build_pass(cgck_ctx_t *c, uint64_t *frames)
{
	if (!c || !frames)
		return set_err(-EINVAL, "cgck_test_l4_build_pass: NULL argument");
	*frames = frame_pass_frames(c->num_cus);
	return 0;
}

// Per-frame connection lookup (cgck_pcb.hip): a memset and one launch for the build,
// one launch for the lookup, no scratch.  The table shape is the product's
// (kPcbTagged) unless cgck_test_pcb_mode's bit 1 asks for the other.
static constexpr bool kPcbTagged = true; // the A/B of DESIGN.md §5.15
static std::atomic<int> g_pcb_mode{0};

// The checks the two calls share; nullptr when pcb passes.
static const char *pcb_refused(const cgck_pcb_t *pcb)
{
	if (((uintptr_t)pcb->conn & 3) != 0 || ((uintptr_t)pcb->bound & 3) != 0)
		return "conn and bound must be 4-byte aligned";
	if (((uintptr_t)pcb->flow & 15) != 0 || ((uintptr_t)pcb->table & 15) != 0)
		return "flow and table must be 16-byte aligned";
	if (pcb->nconn > kPcbMaxConn)
		return "nconn above 1 << 30";
	if (pcb->nconn && !pcb->conn)
		return "NULL conn";
	if (pcb->nflow && !pcb->flow)
		return "NULL flow";
	if (!pcb->table)
		return "NULL table";
	if (pcb->table_bytes < cgck_pcb_table_bytes(pcb->nconn))
		return "table_bytes below cgck_pcb_table_bytes(nconn)";
	return nullptr;
}

static PcbTable pcb_table(const cgck_pcb_t *pcb, int mode)
{
	PcbTable t = {};
	t.conn = pcb->conn;
	t.flow = pcb->flow;
	t.table = pcb->table;
	t.nconn = pcb->nconn;
	t.nflow = pcb->nflow;
	t.mask = pcb_slots(pcb->nconn) - 1;
	t.chain = mode & 1;
	return t;
}

extern "C" int cgck_pcb_build(cgck_ctx_t *c, const cgck_pcb_t *pcb, uint32_t *stat, void *stream)
{
	if (!c || !pcb)
		return set_err(-EINVAL, "cgck_pcb_build: NULL context or pcb");
	if (const char *why = pcb_refused(pcb))
		return set_err(-EINVAL, "cgck_pcb_build: %s", why);
	if (((uintptr_t)stat & 3) != 0)
		return set_err(-EINVAL, "cgck_pcb_build: stat must be 4-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	const int mode = g_pcb_mode.load(std::memory_order_relaxed);
	PcbbParams p = {};
	p.t = pcb_table(pcb, mode);
	p.stat = stat;
	HIP_TRY(launch_pcbb(p, (mode & 2) ? false : kPcbTagged, pick(c, stream)));
	if (pcb->nconn)
		c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_pcb_lookup(cgck_ctx_t *c, const void *base, const cgck_desc_t *desc, const cgck_seg_t *seg,
			       const uint8_t *cls, uint64_t n, const cgck_pcb_t *pcb, const cgck_pcb_res_t *res,
			       void *stream)
{
	if (!c || !pcb || !res || !base)
		return set_err(-EINVAL, "cgck_pcb_lookup: NULL context, pcb, res or base");
	if (n && (!desc || !seg))
		return set_err(-EINVAL, "cgck_pcb_lookup: NULL descriptors or seg");
	if (!res->idx && !res->fidx && !res->kind && !res->count)
		return set_err(-EINVAL, "cgck_pcb_lookup: every output is NULL");
	if (((uintptr_t)desc & 3) != 0 || ((uintptr_t)res->idx & 3) != 0 || ((uintptr_t)res->fidx & 3) != 0 ||
	    ((uintptr_t)res->count & 3) != 0)
		return set_err(-EINVAL, "cgck_pcb_lookup: desc, idx, fidx and count must be 4-byte aligned");
	if (((uintptr_t)seg & 15) != 0)
		return set_err(-EINVAL, "cgck_pcb_lookup: seg must be 16-byte aligned");
	if (const char *why = pcb_refused(pcb))
		return set_err(-EINVAL, "cgck_pcb_lookup: %s", why);
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	const int mode = g_pcb_mode.load(std::memory_order_relaxed);
	PcblParams p = {};
	p.base = (const uint8_t *)base;
	p.desc = desc;
	p.seg = seg;
	p.cls = cls;
	p.n = n;
	p.zero = c->d_zero;
	p.t = pcb_table(pcb, mode);
	p.bound = pcb->bound;
	p.idx = res->idx;
	p.fidx = res->fidx;
	p.kind = res->kind;
	p.count = res->count;
	HIP_TRY(launch_pcbl(p, (mode & 2) ? false : kPcbTagged, c->num_cus, pick(c, stream)));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_test_pcb_pass(cgck_ctx_t *c, uint64_t *frames)
{
	if (!c || !frames)
		return set_err(-EINVAL, "cgck_test_pcb_pass: NULL argument");
	*frames = frame_pass_frames(c->num_cus);
	return 0;
}

extern "C" int cgck_test_pcb_mode(int mode)
{
	if (mode < 0 || mode > 3)
		return set_err(-EINVAL, "cgck_test_pcb_mode: mode must be within 0..3");
	return g_pcb_mode.exchange(mode, std::memory_order_relaxed);
}

// tcp_respond's RSTs for a burst (cgck_l4r.hip): one launch, no scratch.  Under
// `at` the store shape is the product's (kL4rTurned) unless cgck_test_l4_reply_store
// pinned one.
static constexpr bool kL4rTurned = false; // the A/B of DESIGN.md §5.16
static std::atomic<int> g_l4r_store{0};

// The argument rules cgck_l4_reply and cgck_l4_reply_packed share; `what` names the
// caller in the message.
static int l4r_check(const char *what, const cgck_ctx *c, const void *base, uint64_t n, const cgck_l4_reply_in_t *in,
		     const cgck_l4_reply_res_t *res)
{
	if (!c || !base || !in || !res)
		return set_err(-EINVAL, "%s: NULL context, base, in or res", what);
	if (n && (!in->desc || !in->seg))
		return set_err(-EINVAL, "%s: NULL descriptors or seg", what);
	if (!res->seg && !res->flow && !res->cls && !res->queue && !res->count)
		return set_err(-EINVAL, "%s: every output is NULL", what);
	if (((uintptr_t)in->desc & 3) != 0 || ((uintptr_t)in->at & 3) != 0 || ((uintptr_t)res->count & 3) != 0)
		return set_err(-EINVAL, "%s: desc, at and count must be 4-byte aligned", what);
	if (((uintptr_t)in->seg & 15) != 0 || ((uintptr_t)res->seg & 15) != 0 || ((uintptr_t)res->flow & 15) != 0)
		return set_err(-EINVAL, "%s: seg and flow must be 16-byte aligned", what);
	if (in->link.flags & ~kRplLinkBits)
		return set_err(-EINVAL, "%s: link.flags 0x%02x has a bit outside CGCK_FLOW_IP6 | CGCK_FLOW_VLAN", what,
			       in->link.flags);
	if (in->flags & ~kRplFlags)
		return set_err(-EINVAL, "%s: flags 0x%x has an unknown bit", what, in->flags);
	if (res->seg && res->seg == in->seg)
		return set_err(-EINVAL, "%s: the output seg must not be the input seg", what);
	return 0;
}

static int l4r_run(cgck_ctx *c, const void *base, uint64_t n, const cgck_l4_reply_in_t *in, const uint32_t *at,
		   const cgck_l4_reply_res_t *res, hipStream_t st)
{
	L4rParams p = {};
	p.base = (const uint8_t *)base;
	p.desc = in->desc;
	p.seg = in->seg;
	p.cls = in->cls;
	p.kind = in->kind;
	p.verdict = in->verdict;
	p.l2cls = in->l2cls;
	p.at = at;
	p.n = n;
	p.zero = c->d_zero;
	memcpy(p.link, &in->link, sizeof(p.link));
	p.vmask = in->vmask;
	p.flags = in->flags;
	p.seg_out = res->seg;
	p.flow_out = res->flow;
	p.cls_out = res->cls;
	p.queue = res->queue;
	p.count = res->count;
	const int shape = g_l4r_store.load(std::memory_order_relaxed);
	HIP_TRY(launch_l4r(p, shape == 0 ? kL4rTurned : shape == 2, c->num_cus, st));
	c->last_kernel = t_kernel;
	return 0;
}

extern "C" int cgck_l4_reply(cgck_ctx_t *c, const void *base, uint64_t n, const cgck_l4_reply_in_t *in,
			     const cgck_l4_reply_res_t *res, void *stream)
{
	int rc = l4r_check("cgck_l4_reply", c, base, n, in, res);
	if (rc)
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	return l4r_run(c, base, n, in, in->at, res, pick(c, stream));
}

// cgck_l4_reply for the queue bytes, cgck_steer with one queue over them, then
// cgck_l4_reply at the slots the steer gave, on one stream.
extern "C" int cgck_l4_reply_packed(cgck_ctx_t *c, const void *base, uint64_t n, const cgck_l4_reply_in_t *in,
				    const cgck_l4_reply_res_t *res, const cgck_l4_reply_pack_t *pk, void *stream)
{
	int rc = l4r_check("cgck_l4_reply_packed", c, base, n, in, res);
	if (rc)
		return rc;
	if (!pk || !pk->queue || !pk->at || !pk->qoff)
		return set_err(-EINVAL, "cgck_l4_reply_packed: NULL pk, queue, at or qoff");
	if (in->at)
		return set_err(-EINVAL, "cgck_l4_reply_packed: in->at must be NULL (the call computes it into pk->at)");
	if (((uintptr_t)pk->at & 3) != 0 || ((uintptr_t)pk->qoff & 3) != 0)
		return set_err(-EINVAL, "cgck_l4_reply_packed: at and qoff must be 4-byte aligned");
	cgck_steer_res_t sres = {};
	sres.qoff = pk->qoff;
	sres.slot = pk->at;
	if ((rc = steer_check("cgck_l4_reply_packed", c, pk->queue, n, 1, nullptr, &sres, pk->work)))
		return rc;
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	cgck_l4_reply_res_t first = {};
	first.queue = pk->queue;
	if ((rc = l4r_run(c, base, n, in, nullptr, &first, st)))
		return rc;
	if ((rc = steer_run(c, pk->queue, n, 1, nullptr, &sres, pk->work, st)))
		return rc;
	return l4r_run(c, base, n, in, pk->at, res, st);
}

extern "C" int cgck_test_l4_reply_pass(cgck_ctx_t *c, uint64_t *frames)
{
	if (!c || !frames)
		return set_err(-EINVAL, "cgck_test_l4_reply_pass: NULL argument");
	*frames = frame_pass_frames(c->num_cus);
	return 0;
}

extern "C" int cgck_test_l4_reply_store(int shape)
{
	if (shape < 0 || shape > 2)
		return set_err(-EINVAL, "cgck_test_l4_reply_store: shape must be 0 (the product's), 1 (own lanes) or 2 (turned)");
	return g_l4r_store.exchange(shape, std::memory_order_relaxed);
}

extern "C" int cgck_dst_cache(cgck_ctx_t *c, const cgck_dst_params_t *prm, cgck_dst_entry_t *out, uint32_t cap,
			      uint32_t *count, void *stream)
{
	if (!c || !prm || !out || !count)
		return set_err(-EINVAL, "cgck_dst_cache: NULL argument");
	if (cap == 0 || cap > 0x7fffffffu)
		return set_err(-EINVAL, "cgck_dst_cache: cap must be in 1..INT_MAX (t_dst_cache_size)");
	const bool filter = prm->rss_queue_id < 128 && prm->rss_queue_num > 1; // con-gen.c:337
	if (filter && !prm->rss_key)
		return set_err(-EINVAL, "cgck_dst_cache: RSS filter on but rss_key is NULL");
	// scan_ip_range (con-gen.c:131-133) never yields min > max.
	if (prm->laddr_min > prm->laddr_max || prm->faddr_min > prm->faddr_max)
		return set_err(-EINVAL, "cgck_dst_cache: address range with min > max");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	// con-gen.c:314-315: the product is formed in 32-bit unsigned arithmetic.
	const uint32_t nl = prm->laddr_max - prm->laddr_min + 1u;
	const uint32_t nf = prm->faddr_max - prm->faddr_min + 1u;
	const uint32_t n = nl * nf * (uint32_t)(65535 - 5000 + 1);
	if (n == 0) {
		HIP_TRY(hipMemsetAsync(count, 0, 4, st));
		return 0;
	}
	int rc;
	DstParams p = {};
	p.laddr_min = prm->laddr_min;
	p.faddr_min = prm->faddr_min;
	p.nf = nf;
	p.n = n;
	p.q64 = 64 / nf;
	p.r64 = 64 % nf;
	p.fport_be = prm->fport;
	p.filter = filter;
	p.cap = cap;
	if (filter) {
		if ((rc = rss_prepare(c, prm->rss_key, prm->rss_key_size, 12, st)))
			return rc;
		// rss_hash4 stores fport as given (subr.c:519): bytes 8, 9 of the data.
		p.hconst = c->h_rss_tab[8 * 256 + (prm->fport & 255u)] ^ c->h_rss_tab[9 * 256 + (prm->fport >> 8)];
		for (uint32_t h = 0; h < 128; h++)
			if (h % prm->rss_queue_num == prm->rss_queue_id)
				(h < 64 ? p.pass_lo : p.pass_hi) |= 1ull << (h & 63);
		p.tab = c->d_rss_tab;
	}
	p.iters = dst_iters(n, cap, filter, p.pass_lo, p.pass_hi, c->num_cus);
	const uint64_t tile = 256ull * p.iters;
	p.ntiles = (uint32_t)(((uint64_t)n + tile - 1) / tile);
	const size_t sbytes = 16 + (size_t)p.ntiles * 8;
	if ((rc = grow_dev((void **)&c->d_dst, &c->d_dst_cap, sbytes)))
		return rc;
	p.out = out;
	p.ctl = (uint32_t *)c->d_dst;
	p.count = count;
	p.status = (uint64_t *)(c->d_dst + 16);
	HIP_TRY(hipMemsetAsync(c->d_dst, 0, sbytes, st));
	HIP_TRY(launch_dst_cache(p, c->num_cus, st));
	c->last_kernel = t_kernel;
	return filter ? rss_note_use(c, st) : 0;
}

extern "C" int cgck_dst_cache_host(cgck_ctx_t *c, const cgck_dst_params_t *prm, cgck_dst_entry_t *out,
				   uint32_t cap, uint32_t *count)
{
	if (!c || !prm || !out || !count)
		return set_err(-EINVAL, "cgck_dst_cache_host: NULL argument");
	if (cap == 0 || cap > 0x7fffffffu)
		return set_err(-EINVAL, "cgck_dst_cache_host: cap must be in 1..INT_MAX (t_dst_cache_size)");
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	const size_t obytes = (size_t)cap * sizeof(cgck_dst_entry_t);
	if ((rc = grow_dev((void **)&c->d_bytes, &c->d_bytes_cap, obytes + 64)))
		return rc;
	if ((rc = grow_host((void **)&c->h_out, &c->h_out_cap, 64)))
		return rc;
	uint32_t *d_count = (uint32_t *)(c->d_bytes + obytes);
	if ((rc = cgck_dst_cache(c, prm, (cgck_dst_entry_t *)c->d_bytes, cap, d_count, c->stream)))
		return rc;
	// count, then the control words (timeout flag) when the launch ran
	HIP_TRY(hipMemcpyAsync(c->h_out, d_count, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(c->h_out + 1, c->d_dst, 16, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(CGCK_SYNC(c->stream));
	if (c->h_out[1 + 2])
		return set_err(-ETIMEDOUT, "cgck_dst_cache: look-back spin limit reached");
	const uint32_t got = c->h_out[0];
	if (got > cap)
		return set_err(-EIO, "cgck_dst_cache: count %u above cap %u", got, cap);
	if (got)
		HIP_TRY(hipMemcpy(out, c->d_bytes, (size_t)got * sizeof(cgck_dst_entry_t), hipMemcpyDeviceToHost));
	*count = got;
	return 0;
}

// --------------------------------------------------------------------------
// Synthetic batches
// --------------------------------------------------------------------------

extern "C" uint64_t cgck_imix_bytes(uint64_t n)
{
	static const uint16_t cum[13] = {0, 64, 640, 704, 768, 1344, 1408, 2908, 2972, 3548, 3612, 3676, 4252};
	return (n / 12) * (uint64_t)kImixCycleBytes + cum[n % 12];
}

extern "C" int cgck_synth_strided(cgck_ctx_t *c, void *base, uint64_t n, uint64_t stride, uint32_t ip_len,
				  uint64_t seed, void *stream)
{
	if (!c || (n && !base))
		return set_err(-EINVAL, "cgck_synth_strided: bad arguments");
	if (ip_len < 20 || ip_len > stride)
		return set_err(-EINVAL, "cgck_synth_strided: need 20 <= ip_len <= stride");
	if ((uintptr_t)base & 15)
		return set_err(-EINVAL, "cgck_synth_strided: base must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, n * stride, seed, c->num_cus, st));
	HIP_TRY(launch_synth_stamp((uint8_t *)base, n, stride, ip_len, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_strided_ip6(cgck_ctx_t *c, void *base, uint64_t n, uint64_t stride, uint32_t ip_len,
				      uint32_t nh, uint64_t seed, void *stream)
{
	if (!c || (n && !base))
		return set_err(-EINVAL, "cgck_synth_strided_ip6: bad arguments");
	if (ip_len < 40 || ip_len > stride || ip_len > 65535 || nh > 255)
		return set_err(-EINVAL, "cgck_synth_strided_ip6: need 40 <= ip_len <= min(stride, 65535), nh <= 255");
	if ((uintptr_t)base & 15)
		return set_err(-EINVAL, "cgck_synth_strided_ip6: base must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, n * stride, seed, c->num_cus, st));
	HIP_TRY(launch_synth_stamp6((uint8_t *)base, n, stride, ip_len, nh, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_imix(cgck_ctx_t *c, void *base, cgck_desc_t *desc, uint64_t n, uint64_t seed,
			       void *stream)
{
	if (!c || (n && (!base || !desc)))
		return set_err(-EINVAL, "cgck_synth_imix: bad arguments");
	if (((uintptr_t)base & 15) || ((uintptr_t)desc & 3))
		return set_err(-EINVAL, "cgck_synth_imix: misaligned buffers");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, cgck_imix_bytes(n), seed, c->num_cus, st));
	HIP_TRY(launch_synth_imix((uint8_t *)base, (uint32_t *)desc, n, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_imix_ring(cgck_ctx_t *c, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
				    uint32_t l3_off, uint64_t seed, void *stream)
{
	if (!c || (n && (!base || !desc)))
		return set_err(-EINVAL, "cgck_synth_imix_ring: bad arguments");
	if (((uintptr_t)base & 15) || ((uintptr_t)desc & 3))
		return set_err(-EINVAL, "cgck_synth_imix_ring: misaligned buffers");
	if (l3_off > 0xffff || stride < (uint64_t)l3_off + 1500)
		return set_err(-EINVAL, "cgck_synth_imix_ring: a slot must hold l3_off + 1500 bytes");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, n * stride, seed, c->num_cus, st));
	HIP_TRY(launch_synth_ring((uint8_t *)base, (uint32_t *)desc, n, stride, l3_off, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_imix_ip6(cgck_ctx_t *c, void *base, cgck_desc_t *desc, uint64_t n, uint32_t nh,
				   uint64_t seed, void *stream)
{
	if (!c || (n && (!base || !desc)))
		return set_err(-EINVAL, "cgck_synth_imix_ip6: bad arguments");
	if (((uintptr_t)base & 15) || ((uintptr_t)desc & 3))
		return set_err(-EINVAL, "cgck_synth_imix_ip6: misaligned buffers");
	if (nh > 255)
		return set_err(-EINVAL, "cgck_synth_imix_ip6: need nh <= 255");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, cgck_imix_bytes(n), seed, c->num_cus, st));
	HIP_TRY(launch_synth_imix6((uint8_t *)base, (uint32_t *)desc, n, 0, 0, nh, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_imix_ring_ip6(cgck_ctx_t *c, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
					uint32_t l3_off, uint32_t nh, uint64_t seed, void *stream)
{
	if (!c || (n && (!base || !desc)))
		return set_err(-EINVAL, "cgck_synth_imix_ring_ip6: bad arguments");
	if (((uintptr_t)base & 15) || ((uintptr_t)desc & 3))
		return set_err(-EINVAL, "cgck_synth_imix_ring_ip6: misaligned buffers");
	if (l3_off > 0xffff || stride < (uint64_t)l3_off + 1500)
		return set_err(-EINVAL, "cgck_synth_imix_ring_ip6: a slot must hold l3_off + 1500 bytes");
	if (nh > 255)
		return set_err(-EINVAL, "cgck_synth_imix_ring_ip6: need nh <= 255");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, n * stride, seed, c->num_cus, st));
	HIP_TRY(launch_synth_imix6((uint8_t *)base, (uint32_t *)desc, n, stride, l3_off, nh, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_imix_dual(cgck_ctx_t *c, void *base, cgck_desc_t *desc, uint64_t n, uint64_t stride,
				    uint32_t l3_off, uint64_t seed, void *stream)
{
	if (!c || (n && (!base || !desc)))
		return set_err(-EINVAL, "cgck_synth_imix_dual: bad arguments");
	if (((uintptr_t)base & 15) || ((uintptr_t)desc & 3))
		return set_err(-EINVAL, "cgck_synth_imix_dual: misaligned buffers");
	if (stride ? (l3_off > 0xffff || stride < (uint64_t)l3_off + 1500) : l3_off != 0)
		return set_err(-EINVAL, "cgck_synth_imix_dual: a slot must hold l3_off + 1500 bytes (stride 0: the packed "
					"set, l3_off 0)");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	HIP_TRY(launch_synth_fill((uint8_t *)base, stride ? n * stride : cgck_imix_bytes(n), seed, c->num_cus, st));
	HIP_TRY(launch_synth_dual((uint8_t *)base, (uint32_t *)desc, n, stride, l3_off, c->num_cus, st));
	return 0;
}

extern "C" int cgck_synth_eth(cgck_ctx_t *c, void *base, const cgck_desc_t *desc, cgck_desc_t *raw, uint64_t n,
			      uint32_t vlan_every, uint64_t seed, void *stream)
{
	if (!c || (n && (!base || !desc || !raw)))
		return set_err(-EINVAL, "cgck_synth_eth: bad arguments");
	if (((uintptr_t)desc & 3) || ((uintptr_t)raw & 3))
		return set_err(-EINVAL, "cgck_synth_eth: misaligned descriptors");
	if (n == 0)
		return 0;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = pick(c, stream);
	// no frame is written before every l3_off is known to leave room
	int rc = grow_dev((void **)&c->d_dst, &c->d_dst_cap, 16);
	if (rc)
		return rc;
	uint32_t flag = 0;
	HIP_TRY(hipMemsetAsync(c->d_dst, 0, 4, st));
	HIP_TRY(launch_synth_eth_check((const uint32_t *)desc, n, (uint32_t *)c->d_dst, c->num_cus, st));
	HIP_TRY(hipMemcpyAsync(&flag, c->d_dst, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(CGCK_SYNC(st));
	if (flag)
		return set_err(-EINVAL, "cgck_synth_eth: an l3_off below 18 leaves no room for the header and a tag");
	HIP_TRY(launch_synth_eth((uint8_t *)base, (const uint32_t *)desc, (uint32_t *)raw, n, vlan_every, seed, c->num_cus,
				 st));
	return 0;
}

extern "C" int cgck_probe_read(cgck_ctx_t *c, const void *src, uint64_t bytes, uint32_t *sink, void *stream)
{
	if (!c || !src || !sink || ((uintptr_t)src & 15))
		return set_err(-EINVAL, "cgck_probe_read: bad arguments");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(launch_probe_read(src, bytes, sink, c->num_cus, c->family, pick(c, stream)));
	return 0;
}

// --------------------------------------------------------------------------
// Plumbing
// --------------------------------------------------------------------------

extern "C" int cgck_dev_alloc(size_t bytes, void **ptr)
{
	if (!ptr)
		return set_err(-EINVAL, "cgck_dev_alloc: NULL out");
	*ptr = nullptr;
	if (cgck_device_count() <= 0)
		return set_err(-ENODEV, "cgck: no HIP device visible");
	// Plain hipMalloc.  Physically contiguous allocations
	// (hipDeviceMallocContiguous) were measured as a cure for the 64 B
	// fast/slow state: every contiguous 1 GiB input of a
	// probe read fast, but whole bench runs moved by -1.1..+2.7 points from
	// box to box (profiles/r01/alloc_ab.log), so they stay an A/B option:
	// $CGCK_DEV_ALLOC_FLAGS sets hipExtMallocWithFlags flags for requests up to
	// $CGCK_DEV_ALLOC_CONTIG_MAX bytes (default 8 GiB).
	static const unsigned cflags = [] {
		const char *e = CGCK_ENV("CGCK_DEV_ALLOC_FLAGS");
		return e ? (unsigned)strtoul(e, nullptr, 0) : 0u;
	}();
	static const size_t cmax = [] {
		const char *e = CGCK_ENV("CGCK_DEV_ALLOC_CONTIG_MAX");
		return e ? (size_t)strtoull(e, nullptr, 0) : (size_t)8 << 30;
	}();
	const unsigned aflags = bytes <= cmax ? cflags : 0u;
	if (aflags) {
		const hipError_t e = hipExtMallocWithFlags(ptr, bytes ? bytes : 1, aflags);
		if (e == hipSuccess)
			return 0;
		(void)hipGetLastError();
		if (CGCK_ENV("CGCK_ALLOC_VERBOSE"))
			fprintf(stderr, "cgck_dev_alloc: flags %#x for %zu bytes failed (%s), plain hipMalloc\n",
				aflags, bytes, hipGetErrorString(e));
	}
	*ptr = nullptr;
	HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1));
	return 0;
}

extern "C" int cgck_dev_free(void *ptr)
{
	if (ptr)
		free_or_park(ptr, false);
	return 0;
}

extern "C" int cgck_host_alloc(size_t bytes, void **ptr)
{
	if (!ptr)
		return set_err(-EINVAL, "cgck_host_alloc: NULL out");
	*ptr = nullptr;
	HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
	return 0;
}

extern "C" int cgck_host_free(void *ptr)
{
	if (ptr)
		free_or_park(ptr, true);
	return 0;
}

extern "C" int cgck_memcpy(void *dst, const void *src, size_t bytes, void *stream)
{
	HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
	return 0;
}

extern "C" int cgck_memset(void *dst, int value, size_t bytes, void *stream)
{
	HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
	return 0;
}

extern "C" int cgck_event_create(cgck_event_t **ev)
{
	if (!ev)
		return set_err(-EINVAL, "cgck_event_create: NULL out");
	cgck_event *e = (cgck_event *)calloc(1, sizeof(*e));
	if (!e)
		return set_err(-ENOMEM, "cgck_event_create: out of memory");
	hipError_t h = hipEventCreate(&e->ev);
	if (h != hipSuccess) {
		free(e);
		return set_err(-EIO, "hipEventCreate: %s", hipGetErrorString(h));
	}
	*ev = e;
	return 0;
}

extern "C" int cgck_event_destroy(cgck_event_t *ev)
{
	if (ev) {
		(void)hipEventDestroy(ev->ev);
		free(ev);
	}
	return 0;
}

extern "C" int cgck_event_record(cgck_ctx_t *c, cgck_event_t *ev, void *stream)
{
	if (!c || !ev)
		return set_err(-EINVAL, "cgck_event_record: bad arguments");
	HIP_TRY(hipEventRecord(ev->ev, pick(c, stream)));
	return 0;
}

extern "C" int cgck_event_elapsed_ms(cgck_event_t *a, cgck_event_t *b, float *ms)
{
	if (!a || !b || !ms)
		return set_err(-EINVAL, "cgck_event_elapsed_ms: bad arguments");
	HIP_TRY(hipEventSynchronize(b->ev));
	HIP_TRY(hipEventElapsedTime(ms, a->ev, b->ev));
	return 0;
}
