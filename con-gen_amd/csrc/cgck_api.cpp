// cgck_api.cpp — host side of libcgck.so: the C-ABI declared in
// include/cgck.h.  Contexts (stream + staging), device-resident and
// host-resident batches, registered rings, the burst server, the Toeplitz
// RSS batch and dst-cache entry points, synthetic generation and timing.
// The drop-in symbols and the per-thread RX / TX windows are in
// cgck_dropin.cpp.
//
// Every checksum this library returns is computed by the gfx950 kernels
// (cgck_group.hip, cgck_lane.hip); there is no host arithmetic path.  Without
// a usable device every entry point fails with -ENODEV.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <atomic>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "cgck_host.h"
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

// hipFree / hipHostFree synchronise the device: with a burst server resident
// on it (a persistent kernel) such a free waits until every server idles out
// — 200 ms of a worker's loop (a coalesced loop whose fills outgrew the
// staging: tools/txloop, profiles/r06/stall/), or forever while other
// workers keep theirs busy.  So while any server is resident a buffer is not
// freed but parked, and parked buffers are freed once the last server has
// closed (burst_close).
static void free_or_park(void *p, bool host);

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
	if (c->bbox)
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
// Burst server (cgck_group.hip): small host-resident batches without a launch
// or a stream synchronisation each
// --------------------------------------------------------------------------

static double now_s()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec + ts.tv_nsec * 1e-9;
}

#if CGCK_LAB
hipError_t cgck::lab_sync(const char *where, hipStream_t st)
{
	const double t0 = now_s();
	const hipError_t e = hipStreamSynchronize(st);
	if (now_s() - t0 > 0.02)
		fprintf(stderr, "cgck lab: hipStreamSynchronize at %s took %.1f ms\n", where, (now_s() - t0) * 1e3);
	return e;
}
#endif

// (Re)launch the server's K workgroups; the first request each serves is
// the one after start_seq.
#if CGCK_LAB
static thread_local uint64_t t_lab_host[2]; // cgck_lab_burst_times
thread_local double t_lab_post[16];         // cgck_lab_post_times (cgck_dropin.cpp), TSC ticks
#define LAB_TICK(i, t0) (t_lab_post[2 * (i)] += (double)(__builtin_ia32_rdtsc() - (t0)), t_lab_post[2 * (i) + 1] += 1)
#endif

// Lab A/B bits of the server kernel ($CGCK_SERVER_OPTS; 0 in the product).
static uint32_t server_opts()
{
	static const uint32_t v = [] {
		const char *e = CGCK_ENV("CGCK_SERVER_OPTS");
		return e && *e ? (uint32_t)strtoul(e, nullptr, 0) : 0u;
	}();
	return v;
}

// Server launches in this process: a relay word left by one launch (in
// device memory a later server may get again) never matches another's tag.
static std::atomic<uint32_t> g_burst_epoch{0};

// No server kernel runs while a host mapping changes.  cgck_host_register /
// _unregister (and burst open / close) take g_map_wr, raise g_map_changing,
// wait until no context with a server is inside a request (its bbusy word),
// and drain every open server (the next request relaunches it).  A request
// (post, wait, relaunch) runs inside a MapGuard on its own context: it sets
// the context's bbusy and then checks g_map_changing (both sequentially
// consistent, so either the writer sees the context busy or the request sees
// the change and steps back until it is over).  The request path thus writes
// only its own context's line and reads a line no request writes: no
// process-wide lock or shared read-modify-write per request (32 workers each
// posting bursts do not bounce a lock line).  g_srv lists the
// contexts with an open server (changed under g_map_wr).
namespace {
std::mutex g_map_wr;
std::mutex g_park_mu;
std::vector<std::pair<void *, bool>> g_parked; // (buffer, host)
std::atomic<uint32_t> g_map_changing{0};
std::mutex g_srv_mu;
std::vector<cgck_ctx *> g_srv;

class MapGuard {
      public:
	explicit MapGuard(cgck_ctx *c) : c_(c)
	{
		for (;;) {
			__atomic_store_n(&c_->bbusy, 1u, __ATOMIC_SEQ_CST);
			if (!g_map_changing.load(std::memory_order_seq_cst))
				return;
			__atomic_store_n(&c_->bbusy, 0u, __ATOMIC_RELEASE);
			for (uint32_t k = 0; g_map_changing.load(std::memory_order_acquire); k++) {
				if (k < 4096)
					__builtin_ia32_pause();
				else
					sched_yield();
			}
		}
	}
	~MapGuard() { __atomic_store_n(&c_->bbusy, 0u, __ATOMIC_RELEASE); }
	MapGuard(const MapGuard &) = delete;
	MapGuard &operator=(const MapGuard &) = delete;

      private:
	cgck_ctx *c_;
};

// The writer side: g_map_wr held; no request of any server context is in
// flight on the host side when it returns (ended by ~MapChange).
class MapChange {
      public:
	MapChange() : lk_(g_map_wr)
	{
		g_map_changing.store(1, std::memory_order_seq_cst);
		// (the list copied: no lock held while waiting; it cannot change
		// meanwhile, burst open / close take g_map_wr)
		std::vector<cgck_ctx *> srv;
		{
			std::lock_guard<std::mutex> lk(g_srv_mu);
			srv = g_srv;
		}
		for (cgck_ctx *c : srv)
			for (uint32_t k = 0; __atomic_load_n(&c->bbusy, __ATOMIC_SEQ_CST); k++) {
				if (k < 4096)
					__builtin_ia32_pause();
				else
					sched_yield();
			}
	}
	~MapChange() { g_map_changing.store(0, std::memory_order_release); }
	MapChange(const MapChange &) = delete;
	MapChange &operator=(const MapChange &) = delete;

      private:
	std::lock_guard<std::mutex> lk_;
};
} // namespace

static void free_or_park(void *p, bool host)
{
	bool resident;
	{
		std::lock_guard<std::mutex> lk(g_srv_mu);
		resident = !g_srv.empty();
	}
	if (resident) {
		std::lock_guard<std::mutex> lk(g_park_mu);
		g_parked.emplace_back(p, host);
		return;
	}
	if (host)
		(void)hipHostFree(p);
	else
		(void)hipFree(p);
}

// The parked buffers, freed once no server is resident (caller: after a
// close took its server out of g_srv).
static void free_parked()
{
	{
		std::lock_guard<std::mutex> lk(g_srv_mu);
		if (!g_srv.empty())
			return;
	}
	std::vector<std::pair<void *, bool>> v;
	{
		std::lock_guard<std::mutex> lk(g_park_mu);
		v.swap(g_parked);
	}
	for (const auto &x : v) {
		if (x.second)
			(void)hipHostFree(x.first);
		else
			(void)hipFree(x.first);
	}
}

static bool burst_all_alive(const cgck_ctx *c);
static int burst_restart(cgck_ctx *c);

// The stop word the leader polls: beside the device-memory doorbell (written
// through the large BAR, pushed out of the write-combining buffer) or in the
// host mailbox.
static void burst_stop(cgck_ctx *c, uint32_t v)
{
	if (c->bdoor) {
		__builtin_ia32_sfence();
		__atomic_store_n((uint32_t *)(c->bdoor + 2), v, __ATOMIC_RELAXED);
		__builtin_ia32_sfence();
	}
	__atomic_store_n(&c->bbox->stop, v, __ATOMIC_RELEASE);
}

// Requests complete in order, so the last one known complete is the latest
// seq collected, whatever order the posted requests are collected in (the
// pipelined windows collect a TX fill, then the older RX burst that shares
// nothing with it).  bdone only moves forward: a relaunch starts after it, and
// one that started after an older seq would have its leader poll a slot the
// host has since posted a later request into.
static void burst_done_at(cgck_ctx *c, uint32_t seq)
{
	if ((int32_t)(seq - c->bdone) > 0)
		c->bdone = seq;
}

// Serve every request posted to c and not collected yet (the seqs after
// bdone up to bseq: a pipelined window's burst or fill), relaunching the
// server if it idled out, without collecting them: their outputs stay in
// their slots for the poster's own collect, which then finds them done.
// The caller holds a MapChange, so neither seq moves meanwhile.
// A request not served in 2 s is abandoned (the next launch starts after
// it; its poster's collect times out): it must not be served after the
// mapping it reads has changed.
static void burst_finish_posted(cgck_ctx *c)
{
	BurstBox *b = c->bbox;
	for (uint32_t s = c->bdone, k = 0; s != c->bseq && k < 4; k++) {
		s = burst_next(s);
		const uint32_t n = (uint32_t)(c->breq[s & 1] >> 32) & ~kBurstVram;
		const uint32_t W = burst_wgs(n, c->bwgs, c->bper);
		const double t0 = now_s();
		uint32_t j = 0;
		for (uint32_t spin = 0; j < W;) {
			if ((int32_t)(__atomic_load_n(&b->done[j], __ATOMIC_ACQUIRE) - s) >= 0) {
				j++;
				continue;
			}
			__builtin_ia32_pause();
			if ((++spin & 1023) != 0)
				continue;
			if (!burst_all_alive(c) && burst_restart(c) != 0)
				return;
			if (now_s() - t0 > 2.0) {
				c->bdone = c->bseq;
				return;
			}
		}
		// served: the relaunch after the mapping change starts after it (its
		// outputs stay in the slot for the poster's collect, which finds its
		// done words past it), so it is never served again over the new mapping
		burst_done_at(c, s);
	}
}

// Stop every open server and wait until its workgroups have left (caller
// holds a MapChange, so no request is posted meanwhile).  Requests
// already posted are served first (burst_finish_posted): a relaunch after
// the mapping change must not read or store through a range that is gone.
static void burst_quiesce_all()
{
	std::lock_guard<std::mutex> lk(g_srv_mu);
	for (cgck_ctx *c : g_srv) {
		if (!c->bbox)
			continue;
		(void)hipSetDevice(c->device);
		burst_finish_posted(c);
		burst_stop(c, 1u);
		(void)CGCK_SYNC(c->bstream);
		burst_stop(c, 0u);
	}
}

static int burst_launch(cgck_ctx *c, uint32_t start_seq)
{
	uint32_t epoch;
	while ((epoch = g_burst_epoch.fetch_add(1, std::memory_order_relaxed) + 1) == 0)
		;
	for (uint32_t j = 0; j < c->bwgs; j++)
		__atomic_store_n(&c->bbox->alive[j], (uint8_t)1, __ATOMIC_RELEASE);
	hipError_t e = launch_burst_server(c->bbox_dev, c->bdoor ? c->bdoor : c->bbox_dev->req,
					   c->bdoor ? (const uint32_t *)(c->bdoor + 2) : &c->bbox_dev->stop, c->bstage_dev, c->bvblk,
					   c->bscratch, c->bresp_dev, c->brelay, c->d_zero, (uint32_t)c->bstage_cap,
					   c->bmax, c->bwgs, c->bper, start_seq, epoch, server_opts(), c->bstream);
	if (e != hipSuccess) {
		for (uint32_t j = 0; j < c->bwgs; j++)
			__atomic_store_n(&c->bbox->alive[j], (uint8_t)0, __ATOMIC_RELEASE);
		return set_err(-EIO, "burst server launch: %s", hipGetErrorString(e));
	}
	return 0;
}

static bool burst_all_alive(const cgck_ctx *c)
{
	for (uint32_t j = 0; j < c->bwgs; j++)
		if (!__atomic_load_n(&c->bbox->alive[j], __ATOMIC_ACQUIRE))
			return false;
	return true;
}

// A workgroup has idled out (or the server is draining): stop the rest,
// wait until every workgroup has left, relaunch them for the requests after
// the last one completed (the pending ones are still in their slots).
static int burst_restart(cgck_ctx *c)
{
	(void)hipSetDevice(c->device);
	burst_stop(c, 1u);
	const hipError_t e = CGCK_SYNC(c->bstream);
	burst_stop(c, 0u);
	if (e != hipSuccess)
		return set_err(-EIO, "burst server drain: %s", hipGetErrorString(e));
	return burst_launch(c, c->bdone);
}

// A request costs the poll, the round trips of the request block and the
// packet bytes, and the outputs' write acknowledgements (~5 us for a small
// one, tools/pingpong) instead of a launch and a stream synchronisation
// (~9.4 us for an empty kernel).  Up to kBurstOneWG packets one workgroup
// serves it from one wide read of the block; larger requests are split over
// up to K workgroups, each reading its slice of the descriptors and the
// packet bytes where they lie.  Registered packets are copied into the block
// up to 32 KiB of block (one read for a small request) and read in place
// above; in-place requests carry their range, which the server checks every
// descriptor against.  The TX window's flush goes through cgck_desc_host of
// its ring range, so it takes the server whenever it fits.  Which requests go
// to the server is the caller's choice at open: cgck_burst_open's max_pkts
// and max_bytes (packet bytes per request).  The launch path's many
// workgroups read the fabric faster for hundreds of frames of >= 576 B (256 x
// 576 B: 22.8 vs 29.2 us), the server wins below ~100 KiB of packet bytes
// (profiles/r03/burst), so max_bytes ~96 KiB routes a mixed workload best.
// $CGCK_SERVER_PKTS / _COPY override the caps for A/B runs (lab build).
//
// Two requests may be outstanding (two slots, cgck_internal.h): a posted
// request is collected (burst_wait, then its outputs read from its slot)
// before its slot is posted to again.  The synchronous callers post and
// collect at once; the pipelined windows (cgck_rx_post, cgck_tx_post) leave
// one request posted while the stack works, and a later post that needs its
// slot collects it first (burst_slot_free).
static size_t env_size(const char *v, size_t dflt)
{
	return v && *v ? (size_t)strtoull(v, nullptr, 0) : dflt;
}
static const uint64_t kServerPkts = env_size(CGCK_ENV("CGCK_SERVER_PKTS"), kServerPktsDefault);
static const size_t kServerCopy = env_size(CGCK_ENV("CGCK_SERVER_COPY"), kServerCopyDefault);

// (BurstLayout, burst_layout and the predicates below: cgck_route.h, which
// burst_route names a request's route from)

// Does a request of n packets of at most max_len bytes, `data` packet bytes
// of which `staged` are copied into the block (0 when read in place), go to
// the server?
static bool burst_fits(const cgck_ctx *c, uint64_t n, uint32_t max_len, size_t staged, size_t data)
{
	(void)max_len;
	return c->bbox && burst_fits_caps(c->bmax, kServerPkts, c->bstage_cap, c->bmax_bytes, n, staged, data);
}

static uint8_t *burst_block(const cgck_ctx *c, uint32_t seq) { return c->bstage + (size_t)(seq & 1) * c->bstage_cap; }

static const uint8_t *burst_resp(const cgck_ctx *c, uint32_t seq)
{
	return c->bresp + (size_t)(seq & 1) * burst_resp_slot(c->bmax);
}

// Wait until request seq (n packets) is served.  Requests complete in order,
// so a workgroup's done word at or past seq means its slice is in.
static int burst_wait(cgck_ctx *c, uint32_t seq, uint32_t n, uint64_t range)
{
#if CGCK_LAB
	const uint64_t tl0 = __builtin_ia32_rdtsc();
#endif
	MapGuard map_g(c);
#if CGCK_LAB
	LAB_TICK(4, tl0);
	const uint64_t tl1 = __builtin_ia32_rdtsc();
#endif
	BurstBox *b = c->bbox;
	const uint32_t W = burst_wgs(n, c->bwgs, c->bper);
	const double t0 = now_s();
	uint32_t spin = 0;
	for (uint32_t j = 0; j < W;) {
		if ((int32_t)(__atomic_load_n(&b->done[j], __ATOMIC_ACQUIRE) - seq) >= 0) {
			j++;
			continue;
		}
		__builtin_ia32_pause();
		if ((++spin & 1023) != 0)
			continue;
#if CGCK_LAB
		// lab: a wait past 20 ms says what the server looked like (the
		// driver's bench once saw one loop iteration take the server's
		// 200 ms idle bound)
		if (now_s() - t0 > 0.02 && !(spin & ((1u << 20) - 1))) {
			char dw[200];
			int at = 0;
			for (uint32_t k = 0; k < c->bwgs && at < (int)sizeof(dw) - 16; k++)
				at += snprintf(dw + at, sizeof(dw) - at, " %u:%u%s", k, __atomic_load_n(&b->done[k], __ATOMIC_ACQUIRE),
					       __atomic_load_n(&b->alive[k], __ATOMIC_ACQUIRE) ? "" : "x");
			fprintf(stderr,
				"cgck lab: wait %.1f ms for seq %u (n %u, W %u): bseq %u bdone %u breq %#llx %#llx "
				"slots %p %p done/alive%s\n",
				(now_s() - t0) * 1e3, seq, n, W, c->bseq, c->bdone, (unsigned long long)c->breq[0],
				(unsigned long long)c->breq[1], (void *)c->bslot[0], (void *)c->bslot[1], dw);
		}
#endif
		if (!burst_all_alive(c)) {
			// a workgroup exited between the post and its last poll: drain
			// and relaunch for the pending requests (slices already served
			// are not served again: the server's recheck)
			int rc = burst_restart(c);
			if (rc)
				return rc;
		}
		if (now_s() - t0 > 2.0) {
			// Drain before returning, so no workgroup touches the caller's
			// memory after the call (each leaves within its idle bound),
			// and say which slices never came back.
			char miss[160];
			int at = 0;
			for (uint32_t k = 0; k < W && at < (int)sizeof(miss) - 12; k++)
				if ((int32_t)(__atomic_load_n(&b->done[k], __ATOMIC_ACQUIRE) - seq) < 0)
					at += snprintf(miss + at, sizeof(miss) - at, " %u:%u", k,
						       __atomic_load_n(&b->done[k], __ATOMIC_ACQUIRE));
			miss[at] = 0;
			burst_stop(c, 1u);
			(void)CGCK_SYNC(c->bstream);
			burst_stop(c, 0u);
			uint64_t relay[3] = {0, 0, 0};
			(void)hipMemcpy(relay, c->brelay, sizeof(relay), hipMemcpyDeviceToHost);
			burst_done_at(c, seq); // abandoned: the next launch starts after it
			return set_err(-ETIMEDOUT,
				       "burst server: request %u (n %u, W %u) not served in 2 s; missing (wg:done)%s; "
				       "relay %#llx %#llx %#llx",
				       seq, n, W, miss, (unsigned long long)relay[0], (unsigned long long)relay[1],
				       (unsigned long long)relay[2]);
		}
	}
#if CGCK_LAB
	t_lab_host[1] = (uint64_t)(now_s() * 1e9);
	LAB_TICK(5, tl1);
#endif
	burst_done_at(c, seq);
	if (__atomic_load_n(&b->refused[seq & 1], __ATOMIC_ACQUIRE) == seq)
		return set_err(-EIO,
			       "burst server: request %u refused (block header, or a descriptor outside the block or "
			       "past the %llu-byte range)",
			       seq, (unsigned long long)range);
	return 0;
}

// Collect a posted request: wait for it and copy its outputs where its
// poster asked; frees its slot.
int cgck::burst_collect(cgck_ctx *c, BurstPending *p)
{
	if (!p->seq)
		return p->rc;
	const uint32_t seq = p->seq;
	p->seq = 0;
	if (c->bslot[seq & 1] == p)
		c->bslot[seq & 1] = nullptr;
	// The GPU wrote the done words and the response, so none of their lines
	// is in this core's caches: a posted request is usually served by now,
	// so start those misses together instead of one after the other.
	{
		const uint8_t *o = burst_resp(c, seq);
		__builtin_prefetch(&c->bbox->done[0]);
		const uint32_t lim = 4 * p->n < 512 ? 4 * p->n : 512;
		for (uint32_t at = 0; at < lim; at += 64) {
			if (p->out)
				__builtin_prefetch(o + at);
			if (p->meta)
				__builtin_prefetch(o + burst_meta_off(p->n) + at);
		}
	}
	int rc = burst_wait(c, seq, p->n, p->range);
	if (rc == 0) {
#if CGCK_LAB
		const uint64_t tc0 = __builtin_ia32_rdtsc();
#endif
		const uint8_t *o = burst_resp(c, seq);
		if (p->out)
			memcpy(p->out, o, 4 * (size_t)p->n);
		if (p->meta)
			memcpy(p->meta, o + burst_meta_off(p->n), 4 * (size_t)p->n);
		if (p->verdict)
			memcpy(p->verdict, o + burst_ver_off(p->n), p->n);
#if CGCK_LAB
		LAB_TICK(2, tc0);
#endif
	}
	p->rc = rc;
	return rc;
}

int cgck::burst_ready(cgck_ctx *c, const BurstPending *p)
{
	if (!p->seq)
		return 1;
	const uint32_t W = burst_wgs(p->n, c->bwgs, c->bper);
	for (uint32_t j = 0; j < W; j++)
		if ((int32_t)(__atomic_load_n(&c->bbox->done[j], __ATOMIC_ACQUIRE) - p->seq) < 0) {
			// not served yet: a server that idled out between the post and
			// its last poll is relaunched here, as burst_wait would, so a
			// caller that only ever asks does not wait forever
			if (!burst_all_alive(c)) {
				MapGuard map_g(c);
				(void)burst_restart(c);
			}
			return 0;
		}
	return 1;
}

// The block of the next request (L.bytes of it), with its slot free: a
// posted request still holding that slot is collected first.  A block of up
// to kBurstVramMax bytes (a drop-in call on up to ~1.9 KiB, a burst of up to
// ~165 descriptors in place) goes to the slot's device-memory block when the
// device has one: the host writes it through the large BAR (write-combined)
// and the server reads it locally instead of across the fabric
// (tools/vramdb: 4.70 against 5.55 us for the bare round trip of a 4 KiB
// block, profiles/r06/).  Larger blocks stay in host staging: the host's
// write-combined stores cost ~0.13 us a KiB (0.53 us for 4 KiB against 0.06
// into host memory), which is the worker's time.  So do the blocks of posted
// requests (the pipelined / coalesced windows): their latency is hidden
// behind the stack's work, while the write-combined stores would be the
// worker's own; only their doorbell goes to device memory.
static const size_t kBurstVramMax = env_size(CGCK_ENV("CGCK_BURST_VRAM_MAX"), 2048); // lab A/B: the bound
static const size_t kBurstVramPostedMax = env_size(CGCK_ENV("CGCK_BURST_VRAM_POSTED_MAX"), 0); // lab A/B: posted ones
static int burst_slot_free(cgck_ctx *c, const BurstLayout &L, uint8_t **block, bool posted = false)
{
	const uint32_t seq = burst_next(c->bseq);
	if (BurstPending *p = c->bslot[seq & 1]) {
		const int rc = burst_collect(c, p); // its poster reads p->rc
		(void)rc;
	}
	c->bnext_vram = c->bvblk && L.bytes <= (posted ? kBurstVramPostedMax : kBurstVramMax) && L.bytes <= kBurstFirst;
	*block = c->bnext_vram ? c->bvblk + (size_t)(seq & 1) * kBurstFirst : burst_block(c, seq);
	return 0;
}

// Post the request whose descriptors (and, for base_dev == nullptr, packet
// bytes) are in the next block; returns its seq.
static int burst_post(cgck_ctx *c, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
		      uint32_t max_len, const BurstLayout &L, uint32_t *seq_out, const DescSplit *split = nullptr)
{
	MapGuard map_g(c);
	BurstBox *b = c->bbox;
	const uint32_t seq = burst_next(c->bseq);
	const bool vram = c->bnext_vram;
	BurstReq *r = (BurstReq *)(vram ? c->bvblk + (size_t)(seq & 1) * kBurstFirst : burst_block(c, seq));
	r->n = (uint32_t)n;
	r->flags = flags;
	r->max_len = max_len;
	r->bytes = (uint32_t)L.bytes;
	r->base = (uint64_t)(uintptr_t)base_dev;
	r->range = base_dev ? range : 0;
	r->d_off = (uint32_t)L.d_off;
	r->p_off = (uint32_t)L.p_off;
	r->n1 = split ? split->n1 : 0;
	r->flags2 = split ? split->flags2 : 0;
	c->bseq = seq;
#if CGCK_LAB
	t_lab_host[0] = (uint64_t)(now_s() * 1e9);
#endif
	const uint64_t word = (uint64_t)seq | (uint64_t)((uint32_t)n | (vram ? kBurstVram : 0u)) << 32;
	c->breq[seq & 1] = word;
	if (c->bdoor) {
		// The block's stores (write-combined device memory, or host memory)
		// are out before the doorbell, and the doorbell leaves the
		// write-combining buffer now rather than at its next eviction.
		__builtin_ia32_sfence();
		__atomic_store_n(&c->bdoor[seq & 1], word, __ATOMIC_RELAXED);
		__builtin_ia32_sfence();
	} else {
		__atomic_store_n(&b->req[seq & 1], word, __ATOMIC_RELEASE);
	}
	*seq_out = seq;
	if (!burst_all_alive(c)) {
		int rc = burst_restart(c); // idled out: a new server picks the pending requests up
		if (rc)
			return rc;
	}
	return 0;
}

// Post and collect at once: outputs at burst_resp(c, *seq_out).
static int burst_serve(cgck_ctx *c, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
		       uint32_t max_len, const BurstLayout &L, uint32_t *seq_out)
{
	int rc = burst_post(c, base_dev, range, n, flags, max_len, L, seq_out);
	if (rc)
		return rc;
	return burst_wait(c, *seq_out, (uint32_t)n, range);
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
	size_t pkt_bytes = sum ? sum->pkt_bytes : 0;
	uint32_t max_len = sum ? sum->max_len : 0;
	for (uint64_t i = 0; i < n && !sum; i++) {
		max_len = desc[i].ip_len > max_len ? desc[i].ip_len : max_len;
		const uint64_t end = desc[i].frame_off + desc[i].l3_off + desc[i].ip_len;
		if (end > bytes || end < desc[i].frame_off)
			return set_err(-EINVAL, "cgck_desc_host: descriptor %llu reaches past the %zu bytes given",
				       (unsigned long long)i, bytes);
		pkt_bytes += ((size_t)desc[i].ip_len + 15) & ~(size_t)15;
	}
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
	int rc;
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
	    burst_fits(c, n, max_len, in_place ? 0 : pkt_bytes, pkt_bytes)) {
		// the resident server: no launch, no stream sync
		const BurstLayout L = burst_layout(in_place ? 0 : pkt_bytes, n);
		uint8_t *h;
		if ((rc = burst_slot_free(c, L, &h, pend != nullptr)))
			return rc;
		cgck_desc_t *d = (cgck_desc_t *)(h + L.d_off);
		if (in_place) {
			memcpy(d, desc, 12 * n);
		} else {
			size_t at = 0;
			for (uint64_t i = 0; i < n; i++) {
				memcpy(h + L.p_off + at, (const uint8_t *)base + desc[i].frame_off + desc[i].l3_off,
				       desc[i].ip_len);
				d[i].frame_off = at;
				d[i].l3_off = 0;
				d[i].ip_len = desc[i].ip_len;
				at += ((size_t)desc[i].ip_len + 15) & ~(size_t)15;
			}
		}
		uint32_t seq;
		if ((rc = burst_post(c, in_place ? (const uint8_t *)dev_base : nullptr, bytes, n, flags, max_len, L, &seq,
				     split)))
			return rc;
		BurstPending now;
		BurstPending *q = pend ? pend : &now;
		q->seq = seq;
		q->n = (uint32_t)n;
		q->range = bytes;
		q->out = out;
		q->meta = meta;
		q->verdict = verdict;
		q->rc = 0;
		if (pend) {
			c->bslot[seq & 1] = pend;
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
		if (dev_base) {
			memcpy(d, desc, 12 * n);
		} else {
			size_t at = 0;
			for (uint64_t i = 0; i < n; i++) {
				memcpy(h + at, (const uint8_t *)base + desc[i].frame_off + desc[i].l3_off, desc[i].ip_len);
				d[i].frame_off = at;
				d[i].l3_off = 0;
				d[i].ip_len = desc[i].ip_len;
				at += ((size_t)desc[i].ip_len + 15) & ~(size_t)15;
			}
		}
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
	if (!burst_fits(c, n, max_len, 0, 0))
		return set_err(-ENOSPC, "cgck_burst_request: no burst server open on the context, or %llu packets "
					"exceed its capacity", (unsigned long long)n);
	const BurstLayout L = burst_layout(0, n);
	uint8_t *h;
	if ((rc = burst_slot_free(c, L, &h)))
		return rc;
	memcpy(h + L.d_off, desc, 12 * n);
	uint32_t seq;
	if ((rc = burst_serve(c, (const uint8_t *)dev_base, range, n, flags, max_len, L, &seq)))
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
	MapChange map_c;
	burst_quiesce_all();
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
	MapChange map_c;
	burst_quiesce_all();
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
	if (ip_len <= 0xffff && !(flags & CGCK_STORE) && burst_fits(c, 1, ip_len, span, span)) {
		// the resident server: one descriptor, no launch, no stream sync
		const BurstLayout L = burst_layout(span, 1);
		uint8_t *h;
		if ((rc = burst_slot_free(c, L, &h)))
			return rc;
		if (span)
			memcpy(h + L.p_off, src, span);
		cgck_desc_t *d = (cgck_desc_t *)(h + L.d_off);
		d->frame_off = 0;
		d->l3_off = 0;
		d->ip_len = (uint16_t)ip_len;
		uint32_t seq;
		if ((rc = burst_serve(c, nullptr, 0, 1, flags, ip_len, L, &seq)))
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

// The server's stream.  A resident kernel holds its hardware queue until it
// exits, and HIP multiplexes streams over a few hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default): a plain stream may share the server's
// queue with another stream of the process, whose work then waits behind the
// server until it idles out.  A stream with a CU mask gets a queue of its
// own, so the server is given one (every CU enabled: the mask only buys the
// dedicated queue).  $CGCK_BURST_PLAIN_STREAM (lab build) takes a plain one.
static hipError_t burst_stream(const cgck_ctx *c, hipStream_t *st)
{
	if (CGCK_ENV("CGCK_BURST_PLAIN_STREAM"))
		return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
	uint32_t mask[16];
	const int words = (c->num_cus + 31) / 32 < 16 ? (c->num_cus + 31) / 32 : 16;
	for (int i = 0; i < words; i++)
		mask[i] = ~0u;
	if (c->num_cus % 32 && words == (c->num_cus + 31) / 32)
		mask[words - 1] = (1u << (c->num_cus % 32)) - 1;
	return hipExtStreamCreateWithCUMask(st, (uint32_t)words, mask);
}

// Resident servers a device takes from this process: each holds a hardware
// queue of its own (burst_stream), and with 20 or more a device could not map
// every server's queue on every XCD at once — a server's workgroups on one XCD
// never started (a request not served in 2 s) or waited ms for the
// scheduler's time slice (tools/txloop workers mode, 16 / 20 / 24 / 28 / 32
// workers on one MI355X, profiles/r06/).  With 16 servers the process's
// other streams (HIP's shared queues, GPU_MAX_HW_QUEUES = 4) starved in
// turn: 16 more workers launching their requests recorded no burst in 0.3 s
// (profiles/r06/doorab/workers.log), so the cap leaves them room.  con-gen's
// 32 workers bound over a node's eight GPUs hold four each.
constexpr uint32_t kMaxServersPerDevice = 12;

// The server's stream and memory, freed (no server kernel running).
static void burst_release(cgck_ctx *c)
{
	(void)hipStreamDestroy(c->bstream);
	for (void *h : {(void *)c->bbox, (void *)c->bstage, (void *)c->bresp})
		free_or_park(h, true);
	for (void *d : {(void *)c->bscratch, (void *)c->brelay, (void *)c->bdoor})
		if (d)
			free_or_park(d, false);
	c->bdoor = nullptr;
	c->bvblk = nullptr;
	c->bbox = nullptr;
	c->bstage = nullptr;
	c->bstage_cap = 0;
	c->bresp = nullptr;
	c->bscratch = nullptr;
	c->brelay = nullptr;
}

extern "C" int cgck_burst_open(cgck_ctx_t *c, uint32_t max_pkts, size_t max_bytes, uint32_t idle_ms)
{
	if (!c && !(c = thread_ctx()))
		return -ENODEV; // thread_ctx set the message
	if (c->bbox)
		return set_err(-EBUSY, "cgck_burst_open: already open on this context");
	if (max_pkts == 0 || max_bytes == 0)
		return set_err(-EINVAL, "cgck_burst_open: zero capacity");
	if (max_pkts >= kBurstVram)
		return set_err(-EINVAL, "cgck_burst_open: max_pkts %u", max_pkts);
	HIP_TRY(hipSetDevice(c->device));
	// the block holds the header, the descriptors and the packet bytes; the
	// server's first read fetches kBurstFirst bytes whatever the request
	const size_t cap = burst_stage_cap(max_pkts, max_bytes);
	// two slots of outputs, each for the largest request
	size_t resp_bytes = 2 * (size_t)burst_resp_slot(max_pkts);
	unsigned resp_flags = hipHostMallocCoherent;
	if (const char *e = CGCK_ENV("CGCK_BRESP_MIN")) // lab A/B: allocation size of the outputs
		resp_bytes = resp_bytes < env_size(e, 0) ? env_size(e, 0) : resp_bytes;
	if (const char *e = CGCK_ENV("CGCK_BRESP_FLAGS")) // lab A/B: their hipHostMalloc flags
		resp_flags = (unsigned)env_size(e, hipHostMallocCoherent);
	void *box = nullptr, *st = nullptr, *rs = nullptr, *bd = nullptr, *sd = nullptr, *rd = nullptr, *sc = nullptr;
	hipError_t e = hipHostMalloc(&box, sizeof(BurstBox), hipHostMallocCoherent);
	if (e == hipSuccess)
		e = hipHostMalloc(&st, 2 * cap, hipHostMallocCoherent); // two request slots
	if (e == hipSuccess)
		e = hipHostMalloc(&rs, resp_bytes, resp_flags);
	if (e == hipSuccess)
		e = hipMalloc(&sc, cap);
	// the leader's relay (one per slot, then the exit word), uncached: every poll and store
	// goes to memory, whichever XCD's L2 the workgroups sit behind
	void *rl = nullptr;
	if (e == hipSuccess)
		e = hipExtMallocWithFlags(&rl, 64, hipDeviceMallocUncached);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer(&bd, box, 0);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer(&sd, st, 0);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer(&rd, rs, 0);
	// The doorbell and the small-block slots in device memory the host writes
	// through the large BAR (every VRAM allocation is host-mapped there:
	// tools/vramdb), uncached so the server's polls and reads go to memory,
	// where the host's writes land.  $CGCK_BURST_HOST_DOOR (lab build): the
	// host-memory mailbox and blocks alone, the A/B.
	void *vd = nullptr;
	int large_bar = 0;
	if (e == hipSuccess && !CGCK_ENV("CGCK_BURST_HOST_DOOR") &&
	    hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, c->device) == hipSuccess && large_bar) {
		if (hipExtMallocWithFlags(&vd, 64 + 2 * (size_t)kBurstFirst, hipDeviceMallocUncached) != hipSuccess) {
			(void)hipGetLastError();
			vd = nullptr; // the host-memory mailbox then
		} else {
			// zeroed by the host itself: a hipMemset is asynchronous to the
			// host, and one still in flight when the first request's doorbell
			// was written wiped it (request 1 never served:
			// profiles/r06/bench_r6g)
			memset(vd, 0, 64 + 2 * (size_t)kBurstFirst);
			__builtin_ia32_sfence();
		}
	}
	if (e == hipSuccess)
		e = burst_stream(c, &c->bstream);
	if (e != hipSuccess) {
		for (void *h : {box, st, rs})
			if (h)
				(void)hipHostFree(h);
		for (void *d : {sc, rl, vd})
			if (d)
				(void)hipFree(d);
		return set_err(-EIO, "cgck_burst_open: %s", hipGetErrorString(e));
	}
	c->bdoor = (uint64_t *)vd;
	c->bvblk = vd ? (uint8_t *)vd + 64 : nullptr;
	c->bnext_vram = false;
	c->breq[0] = c->breq[1] = 0;
	memset(box, 0, sizeof(BurstBox));
	memset(st, 0, 2 * cap);
	c->bbox = (BurstBox *)box;
	// one workgroup per kBurstPerWG packets of the largest request, at most
	// kBurstMaxWG (and the device's CUs)
	c->bper = kBurstPerWG;
	if (const char *e = CGCK_ENV("CGCK_SERVER_PER_WG")) // lab A/B: packets per workgroup
		c->bper = atoi(e) > 0 ? (uint32_t)atoi(e) : c->bper;
	c->bwgs = burst_wgs(max_pkts, kBurstMaxWG, c->bper);
	if (c->bwgs > (uint32_t)c->num_cus)
		c->bwgs = (uint32_t)c->num_cus;
	if (const char *e = CGCK_ENV("CGCK_SERVER_WGS")) // lab A/B: K
		c->bwgs = atoi(e) > 0 && atoi(e) <= (int)kBurstMaxWG ? (uint32_t)atoi(e) : c->bwgs;
	c->bbox->idle_ticks = (uint64_t)(idle_ms ? idle_ms : 200) * 100000; // 100 MHz counter
	c->bstage = (uint8_t *)st;
	c->bstage_cap = cap;
	c->bstage_dev = (uint8_t *)sd;
	c->bbox_dev = (BurstBox *)bd;
	c->bresp = (uint8_t *)rs;
	c->bresp_dev = (uint8_t *)rd;
	c->bscratch = (uint8_t *)sc;
	c->brelay = (uint64_t *)rl;
	c->bmax = max_pkts;
	c->bmax_bytes = max_bytes;
	c->bseq = 0;
	c->bdone = 0;
	c->bbad = 0;
	c->bslot[0] = c->bslot[1] = nullptr;
	c->bbusy = 0;
	std::lock_guard<std::mutex> map_wr(g_map_wr); // no mapping changes while it joins g_srv and launches
	bool full = false;
	uint32_t on_dev = 0;
	{
		std::lock_guard<std::mutex> lk(g_srv_mu);
		for (const cgck_ctx *x : g_srv)
			on_dev += x->device == c->device;
		full = on_dev >= kMaxServersPerDevice;
		if (!full)
			g_srv.push_back(c);
	}
	if (full) {
		burst_release(c);
		return set_err(-EBUSY,
			       "cgck_burst_open: %u burst servers already resident on device %d (each holds a hardware "
			       "queue of its own, and a device maps only ~20 at once: beyond that, servers' workgroups "
			       "and other streams' launches stall for ms to s, tools/txloop workers mode); bind the "
			       "workers over more devices (cgck_thread_bind) or leave this one without",
			       on_dev, c->device);
	}
	return burst_launch(c, 0);
}

// Test hooks in the product library (include/cgck.h, tests/test_gpu_burst_seq.py:
// the driver's -m gpu gate runs the 32-bit seq-wrap test against libcgck.so).
// cgck_test_burst_seq: restart ctx's server as if `seq` were the last request
// served (a few seqs before the wrap).  cgck_test_burst_stale: with the
// server running and nothing posted, set the done words of workgroups >= from
// half the seq space ahead, as a word untouched for 2^31 requests would
// compare; the next request must refresh them (a workgroup outside a
// request's slices stores the seq it steps over), or a wider request after it
// would be reported served before those workgroups wrote anything.
extern "C" int cgck_test_burst_seq(cgck_ctx_t *c, uint32_t seq)
{
	if (!c || !c->bbox || c->bslot[0] || c->bslot[1])
		return set_err(-EINVAL, "cgck_test_burst_seq: no open server, or a request posted");
	if (seq == 0)
		return set_err(-EINVAL, "cgck_test_burst_seq: seq 0 is never posted");
	MapGuard map_g(c);
	burst_stop(c, 1u);
	const hipError_t e = CGCK_SYNC(c->bstream);
	burst_stop(c, 0u);
	if (e != hipSuccess)
		return set_err(-EIO, "cgck_test_burst_seq: drain: %s", hipGetErrorString(e));
	for (uint32_t j = 0; j < kBurstMaxWG; j++)
		__atomic_store_n(&c->bbox->done[j], seq, __ATOMIC_RELEASE);
	c->bbox->req[0] = c->bbox->req[1] = 0;
	c->breq[0] = c->breq[1] = 0;
	if (c->bdoor) {
		__atomic_store_n(&c->bdoor[0], 0ull, __ATOMIC_RELAXED);
		__atomic_store_n(&c->bdoor[1], 0ull, __ATOMIC_RELAXED);
		__builtin_ia32_sfence();
	}
	c->bbox->refused[0] = c->bbox->refused[1] = 0;
	c->bseq = c->bdone = seq;
	return burst_launch(c, seq);
}

extern "C" int cgck_test_burst_stale(cgck_ctx_t *c, uint32_t from)
{
	if (!c || !c->bbox || c->bslot[0] || c->bslot[1])
		return set_err(-EINVAL, "cgck_test_burst_stale: no open server, or a request posted");
	for (uint32_t j = from; j < kBurstMaxWG; j++)
		__atomic_store_n(&c->bbox->done[j], c->bseq + 0x7ffffff0u, __ATOMIC_RELEASE);
	return 0;
}

#if CGCK_LAB
// Lab: what one host load of a BurstBox word costs while the server polls
// (ns, mean over reps, each load after ~2 us of spin): out[0] the mailbox
// line (stop, which the leader polls with req), out[1] refused[] (the same
// line today), out[2] done[0], out[3] alive[0].  NULL: the thread's context.
extern "C" int cgck_lab_box_probe(cgck_ctx_t *c, int reps, double out[4])
{
	if (!c)
		c = cgck::thread_ctx_if_any();
	if (!c || !c->bbox || reps <= 0)
		return -EINVAL;
	const volatile uint32_t *w[4] = {&c->bbox->stop, &c->bbox->refused[0], &c->bbox->done[0],
					 (const volatile uint32_t *)&c->bbox->alive[0]};
	for (int k = 0; k < 4; k++) {
		double acc = 0;
		uint32_t sink = 0;
		for (int i = 0; i < reps; i++) {
			for (const double s0 = now_s(); now_s() - s0 < 2e-6;)
				;
			struct timespec a, b;
			clock_gettime(CLOCK_MONOTONIC, &a);
			sink += *w[k];
			__atomic_thread_fence(__ATOMIC_SEQ_CST);
			clock_gettime(CLOCK_MONOTONIC, &b);
			acc += (b.tv_sec - a.tv_sec) * 1e9 + (b.tv_nsec - a.tv_nsec);
		}
		out[k] = acc / reps + (sink == 0xdeadbeef ? 1e-9 : 0);
	}
	return 0;
}

// Lab: workgroup 0's timestamps of the last request (100 MHz ticks: seen,
// block read, computed, published; then the compute phase in shader clocks)
// and the host's view of that request (ns: post, done seen) for
// tools/srvlat.c.
extern "C" int cgck_lab_burst_times(cgck_ctx_t *c, uint64_t dev[5], uint64_t host[2])
{
	if (!c || !c->bbox)
		return -EINVAL;
	for (int i = 0; i < 4; i++)
		dev[i] = __atomic_load_n(&c->bbox->lab_t[i], __ATOMIC_ACQUIRE);
	dev[4] = __atomic_load_n(&c->bbox->lab_cyc, __ATOMIC_ACQUIRE);
	host[0] = t_lab_host[0];
	host[1] = t_lab_host[1];
	return 0;
}

// Lab: thread 0's shader clocks over the last one-workgroup request's body
// call alone (tools/srvlat's body_cycles, against tools/bodylat's).
extern "C" uint64_t cgck_lab_burst_body(cgck_ctx_t *c)
{
	return c && c->bbox ? __atomic_load_n(&c->bbox->lab_body, __ATOMIC_ACQUIRE) : 0;
}
#endif

extern "C" int cgck_burst_close(cgck_ctx_t *c)
{
	if (!c)
		c = thread_ctx_if_any(); // this thread's drop-in context, if it exists
	if (!c || !c->bbox)
		return 0;
	// posted requests complete first: their outputs land where their posters
	// asked (a window still open reads them)
	for (BurstPending *p : {c->bslot[0], c->bslot[1]})
		if (p)
			(void)burst_collect(c, p);
	std::lock_guard<std::mutex> map_wr(g_map_wr); // leaves g_srv with no mapping change under way
	{
		std::lock_guard<std::mutex> lk(g_srv_mu);
		for (size_t i = 0; i < g_srv.size(); i++)
			if (g_srv[i] == c) {
				g_srv.erase(g_srv.begin() + i);
				break;
			}
	}
	(void)hipSetDevice(c->device);
	burst_stop(c, 1u);
	hipError_t e = CGCK_SYNC(c->bstream); // the server sees `stop` within one poll
	burst_release(c);
	free_parked();
	if (e != hipSuccess)
		return set_err(-EIO, "cgck_burst_close: %s", hipGetErrorString(e));
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
	for (uint64_t i = 0; i < n; i++) {
		const uint64_t end = desc[i].frame_off + desc[i].l3_off + desc[i].ip_len;
		if (end > bytes || end < desc[i].frame_off)
			return set_err(-EINVAL, "cgck_rss_desc_host: descriptor %llu reaches past the %zu bytes given",
				       (unsigned long long)i, bytes);
	}
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
	*frames = l2d_pass_frames(c->num_cus);
	return 0;
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
