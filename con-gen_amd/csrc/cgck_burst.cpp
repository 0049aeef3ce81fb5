// cgck_burst.cpp — host side of the burst server (cgck_group.hip): small
// host-resident batches without a launch or a stream synchronisation each.
// The mailbox protocol, the relaunch logic, the map-change barrier, the park
// list, cgck_burst_open / _close, the test hooks and the lab hooks.  A
// context's server state is cgck_ctx::srv (cgck_burst.h), which also declares
// what the server's clients (cgck_api.cpp, cgck_dropin.cpp) call.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "cgck_host.h"

using namespace cgck;

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

static void burst_quiesce_all();

// No server kernel runs while a host mapping changes.  cgck_host_register /
// _unregister (and burst open / close) take g_map_wr, raise g_map_changing,
// wait until no context with a server is inside a request (its srv.busy word),
// and drain every open server (the next request relaunches it).  A request
// (post, wait, relaunch) runs inside a MapGuard on its own context: it sets
// the context's srv.busy and then checks g_map_changing (both sequentially
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

// Back off while busy() holds: 4096 pauses, then the scheduler.
template <class F> inline void spin_while(F busy)
{
	for (uint32_t k = 0; busy(); k++) {
		if (k < 4096)
			__builtin_ia32_pause();
		else
			sched_yield();
	}
}

class MapGuard {
      public:
	explicit MapGuard(cgck_ctx *c) : c_(c)
	{
		for (;;) {
			__atomic_store_n(&c_->srv.busy, 1u, __ATOMIC_SEQ_CST);
			if (!g_map_changing.load(std::memory_order_seq_cst))
				return;
			__atomic_store_n(&c_->srv.busy, 0u, __ATOMIC_RELEASE);
			spin_while([] { return g_map_changing.load(std::memory_order_acquire) != 0; });
		}
	}
	~MapGuard() { __atomic_store_n(&c_->srv.busy, 0u, __ATOMIC_RELEASE); }
	MapGuard(const MapGuard &) = delete;
	MapGuard &operator=(const MapGuard &) = delete;

      private:
	cgck_ctx *c_;
};
} // namespace

// The writer side: g_map_wr held; no request of any server context is in
// flight on the host side and every open server is drained when it returns
// (ended by ~MapChange).
cgck::MapChange::MapChange() : lk_(g_map_wr)
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
		spin_while([c] { return __atomic_load_n(&c->srv.busy, __ATOMIC_SEQ_CST) != 0; });
	burst_quiesce_all();
}

cgck::MapChange::~MapChange() { g_map_changing.store(0, std::memory_order_release); }

// hipFree / hipHostFree synchronise the device: with a burst server resident
// on it (a persistent kernel) such a free waits until every server idles out
// — 200 ms of a worker's loop (a coalesced loop whose fills outgrew the
// staging: tools/txloop, profiles/r06/stall/), or forever while other
// workers keep theirs busy.  So while any server is resident a buffer is not
// freed but parked, and parked buffers are freed once the last server has
// closed (burst_close).
void cgck::free_or_park(void *p, bool host)
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
	if (c->srv.door) {
		__builtin_ia32_sfence();
		__atomic_store_n((uint32_t *)(c->srv.door + 2), v, __ATOMIC_RELAXED);
		__builtin_ia32_sfence();
	}
	__atomic_store_n(&c->srv.box->stop, v, __ATOMIC_RELEASE);
}

// Stop the server, wait until every workgroup has left (each sees `stop`
// within one poll), and clear the stop word for the next launch.
static hipError_t burst_drain(cgck_ctx *c)
{
	burst_stop(c, 1u);
	const hipError_t e = CGCK_SYNC(c->srv.stream);
	burst_stop(c, 0u);
	return e;
}

// Has workgroup j served request seq?  Requests complete in order, so its
// done word at or past seq means its slice is in.
static inline bool burst_served(const BurstBox *b, uint32_t j, uint32_t seq)
{
	return (int32_t)(__atomic_load_n(&b->done[j], __ATOMIC_ACQUIRE) - seq) >= 0;
}

// Requests complete in order, so the last one known complete is the latest
// seq collected, whatever order the posted requests are collected in (the
// pipelined windows collect a TX fill, then the older RX burst that shares
// nothing with it).  srv.done only moves forward: a relaunch starts after it, and
// one that started after an older seq would have its leader poll a slot the
// host has since posted a later request into.
static void burst_done_at(cgck_ctx *c, uint32_t seq)
{
	if ((int32_t)(seq - c->srv.done) > 0)
		c->srv.done = seq;
}

// Serve every request posted to c and not collected yet (the seqs after
// srv.done up to srv.seq: a pipelined window's burst or fill), relaunching the
// server if it idled out, without collecting them: their outputs stay in
// their slots for the poster's own collect, which then finds them done.
// The caller holds a MapChange, so neither seq moves meanwhile.
// A request not served in 2 s is abandoned (the next launch starts after
// it; its poster's collect times out): it must not be served after the
// mapping it reads has changed.
static void burst_finish_posted(cgck_ctx *c)
{
	BurstServer &s = c->srv;
	for (uint32_t q = s.done, k = 0; q != s.seq && k < 4; k++) {
		q = burst_next(q);
		const uint32_t n = (uint32_t)(s.req[q & 1] >> 32) & ~kBurstVram;
		const uint32_t W = burst_wgs(n, s.wgs, s.per_wg);
		const double t0 = now_s();
		uint32_t j = 0;
		for (uint32_t spin = 0; j < W;) {
			if (burst_served(s.box, j, q)) {
				j++;
				continue;
			}
			__builtin_ia32_pause();
			if ((++spin & 1023) != 0)
				continue;
			if (!burst_all_alive(c) && burst_restart(c) != 0)
				return;
			if (now_s() - t0 > 2.0) {
				s.done = s.seq;
				return;
			}
		}
		// served: the relaunch after the mapping change starts after it (its
		// outputs stay in the slot for the poster's collect, which finds its
		// done words past it), so it is never served again over the new mapping
		burst_done_at(c, q);
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
		if (!c->srv.box)
			continue;
		(void)hipSetDevice(c->device);
		burst_finish_posted(c);
		(void)burst_drain(c);
	}
}

// (Re)launch the server's K workgroups; the first request each serves is
// the one after start_seq.
static int burst_launch(cgck_ctx *c, uint32_t start_seq)
{
	const BurstServer &s = c->srv;
	uint32_t epoch;
	while ((epoch = g_burst_epoch.fetch_add(1, std::memory_order_relaxed) + 1) == 0)
		;
	for (uint32_t j = 0; j < s.wgs; j++)
		__atomic_store_n(&s.box->alive[j], (uint8_t)1, __ATOMIC_RELEASE);
	hipError_t e = launch_burst_server(s.box_dev, s.door ? s.door : s.box_dev->req,
					   s.door ? (const uint32_t *)(s.door + 2) : &s.box_dev->stop, s.stage_dev, s.vblk,
					   s.scratch, s.resp_dev, s.relay, c->d_zero, (uint32_t)s.stage_cap, s.max_pkts,
					   s.wgs, s.per_wg, start_seq, epoch, server_opts(), s.stream);
	if (e != hipSuccess) {
		for (uint32_t j = 0; j < s.wgs; j++)
			__atomic_store_n(&s.box->alive[j], (uint8_t)0, __ATOMIC_RELEASE);
		return set_err(-EIO, "burst server launch: %s", hipGetErrorString(e));
	}
	return 0;
}

static bool burst_all_alive(const cgck_ctx *c)
{
	for (uint32_t j = 0; j < c->srv.wgs; j++)
		if (!__atomic_load_n(&c->srv.box->alive[j], __ATOMIC_ACQUIRE))
			return false;
	return true;
}

// A workgroup has idled out (or the server is draining): stop the rest,
// wait until every workgroup has left, relaunch them for the requests after
// the last one completed (the pending ones are still in their slots).
static int burst_restart(cgck_ctx *c)
{
	(void)hipSetDevice(c->device);
	const hipError_t e = burst_drain(c);
	if (e != hipSuccess)
		return set_err(-EIO, "burst server drain: %s", hipGetErrorString(e));
	return burst_launch(c, c->srv.done);
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
// slot collects it first (burst_next_block).
static size_t env_size(const char *v, size_t dflt)
{
	return v && *v ? (size_t)strtoull(v, nullptr, 0) : dflt;
}
static const uint64_t kServerPkts = env_size(CGCK_ENV("CGCK_SERVER_PKTS"), kServerPktsDefault);
const size_t cgck::kServerCopy = env_size(CGCK_ENV("CGCK_SERVER_COPY"), kServerCopyDefault);

// (BurstLayout, burst_layout and the predicates below: cgck_route.h, which
// burst_route names a request's route from)

// Does a request of n packets, `data` packet bytes of which `staged` are
// copied into the block (0 when read in place), go to the server?
bool cgck::burst_fits(const cgck_ctx *c, uint64_t n, size_t staged, size_t data)
{
	const BurstServer &s = c->srv;
	return s.box && burst_fits_caps(s.max_pkts, kServerPkts, s.stage_cap, s.max_bytes, n, staged, data);
}

const uint8_t *cgck::burst_resp(const cgck_ctx *c, uint32_t seq)
{
	return c->srv.resp + (size_t)(seq & 1) * burst_resp_slot(c->srv.max_pkts);
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
	BurstBox *b = c->srv.box;
	const uint32_t W = burst_wgs(n, c->srv.wgs, c->srv.per_wg);
	const double t0 = now_s();
	uint32_t spin = 0;
	for (uint32_t j = 0; j < W;) {
		if (burst_served(b, j, seq)) {
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
			for (uint32_t k = 0; k < c->srv.wgs && at < (int)sizeof(dw) - 16; k++)
				at += snprintf(dw + at, sizeof(dw) - at, " %u:%u%s", k, __atomic_load_n(&b->done[k], __ATOMIC_ACQUIRE),
					       __atomic_load_n(&b->alive[k], __ATOMIC_ACQUIRE) ? "" : "x");
			fprintf(stderr,
				"cgck lab: wait %.1f ms for seq %u (n %u, W %u): bseq %u bdone %u breq %#llx %#llx "
				"slots %p %p done/alive%s\n",
				(now_s() - t0) * 1e3, seq, n, W, c->srv.seq, c->srv.done, (unsigned long long)c->srv.req[0],
				(unsigned long long)c->srv.req[1], (void *)c->srv.slot[0], (void *)c->srv.slot[1], dw);
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
				if (!burst_served(b, k, seq))
					at += snprintf(miss + at, sizeof(miss) - at, " %u:%u", k,
						       __atomic_load_n(&b->done[k], __ATOMIC_ACQUIRE));
			miss[at] = 0;
			(void)burst_drain(c);
			uint64_t relay[3] = {0, 0, 0};
			(void)hipMemcpy(relay, c->srv.relay, sizeof(relay), hipMemcpyDeviceToHost);
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

void cgck::burst_hold(cgck_ctx *c, BurstPending *p) { c->srv.slot[p->seq & 1] = p; }

// Collect a posted request: wait for it and copy its outputs where its
// poster asked; frees its slot.
int cgck::burst_collect(cgck_ctx *c, BurstPending *p)
{
	if (!p->seq)
		return p->rc;
	const uint32_t seq = p->seq;
	p->seq = 0;
	if (c->srv.slot[seq & 1] == p)
		c->srv.slot[seq & 1] = nullptr;
	// The GPU wrote the done words and the response, so none of their lines
	// is in this core's caches: a posted request is usually served by now,
	// so start those misses together instead of one after the other.
	{
		const uint8_t *o = burst_resp(c, seq);
		__builtin_prefetch(&c->srv.box->done[0]);
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
	const uint32_t W = burst_wgs(p->n, c->srv.wgs, c->srv.per_wg);
	for (uint32_t j = 0; j < W; j++)
		if (!burst_served(c->srv.box, j, p->seq)) {
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
BurstBlock cgck::burst_next_block(cgck_ctx *c, const BurstLayout &L, bool posted)
{
	const uint32_t seq = burst_next(c->srv.seq);
	if (BurstPending *p = c->srv.slot[seq & 1])
		(void)burst_collect(c, p); // its poster reads p->rc
	const BurstServer &s = c->srv;
	const bool vram = s.vblk && L.bytes <= (posted ? kBurstVramPostedMax : kBurstVramMax) && L.bytes <= kBurstFirst;
	return {vram ? s.vblk + (size_t)(seq & 1) * kBurstFirst : s.stage + (size_t)(seq & 1) * s.stage_cap, vram};
}

// Post the request whose descriptors (and, for base_dev == nullptr, packet
// bytes) are in blk, the next block; returns its seq.
int cgck::burst_post(cgck_ctx *c, BurstBlock blk, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
		     uint32_t max_len, const BurstLayout &L, uint32_t *seq_out, const DescSplit *split)
{
	MapGuard map_g(c);
	BurstBox *b = c->srv.box;
	const uint32_t seq = burst_next(c->srv.seq);
	BurstReq *r = (BurstReq *)blk.p;
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
	c->srv.seq = seq;
#if CGCK_LAB
	t_lab_host[0] = (uint64_t)(now_s() * 1e9);
#endif
	const uint64_t word = (uint64_t)seq | (uint64_t)((uint32_t)n | (blk.vram ? kBurstVram : 0u)) << 32;
	c->srv.req[seq & 1] = word;
	if (c->srv.door) {
		// The block's stores (write-combined device memory, or host memory)
		// are out before the doorbell, and the doorbell leaves the
		// write-combining buffer now rather than at its next eviction.
		__builtin_ia32_sfence();
		__atomic_store_n(&c->srv.door[seq & 1], word, __ATOMIC_RELAXED);
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
int cgck::burst_serve(cgck_ctx *c, BurstBlock blk, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
		      uint32_t max_len, const BurstLayout &L, uint32_t *seq_out)
{
	int rc = burst_post(c, blk, base_dev, range, n, flags, max_len, L, seq_out);
	if (rc)
		return rc;
	return burst_wait(c, *seq_out, (uint32_t)n, range);
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
	const BurstServer &s = c->srv;
	(void)hipStreamDestroy(s.stream);
	for (void *h : {(void *)s.box, (void *)s.stage, (void *)s.resp})
		free_or_park(h, true);
	for (void *d : {(void *)s.scratch, (void *)s.relay, (void *)s.door})
		if (d)
			free_or_park(d, false);
	c->srv = BurstServer{};
}

extern "C" int cgck_burst_open(cgck_ctx_t *c, uint32_t max_pkts, size_t max_bytes, uint32_t idle_ms)
{
	if (!c && !(c = thread_ctx()))
		return -ENODEV; // thread_ctx set the message
	if (c->srv.box)
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
	BurstServer s = {};
	hipError_t e = hipHostMalloc((void **)&s.box, sizeof(BurstBox), hipHostMallocCoherent);
	if (e == hipSuccess)
		e = hipHostMalloc((void **)&s.stage, 2 * cap, hipHostMallocCoherent); // two request slots
	if (e == hipSuccess)
		e = hipHostMalloc((void **)&s.resp, resp_bytes, resp_flags);
	if (e == hipSuccess)
		e = hipMalloc((void **)&s.scratch, cap);
	// the leader's relay (one per slot, then the exit word), uncached: every poll and store
	// goes to memory, whichever XCD's L2 the workgroups sit behind
	if (e == hipSuccess)
		e = hipExtMallocWithFlags((void **)&s.relay, 64, hipDeviceMallocUncached);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer((void **)&s.box_dev, s.box, 0);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer((void **)&s.stage_dev, s.stage, 0);
	if (e == hipSuccess)
		e = hipHostGetDevicePointer((void **)&s.resp_dev, s.resp, 0);
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
		e = burst_stream(c, &s.stream);
	if (e != hipSuccess) {
		for (void *h : {(void *)s.box, (void *)s.stage, (void *)s.resp})
			if (h)
				(void)hipHostFree(h);
		for (void *d : {(void *)s.scratch, (void *)s.relay, vd})
			if (d)
				(void)hipFree(d);
		return set_err(-EIO, "cgck_burst_open: %s", hipGetErrorString(e));
	}
	memset(s.box, 0, sizeof(BurstBox));
	memset(s.stage, 0, 2 * cap);
	s.door = (uint64_t *)vd;
	s.vblk = vd ? (uint8_t *)vd + 64 : nullptr;
	// one workgroup per kBurstPerWG packets of the largest request, at most
	// kBurstMaxWG (and the device's CUs)
	s.per_wg = kBurstPerWG;
	if (const char *e = CGCK_ENV("CGCK_SERVER_PER_WG")) // lab A/B: packets per workgroup
		s.per_wg = atoi(e) > 0 ? (uint32_t)atoi(e) : s.per_wg;
	s.wgs = burst_wgs(max_pkts, kBurstMaxWG, s.per_wg);
	if (s.wgs > (uint32_t)c->num_cus)
		s.wgs = (uint32_t)c->num_cus;
	if (const char *e = CGCK_ENV("CGCK_SERVER_WGS")) // lab A/B: K
		s.wgs = atoi(e) > 0 && atoi(e) <= (int)kBurstMaxWG ? (uint32_t)atoi(e) : s.wgs;
	s.box->idle_ticks = (uint64_t)(idle_ms ? idle_ms : 200) * 100000; // 100 MHz counter
	s.stage_cap = cap;
	s.max_pkts = max_pkts;
	s.max_bytes = max_bytes;
	c->srv = s; // seq, done, slot, busy and req start at zero
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
	if (!c || !c->srv.box || c->srv.slot[0] || c->srv.slot[1])
		return set_err(-EINVAL, "cgck_test_burst_seq: no open server, or a request posted");
	if (seq == 0)
		return set_err(-EINVAL, "cgck_test_burst_seq: seq 0 is never posted");
	BurstServer &s = c->srv;
	MapGuard map_g(c);
	const hipError_t e = burst_drain(c);
	if (e != hipSuccess)
		return set_err(-EIO, "cgck_test_burst_seq: drain: %s", hipGetErrorString(e));
	for (uint32_t j = 0; j < kBurstMaxWG; j++)
		__atomic_store_n(&s.box->done[j], seq, __ATOMIC_RELEASE);
	s.box->req[0] = s.box->req[1] = 0;
	s.req[0] = s.req[1] = 0;
	if (s.door) {
		__atomic_store_n(&s.door[0], 0ull, __ATOMIC_RELAXED);
		__atomic_store_n(&s.door[1], 0ull, __ATOMIC_RELAXED);
		__builtin_ia32_sfence();
	}
	s.box->refused[0] = s.box->refused[1] = 0;
	s.seq = s.done = seq;
	return burst_launch(c, seq);
}

extern "C" int cgck_test_burst_stale(cgck_ctx_t *c, uint32_t from)
{
	if (!c || !c->srv.box || c->srv.slot[0] || c->srv.slot[1])
		return set_err(-EINVAL, "cgck_test_burst_stale: no open server, or a request posted");
	for (uint32_t j = from; j < kBurstMaxWG; j++)
		__atomic_store_n(&c->srv.box->done[j], c->srv.seq + 0x7ffffff0u, __ATOMIC_RELEASE);
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
	if (!c || !c->srv.box || reps <= 0)
		return -EINVAL;
	const volatile uint32_t *w[4] = {&c->srv.box->stop, &c->srv.box->refused[0], &c->srv.box->done[0],
					 (const volatile uint32_t *)&c->srv.box->alive[0]};
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
	if (!c || !c->srv.box)
		return -EINVAL;
	for (int i = 0; i < 4; i++)
		dev[i] = __atomic_load_n(&c->srv.box->lab_t[i], __ATOMIC_ACQUIRE);
	dev[4] = __atomic_load_n(&c->srv.box->lab_cyc, __ATOMIC_ACQUIRE);
	host[0] = t_lab_host[0];
	host[1] = t_lab_host[1];
	return 0;
}

// Lab: thread 0's shader clocks over the last one-workgroup request's body
// call alone (tools/srvlat's body_cycles, against tools/bodylat's).
extern "C" uint64_t cgck_lab_burst_body(cgck_ctx_t *c)
{
	return c && c->srv.box ? __atomic_load_n(&c->srv.box->lab_body, __ATOMIC_ACQUIRE) : 0;
}
#endif

extern "C" int cgck_burst_close(cgck_ctx_t *c)
{
	if (!c)
		c = thread_ctx_if_any(); // this thread's drop-in context, if it exists
	if (!c || !c->srv.box)
		return 0;
	// posted requests complete first: their outputs land where their posters
	// asked (a window still open reads them)
	for (BurstPending *p : {c->srv.slot[0], c->srv.slot[1]})
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
	hipError_t e = CGCK_SYNC(c->srv.stream); // the server sees `stop` within one poll
	burst_release(c);
	free_parked();
	if (e != hipSuccess)
		return set_err(-EIO, "cgck_burst_close: %s", hipGetErrorString(e));
	return 0;
}
