// cgck_host.h — host-side internals shared by cgck_api.cpp (contexts,
// batches, rings, RSS, plumbing), cgck_burst.cpp (the burst server) and
// cgck_dropin.cpp (the drop-in symbols and the per-thread RX / TX windows).
// Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "cgck_burst.h"
#include "cgck_internal.h"

struct cgck_ctx {
	int device;
	int num_cus;
	hipStream_t stream;
	uint32_t desc_len_hint;
	uint32_t desc_layout; // CGCK_LAYOUT_*
	int family; // enum Family (cgck_params.h), in the lab build with the kNT.. bits ($CGCK_KERNEL)
	const char *last_kernel; // cgck_ctx_last_kernel
	// pinned host staging (drop-in calls, deferred TX)
	uint8_t *h_stage;
	size_t h_stage_cap;
	uint32_t *h_out;
	size_t h_out_cap;
	// device scratch (host-resident batches)
	uint8_t *d_bytes;
	size_t d_bytes_cap;
	uint8_t *d_aux; // descriptors | out | verdict
	size_t d_aux_cap;
	void *d_zero; // kZeroBytes zero bytes (KParams.zero)
	// Toeplitz byte tables of the last key used (cgck_rss.hip)
	uint32_t *d_rss_tab;
	size_t d_rss_tab_cap;
	uint32_t *h_rss_tab; // host copy (malloc)
	size_t h_rss_tab_cap;
	uint8_t *rss_key; // the key the tables were built from (malloc)
	int rss_key_len;
	uint32_t rss_cnt;
	bool rss_valid;
	void *rss_users; // RssUsers (cgck_api.cpp): one event per stream that read d_rss_tab
	// dst-cache scratch: control words + look-back status (zeroed per launch)
	uint8_t *d_dst;
	size_t d_dst_cap;
	cgck::BurstServer srv; // the burst server (cgck_burst.h)
};

// Library-internal: hidden, so calls between the library's own files are
// direct (no PLT hop on the drop-in symbols' per-call path, e.g. reg_find).
#pragma GCC visibility push(hidden)
namespace cgck {

// hipStreamSynchronize; the lab build reports a synchronisation that takes
// more than 20 ms, with where it was called (a loop stall's diagnosis).
#if CGCK_LAB
hipError_t lab_sync(const char *where, hipStream_t st);
#define CGCK_STR2(x) #x
#define CGCK_STR(x) CGCK_STR2(x)
#define CGCK_SYNC(st) ::cgck::lab_sync(__FILE__ ":" CGCK_STR(__LINE__), st)
#else
#define CGCK_SYNC(st) hipStreamSynchronize(st)
#endif

// Thread-local error text (cgck_last_error); returns `code`.
int set_err(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *err_text();

#define HIP_TRY(expr)                                                                     \
	do {                                                                              \
		hipError_t e_ = (expr);                                                   \
		if (e_ != hipSuccess)                                                     \
			return ::cgck::set_err(-EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

int grow_host(void **p, size_t *cap, size_t need);
int grow_dev(void **p, size_t *cap, size_t need);

// One checksum launch on the context (KParams.zero filled in); records the
// kernel's name in c->last_kernel.
int run(cgck_ctx *c, const KParams &p, uint32_t len_hint, hipStream_t st);

// cgck_desc_host without the public flag check (internal flags allowed).
// meta: kFlagRx's per-packet words (nullptr otherwise).
int desc_host(cgck_ctx *c, void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
	      uint32_t *out, uint8_t *verdict, uint32_t *meta = nullptr);
// The same, left posted when the burst server takes it: returns 1 and *pend
// records the request (burst_collect waits for it and copies its outputs to
// out / verdict / meta, which must stay valid until then); 0 when it was
// computed at once (no server, or it does not fit); a negative errno.  A
// later request on the context that needs the slot collects it first.
// sum (optional): the longest ip_len and the 16-byte-rounded packet bytes of
// descriptors the library built itself inside [base, base + bytes), so the
// per-descriptor check is skipped.
struct DescSummary {
	uint32_t max_len;
	size_t pkt_bytes;
};
// A request in two parts: descriptors [n1, n) take flags2 (BurstReq.n1).
struct DescSplit {
	uint32_t n1, flags2;
};
int desc_host_post(cgck_ctx *c, void *base, size_t bytes, const cgck_desc_t *desc, uint64_t n, uint32_t flags,
		   uint32_t *out, uint8_t *verdict, uint32_t *meta, BurstPending *pend,
		   const DescSummary *sum = nullptr, const DescSplit *split = nullptr);

// Staging path of one region for the drop-in symbols (burst server when open,
// else a launch on the context stream and a synchronisation).
int one_region(cgck_ctx *c, const void *src, uint32_t span, uint32_t ip_len, uint32_t flags, uint32_t *out);

// A range registered with cgck_host_register: [lo, hi) and the device
// pointer of lo.
struct RegRange {
	uint8_t *lo, *hi;
	uint8_t *dev;
};
// Is [p, p + bytes) inside one registered range?  Fills *r when it is.
bool reg_find(const void *p, size_t bytes, RegRange *r);
// Bumped by every cgck_host_register / _unregister: a range found under one
// value stays valid while the value holds (the drop-ins' per-thread cache).
extern std::atomic<uint64_t> g_reg_gen;

// The calling thread's drop-in context (created on first use); nullptr with
// the error text set when no gfx950 device can be used.
cgck_ctx *thread_ctx();
cgck_ctx *thread_ctx_if_any(); // the context if this thread made one, else nullptr
// Report a failure of a call that has no error channel (the drop-in
// symbols): the handler of cgck_set_error_handler, then abort.
[[noreturn]] void die(const char *what);

int rss_prepare(cgck_ctx *c, const uint8_t *key, int key_size, uint32_t cnt, hipStream_t st);
int rss_note_use(cgck_ctx *c, hipStream_t st);
constexpr uint32_t kRssMaxCnt = 65536;

} // namespace cgck
#pragma GCC visibility pop
