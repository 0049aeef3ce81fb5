// cgck_burst.h — host side of the resident burst server (cgck_burst.cpp): a
// context's server state and what the server's clients call (cgck_api.cpp's
// host-resident batches and mapping changes, cgck_dropin.cpp's windows).
// Part of cgck_host.h.  Not part of the C-ABI.
#pragma once
#include <mutex>

#include "cgck_internal.h"

struct cgck_ctx;

namespace cgck {
// A request left posted on the burst server (desc_host_post): where its
// outputs go when it is collected (burst_collect) and its result.
struct BurstPending {
	uint32_t seq; // 0: not pending
	uint32_t n;
	uint64_t range;
	uint32_t *out, *meta;
	uint8_t *verdict;
	int rc;
};

// burst server (cgck_burst_open): mailbox, request block and outputs in
// host-coherent pinned memory, the block's device copy in scratch
struct BurstServer {
	BurstBox *box;   // nullptr: closed
	uint8_t *stage;  // request block: [BurstReq | descriptors | packet bytes]
	size_t stage_cap;
	uint8_t *stage_dev; // device view of stage
	BurstBox *box_dev;  // device view of box
	uint8_t *resp;      // a request's outputs, packed by its n (burst_meta_off / burst_ver_off)
	uint8_t *resp_dev;
	uint8_t *scratch;   // device: the server's copy of the block (stage_cap bytes)
	uint64_t *relay;    // device, uncached: the leader's relay word
	uint32_t max_pkts;  // packets per request
	size_t max_bytes;   // packet bytes per request (cgck_burst_open's max_bytes)
	uint32_t wgs;       // workgroups of the server (K)
	uint32_t per_wg;    // packets per workgroup of a wide request
	uint32_t seq;       // the last request posted
	uint32_t done;      // the last request known complete (a relaunch serves the ones after it)
	BurstPending *slot[2]; // a posted request not yet collected, per slot
	uint32_t busy;      // the owner thread is inside a request (MapGuard, cgck_burst.cpp)
	// device memory the host writes through the large BAR (nullptr: none, the
	// mailbox words are box->req): the two mailbox words the leader polls,
	// then two kBurstFirst request slots for small blocks
	uint64_t *door;
	uint8_t *vblk;
	uint64_t req[2];    // the last mailbox word posted per slot (host copy)
	hipStream_t stream; // the server's own stream (it stays resident)
};

#pragma GCC visibility push(hidden)
struct DescSplit; // cgck_host.h

extern const size_t kServerCopy; // burst_in_place's server_copy
bool burst_fits(const cgck_ctx *c, uint64_t n, size_t staged, size_t data);
// The block of the next request, and whether it is a device-memory slot.
struct BurstBlock { uint8_t *p; bool vram; };
BurstBlock burst_next_block(cgck_ctx *c, const BurstLayout &L, bool posted = false);
int burst_post(cgck_ctx *c, BurstBlock blk, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
	       uint32_t max_len, const BurstLayout &L, uint32_t *seq_out, const DescSplit *split = nullptr);
int burst_serve(cgck_ctx *c, BurstBlock blk, const uint8_t *base_dev, uint64_t range, uint64_t n, uint32_t flags,
		uint32_t max_len, const BurstLayout &L, uint32_t *seq_out);
const uint8_t *burst_resp(const cgck_ctx *c, uint32_t seq);
// The posted request *p stays in its slot until it is collected.
void burst_hold(cgck_ctx *c, BurstPending *p);
int burst_collect(cgck_ctx *c, BurstPending *pend);
// Without waiting: is the posted request's every slice served (1), or not
// yet (0)?  A request that was computed at once (seq 0) is ready.
int burst_ready(cgck_ctx *c, const BurstPending *pend);

// A change of the host mappings (cgck_host_register / _unregister): while one
// lives no server request is in flight on the host side and no server runs.
class MapChange {
      public:
	MapChange();
	~MapChange();
	MapChange(const MapChange &) = delete;
	MapChange &operator=(const MapChange &) = delete;

      private:
	std::lock_guard<std::mutex> lk_;
};

// hipFree / hipHostFree, or parked while any server is resident.
void free_or_park(void *p, bool host);
#pragma GCC visibility pop

} // namespace cgck
