// cgck_steer_plan.h — the geometry of cgck_steer (include/cgck.h, section 3;
// cgck_steer.hip), as a pure function of (n, queue_num): tests read it through
// cgck_test_steer_plan without a device, the launcher and cgck_steer_work_bytes
// through steer_plan().
#pragma once
#include <cstddef>
#include <cstdint>

namespace cgck {

constexpr uint32_t kSteerThreads = 256;             // count / scatter / one-launch workgroup: 4 waves
constexpr uint32_t kSteerWaves = kSteerThreads / 64;
constexpr uint32_t kSteerStep = kSteerThreads;      // a tile is a multiple of the workgroup's wave-steps (4 x 64 frames)
constexpr uint32_t kSteerBaseTile = 4096;           // 16 wave-steps per wave; every receive burst is one tile
constexpr uint32_t kSteerMaxQueues = 128;           // RSS_QUEUE_ID_MAX
constexpr uint32_t kSteerMaxBins = kSteerMaxQueues + 1; // the queues and the unsteered bin
constexpr uint32_t kSteerScanThreads = 1024;        // the scan workgroup
constexpr uint32_t kSteerScanPer = 4;               // words per thread and pass
constexpr uint32_t kSteerScanPass = kSteerScanThreads * kSteerScanPer; // words per pass
constexpr uint64_t kSteerBudget = 64 * (uint64_t)kSteerScanPass;       // tiles x bins: at most 64 scan passes (1 MiB)

struct SteerPlan {
	uint32_t tile;     // frames per workgroup pass
	uint32_t tiles;    // ceil(n / tile)
	size_t work_bytes; // room for u32 hist[queue_num + 1][tiles]; 0 when one launch serves the call
};

// queue_num in 1..128 and n <= 0xFFFFFFFF (the callers check).  The tile doubles
// from kSteerBaseTile until tiles x (queue_num + 1) fits kSteerBudget.
SteerPlan steer_plan(uint64_t n, uint32_t queue_num);

} // namespace cgck
