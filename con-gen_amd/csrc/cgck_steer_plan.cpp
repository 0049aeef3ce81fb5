// cgck_steer_plan.cpp — steer_plan() and its two C entry points (no device, no
// context): cgck_steer_work_bytes and the test hook cgck_test_steer_plan.
#include "cgck_steer_plan.h"

namespace cgck {

static_assert(kSteerBaseTile % kSteerStep == 0, "a tile is whole wave-steps of the workgroup");

SteerPlan steer_plan(uint64_t n, uint32_t queue_num)
{
	const uint64_t bins = (uint64_t)queue_num + 1;
	uint64_t tile = kSteerBaseTile;
	while (((n + tile - 1) / tile) * bins > kSteerBudget)
		tile *= 2;
	const uint64_t tiles = (n + tile - 1) / tile;
	SteerPlan p;
	p.tile = (uint32_t)tile;
	p.tiles = (uint32_t)tiles;
	// Past the base tile the product tiles x bins falls back to half the budget
	// at every doubling; the whole budget is asked for there, so that the bytes
	// never shrink as n grows.
	p.work_bytes = tiles <= 1 ? 0 : (size_t)(tile == kSteerBaseTile ? tiles * bins : kSteerBudget) * 4;
	return p;
}

} // namespace cgck

static bool steer_plan_args(uint64_t n, uint32_t queue_num)
{
	return queue_num >= 1 && queue_num <= cgck::kSteerMaxQueues && n <= 0xFFFFFFFFull;
}

extern "C" size_t cgck_steer_work_bytes(uint64_t n, uint32_t queue_num)
{
	return steer_plan_args(n, queue_num) ? cgck::steer_plan(n, queue_num).work_bytes : 0;
}

extern "C" int cgck_test_steer_plan(uint64_t n, uint32_t queue_num, uint32_t *tile, uint32_t *tiles,
				    size_t *work_bytes)
{
	if (!steer_plan_args(n, queue_num))
		return -22; // -EINVAL
	const cgck::SteerPlan p = cgck::steer_plan(n, queue_num);
	if (tile)
		*tile = p.tile;
	if (tiles)
		*tiles = p.tiles;
	if (work_bytes)
		*work_bytes = p.work_bytes;
	return 0;
}
