// encode_workspace.h -- workspaces of the encode side of hip_abi.hip as one carve each (workspace_carve.h): over NULL it gives
// the bytes the call allocates, over the allocation the pointers of the launch. So far the viz tables; the encode call's zero
// block, d_finrec and the batch-shape staging buffer are still laid out by hand in hip_abi.hip. `Cloud` and `Block` are VizCloud
// and VizBlock: parameters because a plain compiler cannot take stage1_launch.h, and tests/test_workspace_carve.py checks the
// layout without a device. Host only.
#pragma once

#include "stage1_device.h"
#include "workspace_carve.h"

namespace cldn {

// h_viz of the viz pre-filter: [clouds | blocks | kept counts]. d_viz_tables is a copy of the first *device_bytes of it: the
// same carve over d_viz_tables.p gives VizLaunch::clouds and ::blocks (the kept counts would lie behind that allocation).
template <class Cloud, class Block>
size_t carve_viz_tables(void* base, uint32_t n_clouds, uint32_t n_blocks, Cloud** clouds, Block** blocks, size_t* device_bytes,
                        uint64_t** kept = nullptr) {
  Carve ws(base);
  *clouds = ws.take<Cloud>(n_clouds);
  *blocks = ws.take<Block>(n_blocks, 64);
  uint64_t* const k = ws.take<uint64_t>((size_t)n_clouds + 1u, 64);  // survivors per cloud, total
  if (kept) *kept = k;
  *device_bytes = ws.bytes() - ((size_t)n_clouds + 1u) * sizeof(uint64_t);
  return ws.bytes();
}

}  // namespace cldn
