// batch_q9_kernels.hip -- the gfx950 kernels of BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS and BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS
// (batch_greedy.h): the items of a batch at qualities 9 and 10, one live chain each on a private H9 table (br_batch_item_h9,
// batch_greedy_device.h), and the items of quality 9 behind a custom dictionary (br_batch_item_h9_dict, batch_q9_device.h).  A
// translation unit of its own, so that the parse kernels of lz77_kernels.hip compile as they did.
#include <hip/hip_runtime.h>

#include <stdexcept>

#undef BR_CHAIN_PROFILE  // (the profiling build: the chain's cycle counters are a device variable of lz77_kernels.hip, not linked across units)
#include "batch_greedy_device.h"
#include "batch_q9_device.h"
#include "device_api.h"
#include "device_scan.h"  // HIP_CHECK

namespace brotli_mi355x {

// One wavefront per table, persistent over the group like k_parse_batch: it takes the next place of `order` (largest item first)
// from the device counter until none is left, and empties the counters of its table in front of every item.  The chain is bound by
// the latency of its own dependent loads -- ring counters, up to 2 x 256 ring entries, the text behind every entry in reach -- and a
// table is 32 MiB, so every ring is a miss of the L2: the throughput of the launch is the number of chains in flight, 255 within
// the 8 GiB the tables of a group may take, one wavefront per CU.  Workgroup memory: the scratch of an H9 chain (the candidates of
// two positions, 2 x 274) and the 256 histogram words of should_compress.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_parse_batch_h9(BatchParseJob J, ChainTables T) {
  __shared__ ChainScratchT<true, false> scratch;
  __shared__ uint32_t histo[256];
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_batch_item_h9(J, T, scratch, histo, index, table);
}

// The same launch shape, workgroup memory and occupancy bounds behind a custom dictionary: siblings of k_parse_batch_h9, so that
// the instance without a dictionary compiles as it did.  k_parse_batch_h9_dict: the call's shared dictionary (J.dict: its image is
// replayed over the table, or filed by the chain where there is no image); k_parse_batch_h9_dicts: a dictionary per item
// (J.item_dict_bytes), filed by the chain or, where the group has built an image of it (J.images, J.item_image), replayed.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_parse_batch_h9_dict(BatchParseJob J, ChainTables T) {
  __shared__ ChainScratchT<true, false> scratch;
  __shared__ uint32_t histo[256];
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_batch_item_h9_dict<false>(J, T, scratch, histo, index, table);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_parse_batch_h9_dicts(BatchParseJob J, ChainTables T) {
  __shared__ ChainScratchT<true, false> scratch;
  __shared__ uint32_t histo[256];
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_batch_item_h9_dict<true>(J, T, scratch, histo, index, table);
}

void lz77_batch_parse_h9(const BatchParseJob& J) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  // (what the scratch and the table layout are sized for)
  if (J.P.hasher_kind != 9 || J.P.block_bits != 8 || J.P.ndist > 16) throw std::runtime_error("brotli_mi355x: not the job of an H9 batch chain");
  // (what batch_q9_device.h argues from: dictionary + item end inside the first half of the smallest ring buffer, 1 << 18)
  if (J.dict.bytes > 65536 || (J.dict.bytes != 0 && J.item_dict_bytes != nullptr) || J.P.ring_mask < (1u << 18) - 1u)
    throw std::runtime_error("brotli_mi355x: not the job of an H9 batch chain");
  const ChainTables T = batch_chain_tables(J);
  const uint32_t grid = J.tables < J.n_items ? J.tables : J.n_items;
  const auto kernel = J.item_dict_bytes != nullptr ? k_parse_batch_h9_dicts : (J.dict.bytes != 0 ? k_parse_batch_h9_dict : k_parse_batch_h9);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
