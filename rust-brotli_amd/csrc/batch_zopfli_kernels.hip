// batch_zopfli_kernels.hip -- the gfx950 kernel of batch_zopfli.h: the small items of a batch at quality 11, one
// sequential Zopfli walk each (batch_zopfli_device.h over zopfli_device.h).
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "batch_zopfli_device.h"
#include "device_api.h"
#include "device_scan.h"

namespace brotli_mi355x {

// One wavefront per table, persistent over the group like k_quick_batch: it takes the next place of `order` (largest item first)
// from the device counter until none is left, and empties its hasher in front of every item.  All lanes run the sequential
// programme with identical scalar state; they differ where a position's candidates and the lengths of a copy are spread over them
// (z_update_nodes).  Workgroup memory as in k_zopfli_parse -- the node window, the literal-cost window, the cost tables and the
// queue, 104 KiB -- so one workgroup per CU: a walk is bound by the latency of its own dependent loads, and the throughput of
// the launch is the number of CUs.
__global__ __launch_bounds__(64) void k_zopfli_batch(ZopfliBatchJob J, ZopfliTables T) {
  __shared__ ZNode window[kZWin];   // (ZNodeView)
  __shared__ float lc_window[kZWin];
  __shared__ float cost_cmd[704], cost_dist[1200];  // (ZCostModel: every length of every candidate looks one of each up)
  __shared__ ZQueue queue;          // (indexed dynamically: in registers it would live in scratch memory)
  __shared__ uint32_t histo[256];   // should_compress
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  ZFast fast;
  fast.window = window;
  fast.lc_window = lc_window;
  fast.cost_cmd = cost_cmd;
  fast.cost_dist = J.dist_alphabet_size <= 1136 ? cost_dist : (float*)nullptr;
  fast.queue = &queue;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_zopfli_batch_item(J, T, histo, fast, index, table);
}

// The same behind a dictionary per item (br_zopfli_batch_item<true>): an instance of its own, so that k_zopfli_batch carries none
// of the dictionary steps.  Launch shape and workgroup memory are those of k_zopfli_batch.
__global__ __launch_bounds__(64) void k_zopfli_batch_dicts(ZopfliBatchJob J, ZopfliTables T) {
  __shared__ ZNode window[kZWin];
  __shared__ float lc_window[kZWin];
  __shared__ float cost_cmd[704], cost_dist[1200];
  __shared__ ZQueue queue;
  __shared__ uint32_t histo[256];
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  ZFast fast;
  fast.window = window;
  fast.lc_window = lc_window;
  fast.cost_cmd = cost_cmd;
  fast.cost_dist = J.dist_alphabet_size <= 1136 ? cost_dist : (float*)nullptr;
  fast.queue = &queue;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_zopfli_batch_item<true>(J, T, histo, fast, index, table);
}

static void zopfli_batch_launch(const ZopfliBatchJob& J, bool dicts) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  const DeviceTables& dt = dev_tables();
  ZopfliTables T;
  T.lut_buckets = dt.dict_lut_buckets;
  T.lut_words = dt.dict_lut_words;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  T.dict_size_bits_by_length = dt.dict_size_bits_by_length;
  T.logs.logs_16 = dt.logs_16;
  T.logs.logs_8 = dt.logs_8;
  const uint32_t grid = J.tables < J.n_items ? J.tables : J.n_items;
  if (dicts)
    hipLaunchKernelGGL(k_zopfli_batch_dicts, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  else
    hipLaunchKernelGGL(k_zopfli_batch, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  HIP_CHECK(hipGetLastError());
}

void lz77_zopfli_batch_parse(const ZopfliBatchJob& J) { zopfli_batch_launch(J, false); }

void lz77_zopfli_batch_parse_dicts(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its dictionary sizes");
  zopfli_batch_launch(J, true);
}

}  // namespace brotli_mi355x
