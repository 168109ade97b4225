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
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_zopfli_batch_item<kZBatchItemDicts>(J, T, histo, fast, index, table);
}

// The same behind the one dictionary of the call (br_zopfli_batch_item<kZBatchSharedDict>): a chain replays the call's tree image
// where k_zopfli_batch_dicts resets and prepends; from the stitch on the two are one code.  A third instance, so that the other two
// compile as they did.  Launch shape and workgroup memory are those of k_zopfli_batch.
__global__ __launch_bounds__(64) void k_zopfli_batch_dict(ZopfliBatchJob J, ZopfliTables T) {
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
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_zopfli_batch_item<kZBatchSharedDict>(J, T, histo, fast, index, table);
}

// ---- the tree image of the call's dictionary (lz77_zopfli_dict_image): three launches on the stream, each behind the one in front
// The fill and the class pass move bytes: at most 1 MiB of image and 128 KiB of classes, 16 bytes and one entry per thread and
// step, 64 workgroups of 256 threads -- a few microseconds either way, not worth shaping further.
static constexpr uint32_t kZImageFillGroups = 64, kZImageFillThreads = 256;
__global__ __launch_bounds__(256) void k_zopfli_image_fill(uint32_t* buckets, uint32_t* forest, uint32_t lgwin, uint32_t slots) {
  br_zopfli_image_fill(buckets, forest, lgwin, slots, blockIdx.x * kZImageFillThreads + threadIdx.x, kZImageFillGroups * kZImageFillThreads);
}
__global__ __launch_bounds__(256) void k_zopfli_image_classes(const uint8_t* __restrict__ text, uint32_t end, uint32_t entries, uint16_t* __restrict__ classes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < entries) br_zopfli_image_class_entry(text, end, classes, i);
}
// The store launch: kZImageClasses / 64 = 16 workgroups of ONE wavefront, a class of keys per lane.  Why 16 and one wavefront each:
// a lane's work is a chain of dependent loads (the walk down a tree, then the scan for its next position), so a wavefront is bound
// by latency, not by issue or bandwidth, and the time of the launch is that of its slowest lane -- (stored positions / classes)
// Stores plus one scan of all class entries, the latter the same for every lane whatever the number of classes.  At 64 KiB that is
// 64 Stores beside 4 088 scan steps of 32 bytes: 16 times the lanes of one wavefront already put the Stores below the scan, and more
// classes would shorten only the smaller term while every further lane reads the whole class array again.  One wavefront per
// workgroup lets the dispatcher deal the 16 over as many CUs (two per XCD), each with an L1 of its own for the 128 KiB of
// classes its lanes walk through together; nothing is shared inside a workgroup, so a larger one would only stack them on one CU.
// The workgroups exchange nothing (see br_zopfli_image_store_class): every word has one writer, its only reader.
__global__ __launch_bounds__(64) void k_zopfli_image_store(const uint8_t* __restrict__ text, uint32_t D, uint32_t lgwin, const uint16_t* __restrict__ classes,
                                                           uint32_t* buckets, uint32_t* forest) {
  const uint32_t cls = blockIdx.x * 64u + threadIdx.x;
  if (cls >= kZImageClasses) return;
  const ZopfliParams Z = br_zopfli_image_params(lgwin, D);
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  br_zopfli_image_store_class(z_hasher_of(Z, B), Z, text, classes, zopfli_dict_image_stored(D), cls);
}

void lz77_zopfli_dict_image(const uint8_t* dict, uint32_t D, uint32_t lgwin, uint16_t* classes, uint32_t* buckets, uint32_t* forest) {
  if (lgwin < 10 || lgwin > 24 || D > (1u << lgwin) - 16u) throw std::runtime_error("brotli_mi355x: a dictionary the Zopfli tree image does not take");
  const uint32_t end = zopfli_dict_image_stored(D), entries = zopfli_dict_image_class_entries(D);
  hipLaunchKernelGGL(k_zopfli_image_fill, dim3(kZImageFillGroups), dim3(kZImageFillThreads), 0, BR_STREAM, buckets, forest, lgwin,
                     zopfli_dict_image_slots(D, lgwin));
  HIP_CHECK(hipGetLastError());
  if (end == 0) return;  // (nothing is stored: the image is the empty hasher)
  hipLaunchKernelGGL(k_zopfli_image_classes, dim3((entries + 255) / 256), dim3(256), 0, BR_STREAM, dict, end, entries, classes);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_zopfli_image_store, dim3(kZImageClasses / 64), dim3(64), 0, BR_STREAM, dict, D, lgwin, classes, buckets, forest);
  HIP_CHECK(hipGetLastError());
}

static void zopfli_batch_launch(const ZopfliBatchJob& J, int dict) {
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
  if (dict == kZBatchSharedDict)
    hipLaunchKernelGGL(k_zopfli_batch_dict, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  else if (dict == kZBatchItemDicts)
    hipLaunchKernelGGL(k_zopfli_batch_dicts, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  else
    hipLaunchKernelGGL(k_zopfli_batch, dim3(grid), dim3(64), 0, BR_STREAM, J, T);
  HIP_CHECK(hipGetLastError());
}

void lz77_zopfli_batch_parse(const ZopfliBatchJob& J) { zopfli_batch_launch(J, kZBatchNoDict); }

void lz77_zopfli_batch_parse_dicts(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its dictionary sizes");
  zopfli_batch_launch(J, kZBatchItemDicts);
}

void lz77_zopfli_batch_parse_dict(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && (J.image_buckets == nullptr || J.image_forest == nullptr || J.dict_bytes < 2))
    throw std::runtime_error("brotli_mi355x: a shared-dictionary batch group without its tree image");
  zopfli_batch_launch(J, kZBatchSharedDict);
}

}  // namespace brotli_mi355x
