// quick_kernels.hip -- gfx950 kernels of qualities 2..4 (quick_api.h, quick_device.h): the BasicHasher family under the
// greedy / lazy parse, one wavefront per stream walking the reference's own hash table block by block.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "batch_quick_device.h"
#include "quick_device.h"
#include "device_scan.h"

namespace brotli_mi355x {

static QuickTables quick_tables() {
  const DeviceTables& dt = dev_tables();
  QuickTables T;
  T.dict_hash = dt.dict_hash;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  return T;
}

__global__ __launch_bounds__(256) void k_quick_fill(uint32_t* __restrict__ p, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}
void lz77_quick_init(const QuickJob& J) {
  hipLaunchKernelGGL(k_quick_fill, dim3(256), dim3(256), 0, BR_STREAM, J.table, quick_table_words(J));
  HIP_CHECK(hipGetLastError());
}

// slots: positions moved down by delta (0 where they fall in front of the new text); books: as they are
__global__ __launch_bounds__(256) void k_quick_import(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t slots, uint32_t words, uint32_t delta) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) {
    const uint32_t v = src[i];
    dst[i] = i < slots ? (v >= delta ? v - delta : 0u) : v;
  }
}
void lz77_quick_import(const QuickJob& J, const uint32_t* table_src, uint32_t delta) {
  hipLaunchKernelGGL(k_quick_import, dim3(256), dim3(256), 0, BR_STREAM, J.table, table_src, quick_slots(J), quick_table_words(J), delta);
  HIP_CHECK(hipGetLastError());
}

// HasherPrependCustomDictionary files the dictionary positions in ascending order into a table that holds nothing else yet
// (lz77_quick_init comes first): what a slot ends up with is the LARGEST position filed under it -- one thread per position and
// an atomic maximum give the table of the sequential loop (br_quick_prepend, which the emulation runs).  A shard of
// BrotliEncoderCompressMulti is primed with up to a window of text in front of it, several times its own size.
__global__ __launch_bounds__(256) void k_quick_prepend(QuickJob J, const uint8_t* __restrict__ text, uint32_t count) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint64_t v = (br_load64(text + i) << (64u - 8u * J.hash_len)) * kQuickHashMul64;
    const uint32_t key = (uint32_t)(v >> (64u - J.bucket_bits));
    atomicMax(J.table + key + ((i >> 3) & (J.sweep - 1u)), i);
  }
}
void lz77_quick_prepend(const Lz77Params& P, const Lz77Buffers& B, const QuickJob& J, uint32_t dict_bytes) {
  if (dict_bytes <= kQuickHtl - 1u) return;
  const uint32_t count = dict_bytes - (kQuickHtl - 1u);
  const uint32_t blocks = (count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096;
  hipLaunchKernelGGL(k_quick_prepend, dim3(blocks), dim3(256), 0, BR_STREAM, J, (const uint8_t*)B.text, count);
  HIP_CHECK(hipGetLastError());
}

// One wavefront per stream: all lanes run the sequential parse with identical scalar state (lane 0 writes).
__global__ __launch_bounds__(64) void k_quick_block(QuickJob J, Lz77Params P, QuickTables T, const uint8_t* __restrict__ text, const Segment* __restrict__ segments,
                                                    const SegEntry* __restrict__ entries, Command* __restrict__ cmds, SegExit* __restrict__ exits, uint32_t block) {
  if (blockIdx.x != 0) return;
  const Segment seg = segments[block];
  br_quick_block(J, P, T, text, seg, entries[block], cmds + seg.cmd_base, exits + block);
}
void lz77_quick_block(const Lz77Params& P, const Lz77Buffers& B, const QuickJob& J, uint32_t block) {
  hipLaunchKernelGGL(k_quick_block, dim3(1), dim3(64), 0, BR_STREAM, J, P, quick_tables(), (const uint8_t*)B.text, (const Segment*)B.segments, (const SegEntry*)B.entries, B.cmds,
                     B.exits, block);
  HIP_CHECK(hipGetLastError());
}

// ---- batch_quick.h: the small items of a batch at these qualities, one chain each.  One wavefront per table, persistent over
// the group like k_parse_batch: it takes the next place of `order` (largest item first) from the device counter until none is
// left, and zeroes its table in front of every item.  A chain is bound by the latency of its own dependent loads; the
// throughput of the launch is the number of chains in flight.
__global__ __launch_bounds__(64) void k_quick_batch(QuickBatchJob J, QuickTables T, EntropyTables logs) {
  __shared__ uint32_t histo[256];
  __shared__ SegExit exit_slot;
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_quick_batch_item<false>(J, T, logs, histo, &exit_slot, index, table);
}

// The same launch for items behind a shared custom dictionary (J.dict_bytes, J.image): a chain copies the call's table image over
// its table where the one above zeroes it.  (Two kernels, not two instances of a template: the compiler cuts the exit slot of a
// plain kernel down to the fields that are read, and leaves the one of a template instance whole.)
__global__ __launch_bounds__(64) void k_quick_batch_dict(QuickBatchJob J, QuickTables T, EntropyTables logs) {
  __shared__ uint32_t histo[256];
  __shared__ SegExit exit_slot;
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_quick_batch_item<true>(J, T, logs, histo, &exit_slot, index, table);
}

// The same launch for items behind a custom dictionary each (J.item_dict_bytes): a chain zeroes its table and files its item's
// dictionary itself, 64 positions per step (br_quick_batch_file), or copies the image the group has built of that dictionary
// (J.images, J.item_image: k_quick_dict_images below).  (A kernel of its own for the reason above.)
__global__ __launch_bounds__(64) void k_quick_batch_dicts(QuickBatchJob J, QuickTables T, EntropyTables logs) {
  __shared__ uint32_t histo[256];
  __shared__ SegExit exit_slot;
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_quick_batch_item<true, true>(J, T, logs, histo, &exit_slot, index, table);
}

// The table images of a group behind a dictionary per item (batch_quick.h: lz77_quick_dict_images), all in one launch: blockIdx.y
// is the image, the threads of its row file the dictionary's positions with the atomic maximum of k_quick_prepend into a table
// the caller has zeroed.  Every 8-byte load ends inside the dictionary's copy: count = D - 7 positions.
__global__ __launch_bounds__(256) void k_quick_dict_images(QuickJob J, const uint8_t* __restrict__ text, uint32_t n_images,
                                                            const uint32_t* __restrict__ text_at, const uint32_t* __restrict__ dict_bytes,
                                                            uint32_t* __restrict__ images) {
  const uint32_t image = blockIdx.y;
  if (image >= n_images) return;
  const uint32_t D = dict_bytes[image];
  if (D <= kQuickHtl - 1u) return;
  const uint32_t count = D - (kQuickHtl - 1u);
  const uint8_t* __restrict__ dict = text + text_at[image];
  uint32_t* __restrict__ table = images + (size_t)image * quick_table_words(J);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint64_t v = (br_load64(dict + i) << (64u - 8u * J.hash_len)) * kQuickHashMul64;
    const uint32_t key = (uint32_t)(v >> (64u - J.bucket_bits));
    atomicMax(table + key + ((i >> 3) & (J.sweep - 1u)), i);
  }
}
void lz77_quick_dict_images(const QuickJob& Q, const uint8_t* text, uint32_t n_images, const uint32_t* text_at_dev, const uint32_t* dict_bytes_dev,
                            uint32_t* images) {
  if (n_images == 0) return;
  // (a dictionary has at most 65536 bytes: 64 blocks of 256 threads file four positions each at the most)
  hipLaunchKernelGGL(k_quick_dict_images, dim3(64, n_images), dim3(256), 0, BR_STREAM, Q, text, n_images, text_at_dev, dict_bytes_dev, images);
  HIP_CHECK(hipGetLastError());
}

// Items of two to kBatchLongBlocks input blocks (batch_quick.h): the launch shape of k_quick_batch, the item code walks from
// block to block and leaves one BatchLongRecord per item.
__global__ __launch_bounds__(64) void k_quick_batch_long(QuickBatchJob J, BatchLongRecord* __restrict__ records, QuickTables T, EntropyTables logs) {
  __shared__ uint32_t histo[256];
  __shared__ SegExit exit_slot;
  const uint32_t table = blockIdx.x;
  if (table >= J.tables) return;
  for (uint32_t index; br_batch_next_index(J.counter, J.order, J.n_items, index);) br_quick_batch_item_long(J, records, T, logs, histo, &exit_slot, index, table);
}

static EntropyTables entropy_tables() {
  const DeviceTables& dt = dev_tables();
  EntropyTables logs;
  logs.logs_16 = dt.logs_16;
  logs.logs_8 = dt.logs_8;
  return logs;
}
// one wavefront per table, none without an item; 0: an empty group, nothing to launch
static uint32_t quick_batch_grid(const QuickBatchJob& J) {
  if (J.n_items == 0) return 0;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  return J.tables < J.n_items ? J.tables : J.n_items;
}

void lz77_quick_batch_parse(const QuickBatchJob& J) {
  const uint32_t grid = quick_batch_grid(J);
  if (grid == 0) return;
  hipLaunchKernelGGL(k_quick_batch, dim3(grid), dim3(64), 0, BR_STREAM, J, quick_tables(), entropy_tables());
  HIP_CHECK(hipGetLastError());
}

void lz77_quick_batch_parse_dict(const QuickBatchJob& J) {
  const uint32_t grid = quick_batch_grid(J);
  if (grid == 0) return;
  if (J.dict_bytes == 0 || J.image == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its table image");
  hipLaunchKernelGGL(k_quick_batch_dict, dim3(grid), dim3(64), 0, BR_STREAM, J, quick_tables(), entropy_tables());
  HIP_CHECK(hipGetLastError());
}

void lz77_quick_batch_parse_dicts(const QuickBatchJob& J) {
  const uint32_t grid = quick_batch_grid(J);
  if (grid == 0) return;
  if (J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a batch group with a dictionary per item without their sizes");
  hipLaunchKernelGGL(k_quick_batch_dicts, dim3(grid), dim3(64), 0, BR_STREAM, J, quick_tables(), entropy_tables());
  HIP_CHECK(hipGetLastError());
}

void lz77_quick_batch_parse_long(const QuickBatchJob& J, BatchLongRecord* records) {
  const uint32_t grid = quick_batch_grid(J);
  if (grid == 0) return;
  hipLaunchKernelGGL(k_quick_batch_long, dim3(grid), dim3(64), 0, BR_STREAM, J, records, quick_tables(), entropy_tables());
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
