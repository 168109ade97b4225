// zopfli_entry_kernels.hip -- the gfx950 kernels behind the introspection entries of zopfli_entry.inc: the static dictionary search,
// the logarithms and the literal / histogram cost model of zopfli_device.h, called on inputs handed in directly.  Nothing of the
// product's own path goes through here.
#include <hip/hip_runtime.h>

#include "batch_zopfli_device.h"
#include "device_api.h"
#include "device_scan.h"
#include "zopfli_device.h"
#include "zopfli_entry_api.h"

namespace brotli_mi355x {

static ZopfliTables zopfli_entry_tables() {
  const DeviceTables& dt = dev_tables();
  ZopfliTables T;
  T.lut_buckets = dt.dict_lut_buckets;
  T.lut_words = dt.dict_lut_words;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  T.dict_size_bits_by_length = dt.dict_size_bits_by_length;
  T.logs.logs_16 = dt.logs_16;
  T.logs.logs_8 = dt.logs_8;
  return T;
}

__global__ __launch_bounds__(64) void k_zdebug_dictionary(ZopfliTables T, const uint8_t* __restrict__ text, uint32_t n_queries,
                                                          const uint32_t* __restrict__ at, const uint32_t* __restrict__ min_length,
                                                          const uint32_t* __restrict__ max_length, uint32_t* __restrict__ matches,
                                                          uint32_t* __restrict__ any) {
  const uint32_t q = blockIdx.x * 64u + threadIdx.x;
  if (q >= n_queries) return;
  uint32_t found[38];  // (as z_find_all_matches holds them)
  for (uint32_t i = 0; i <= 37; ++i) found[i] = kZInvalidMatch;
  any[q] = z_find_all_dictionary_matches(T, text + at[q], min_length[q], max_length[q], found) ? 1u : 0u;
  for (uint32_t i = 0; i <= 37; ++i) matches[(size_t)q * 38 + i] = found[i];
}

__global__ __launch_bounds__(256) void k_zdebug_fast_log2(ZopfliTables T, uint32_t mode, uint32_t n, const unsigned long long* __restrict__ values,
                                                          uint32_t* __restrict__ out_bits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = values[i];
  float r;
  if (mode == 0) r = z_fast_log2(T.logs, v);
  else if (mode == 1) r = br_fast_log2(T.logs, (uint32_t)v);
  else r = T.logs.logs_16[v & 0xffffu];
  out_bits[i] = z_to_bits(r);
}

// All lanes run the sequential cost model with identical state, the cost tables in workgroup memory, as k_zopfli_parse has it.
__global__ __launch_bounds__(64) void k_zdebug_literal_costs(ZopfliTables T, uint32_t n_jobs, const uint32_t* __restrict__ lengths,
                                                             const unsigned long long* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                             uint32_t* histo, float* cost, float* prefix) {
  __shared__ float cost_cmd[704], cost_dist[544];
  const uint32_t j = blockIdx.x;
  if (j >= n_jobs) return;
  const uint32_t len = lengths[j];
  const uint8_t* d = data + offsets[j];
  uint32_t* h = histo + (size_t)j * 768;
  z_literal_costs(T, d, len, h, cost + offsets[j]);
  __syncthreads();
  ZCostModel model;
  model.cost_cmd = cost_cmd;
  model.cost_dist = cost_dist;
  model.literal_costs = prefix + offsets[j] + 2 * (size_t)j;
  model.distance_histogram_size = 544;
  model.min_cost_cmd = 0.0f;
  model.num_bytes = len;
  z_model_from_literal_costs(model, T, d, h);
}

__global__ __launch_bounds__(64) void k_zdebug_cost_from_histogram(ZopfliTables T, uint32_t n_jobs, const uint32_t* __restrict__ sizes,
                                                                   const uint32_t* __restrict__ literal, const unsigned long long* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ histograms, float* __restrict__ cost) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_jobs) return;
  z_set_cost_from_histogram(T, histograms + offsets[j], sizes[j], literal[j] != 0, cost + offsets[j]);
}

void zopfli_debug_dictionary_matches(const uint8_t* text, uint32_t n_queries, const uint32_t* at, const uint32_t* min_length,
                                     const uint32_t* max_length, uint32_t* matches, uint32_t* any) {
  if (n_queries == 0) return;
  hipLaunchKernelGGL(k_zdebug_dictionary, dim3((n_queries + 63) / 64), dim3(64), 0, BR_STREAM, zopfli_entry_tables(), text, n_queries, at, min_length,
                     max_length, matches, any);
  HIP_CHECK(hipGetLastError());
}

void zopfli_debug_fast_log2(uint32_t mode, uint32_t n, const unsigned long long* values, uint32_t* out_bits) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_zdebug_fast_log2, dim3((n + 255) / 256), dim3(256), 0, BR_STREAM, zopfli_entry_tables(), mode, n, values, out_bits);
  HIP_CHECK(hipGetLastError());
}

void zopfli_debug_literal_costs(uint32_t n_jobs, const uint32_t* lengths, const unsigned long long* offsets, const uint8_t* data,
                                uint32_t* histo, float* cost, float* prefix) {
  if (n_jobs == 0) return;
  hipLaunchKernelGGL(k_zdebug_literal_costs, dim3(n_jobs), dim3(64), 0, BR_STREAM, zopfli_entry_tables(), n_jobs, lengths, offsets, data, histo, cost,
                     prefix);
  HIP_CHECK(hipGetLastError());
}

void zopfli_debug_cost_from_histogram(uint32_t n_jobs, const uint32_t* sizes, const uint32_t* literal, const unsigned long long* offsets,
                                      const uint32_t* histograms, float* cost) {
  if (n_jobs == 0) return;
  hipLaunchKernelGGL(k_zdebug_cost_from_histogram, dim3((n_jobs + 63) / 64), dim3(64), 0, BR_STREAM, zopfli_entry_tables(), n_jobs, sizes, literal,
                     offsets, histograms, cost);
  HIP_CHECK(hipGetLastError());
}

// the hasher and the parameters the prepend looks at (a Store compares 128 bytes inside the dictionary: nothing else matters)
static ZopfliParams zopfli_entry_prepend_params(uint32_t dict_bytes, uint32_t lgwin) {
  ZopfliParams Z{};
  Z.quality = 11;
  Z.lgwin = lgwin;
  Z.max_backward_limit = (1u << lgwin) - 16u;
  Z.ring_mask = 0xffffffffu;
  Z.dict_break = dict_bytes;
  return Z;
}
__global__ __launch_bounds__(64) void k_zdebug_prepend(ZopfliParams Z, const uint8_t* __restrict__ text, uint32_t dict_bytes, uint32_t mode,
                                                       uint32_t* buckets, uint32_t* forest) {
  if (blockIdx.x != 0) return;
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  br_zopfli_batch_reset(B, Z.lgwin, dict_bytes);
  br_zopfli_batch_prepend(z_hasher_of(Z, B), Z, text, dict_bytes, mode == 0);
}
// mode 3: one wavefront replays the image over a table of 0xA5 bytes, as a chain does in front of an item of item_bytes bytes
__global__ __launch_bounds__(64) void k_zdebug_replay(const uint32_t* __restrict__ image_buckets, const uint32_t* __restrict__ image_forest, uint32_t lgwin,
                                                      uint32_t dict_bytes, uint32_t item_bytes, uint32_t* buckets, uint32_t* forest) {
  if (blockIdx.x != 0) return;
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  br_zopfli_batch_replay(B, image_buckets, image_forest, lgwin, dict_bytes, item_bytes);
}
void zopfli_debug_replay(const uint32_t* image_buckets, const uint32_t* image_forest, uint32_t lgwin, uint32_t dict_bytes, uint32_t item_bytes,
                         uint32_t* buckets, uint32_t* forest) {
  hipLaunchKernelGGL(k_zdebug_replay, dim3(1), dim3(64), 0, BR_STREAM, image_buckets, image_forest, lgwin, dict_bytes, item_bytes, buckets, forest);
  HIP_CHECK(hipGetLastError());
}
void zopfli_debug_prepend(const uint8_t* text, uint32_t dict_bytes, uint32_t lgwin, uint32_t mode, uint32_t* buckets, uint32_t* forest) {
  hipLaunchKernelGGL(k_zdebug_prepend, dim3(1), dim3(64), 0, BR_STREAM, zopfli_entry_prepend_params(dict_bytes, lgwin), text, dict_bytes, mode, buckets,
                     forest);
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
