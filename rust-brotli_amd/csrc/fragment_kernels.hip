// fragment_kernels.hip -- gfx950 kernels of qualities 0 and 1 (fragment_api.h, fragment_device.h): one wavefront per fragment,
// all fragments of a batch side by side (grid = number of fragments), code tables / histograms / Huffman nodes in workgroup
// memory; and the join of the fragments' slots into one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "fragment_device.h"
#include "device_api.h"
#include "device_scan.h"

namespace brotli_mi355x {

// the hash tables of the fragments of a batch: words [0, 1 << table_bits) of every fragment's slab (table_offset: a multiple of 4)
__global__ __launch_bounds__(256) void k_fragment_clear(uint32_t* __restrict__ tables, const FragmentJob* __restrict__ jobs, const uint32_t* __restrict__ order) {
  const FragmentJob job = jobs[order ? order[blockIdx.y] : blockIdx.y];
  uint4* p = (uint4*)(tables + job.table_offset);  // (the plan's strides are 0)
  const uint32_t n = (1u << job.table_bits) / 4u;  // (table_bits >= 8)
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = zero;
}

// Workgroup: the fragment's hash table in workgroup memory (dynamic: 4 << workgroup_table_bits bytes, zeroed by the item code),
// for the small fragments of a batch -- a fragment is a chain of dependent table look-ups, and these stay inside the CU.
template <bool Workgroup>
__global__ __launch_bounds__(64) void k_fragment(int quality, EntropyTables et, const uint8_t* __restrict__ input, const FragmentJob* __restrict__ jobs,
                                                 const uint32_t* __restrict__ order, FragmentBuffers B, const FragmentState* __restrict__ states_in,
                                                 FragmentState* __restrict__ states_out, FragmentResult* __restrict__ results, uint8_t* __restrict__ out) {
  __shared__ FragmentScratch S;
  __shared__ uint64_t cmd_code_words[kTreeBitsWords];
  extern __shared__ uint32_t workgroup_table[];
  const uint32_t j = BR_UNIFORM(order ? order[blockIdx.x] : blockIdx.x);
  FragmentJob job = jobs[j];
  job.in_offset = BR_UNIFORM(job.in_offset);
  job.in_size = BR_UNIFORM(job.in_size);
  job.is_last = BR_UNIFORM(job.is_last);
  job.table_bits = BR_UNIFORM(job.table_bits);
  job.start_bits = BR_UNIFORM(job.start_bits);
  job.state_in = BR_UNIFORM(job.state_in);
  if (Workgroup) br_fragment_job(quality, et, input, job, j, B, FrTableWorkgroup{workgroup_table}, states_in, states_out, results, out, S, cmd_code_words);
  else br_fragment_job(quality, et, input, job, j, B, states_in, states_out, results, out, S, cmd_code_words);
}

void frag_compress_jobs(int quality, const uint8_t* input, const FragmentJob* jobs_dev, const uint32_t* order_dev, uint32_t n,
                        uint32_t workgroup_table_bits, const FragmentBuffers& B, const FragmentState* states_in_dev,
                        FragmentState* states_out_dev, FragmentResult* results_dev, uint8_t* out) {
  if (n == 0) return;
  if (B.table_stride != 0 || B.cmd_stride != 0 || B.lit_stride != 0) throw std::runtime_error("brotli_mi355x: the fragment kernels take per-job offsets, not strides");
  if (workgroup_table_bits > kFragmentWorkgroupTableBitsMax) throw std::runtime_error("brotli_mi355x: a fragment table of this size does not fit workgroup memory");
  const DeviceTables& dt = dev_tables();
  EntropyTables et;
  et.logs_16 = dt.logs_16;
  et.logs_8 = dt.logs_8;
  if (workgroup_table_bits != 0) {
    hipLaunchKernelGGL(k_fragment<true>, dim3(n), dim3(64), (size_t)4 << workgroup_table_bits, BR_STREAM, quality, et, input, jobs_dev, order_dev, B,
                       states_in_dev, states_out_dev, results_dev, out);
  } else {
    hipLaunchKernelGGL(k_fragment_clear, dim3(32, n), dim3(256), 0, BR_STREAM, B.table, jobs_dev, order_dev);
    hipLaunchKernelGGL(k_fragment<false>, dim3(n), dim3(64), 0, BR_STREAM, quality, et, input, jobs_dev, order_dev, B, states_in_dev, states_out_dev,
                       results_dev, out);
  }
  HIP_CHECK(hipGetLastError());
}

// 64 bits of a piece per thread: read across two source words, OR into (at most) two destination words.  Pieces are disjoint in
// dst, so only their first and last words are shared -- every word goes through an atomic OR all the same (dst starts zeroed).
__global__ __launch_bounds__(256) void k_fragment_join(const uint64_t* __restrict__ src, const FragmentPiece* __restrict__ pieces, unsigned long long* __restrict__ dst) {
  const FragmentPiece pc = pieces[blockIdx.y];
  const uint64_t chunks = (pc.nbits + 63) >> 6;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = pc.src_bit + (c << 6);
    const uint64_t left = pc.nbits - (c << 6);
    const uint32_t sh = (uint32_t)(s & 63u);
    uint64_t v = src[s >> 6] >> sh;
    if (sh != 0 && left > 64u - sh) v |= src[(s >> 6) + 1] << (64u - sh);
    if (left < 64) v &= (1ull << left) - 1ull;
    if (v == 0) continue;
    const uint64_t d = pc.dst_bit + (c << 6);
    const uint32_t dh = (uint32_t)(d & 63u);
    atomicOr(dst + (d >> 6), (unsigned long long)(v << dh));
    if (dh != 0 && (v >> (64u - dh)) != 0) atomicOr(dst + (d >> 6) + 1, (unsigned long long)(v >> (64u - dh)));
  }
}

void frag_join(const uint8_t* src, const FragmentPiece* pieces_dev, uint32_t n, uint8_t* dst) { frag_join_bounded(src, pieces_dev, n, dst, 0); }

void frag_join_bounded(const uint8_t* src, const FragmentPiece* pieces_dev, uint32_t n, uint8_t* dst, uint64_t longest_bits) {
  if (n == 0) return;
  // (256 threads x 64 bits per block and round: a batch of small streams has thousands of pieces of a few KiB)
  const uint64_t blocks = longest_bits == 0 ? 64 : std::min<uint64_t>(64, (longest_bits + 256 * 64 - 1) / (256 * 64));
  hipLaunchKernelGGL(k_fragment_join, dim3((uint32_t)std::max<uint64_t>(1, blocks), n), dim3(256), 0, BR_STREAM, (const uint64_t*)src, pieces_dev, (unsigned long long*)dst);
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
