// batch_device_kernels.hip -- the gfx950 kernels of BrotliMi355xCompressBatchDevice (batch_device.h): the items of a group come
// out of the caller's device memory into the group's two texts (k_batch_stage_device; behind dictionaries that lie there too:
// k_batch_stage_dicts_device), and the streams of a group go from its output to the caller's device memory (k_batch_deliver).
// A translation unit of its own, so that the kernels of lz77_kernels.hip compile as they did.
#include <hip/hip_runtime.h>

#include "batch_device.h"
#include "device_api.h"
#include "device_scan.h"  // HIP_CHECK

namespace brotli_mi355x {

// dst[0 .. n) = src[0 .. n) by one workgroup; src and dst have any alignment and do not overlap.
// Writes: exactly dst[0 .. n).  The body goes in 16-byte stores at 16-byte boundaries of the DESTINATION, one per lane and step, so
// that a wavefront writes 1 KiB in a row; the up to 15 bytes in front of the first boundary and behind the last go byte by byte --
// their neighbours in the same word are another workgroup's to write.  Below 32 bytes everything goes byte by byte.
// Reads: the aligned dwords that hold a source byte and no other.  A body word takes the four or five aligned dwords around its
// 16 source bytes and funnel-shifts them by the source's misalignment against the destination (one value for the whole copy); the
// fifth dword is only needed where that misalignment is not 0, and then it holds a source byte -- where it is 0 its address is
// clamped to the last dword of the source, and its value is not used.
__device__ __forceinline__ void batch_copy_any(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n) {
  if (n < 32u) {
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
    return;
  }
  const uint32_t head = (uint32_t)((0u - (uintptr_t)dst) & 15u);
  const uint32_t words = (n - head) >> 4;  // at least 1
  const uint32_t tail_at = head + 16u * words;
  const uint8_t* __restrict__ body = src + head;
  const uint32_t mis = (uint32_t)((uintptr_t)body & 3u);
  const uint32_t* __restrict__ s32 = (const uint32_t*)(body - mis);
  const uint32_t* __restrict__ last = (const uint32_t*)((uintptr_t)(src + (n - 1u)) & ~(uintptr_t)3);
  uint4* __restrict__ d128 = (uint4*)(dst + head);
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
    uint32_t d[5], v[4];
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) {
      const uint32_t* p = s32 + (4u * w + j);
      d[j] = *(p > last ? last : p);
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) v[j] = __funnelshift_r(d[j], d[j + 1], 8u * mis);
    d128[w] = make_uint4(v[0], v[1], v[2], v[3]);
  }
  const uint32_t edge = head + (n - tail_at);  // at most 30
  for (uint32_t t = threadIdx.x; t < edge; t += blockDim.x) {
    const uint32_t k = t < head ? t : tail_at + (t - head);
    dst[k] = src[k];
  }
}

// Kernel A.  One workgroup per item, the shape of k_batch_dict_text: the item goes to its place in the padded text (a 64-byte
// boundary) and to its place in the packed text (any alignment, the neighbours abut).  Both texts are zero beforehand.
__global__ __launch_bounds__(256) void k_batch_stage_device(const uint8_t* const* __restrict__ srcs, const BatchItem* __restrict__ items,
                                                             const uint32_t* __restrict__ starts, uint32_t n_items, uint8_t* __restrict__ text,
                                                             uint8_t* __restrict__ packed) {
  const uint32_t i = blockIdx.x;
  if (i >= n_items) return;
  const BatchItem it = items[i];
  const uint8_t* src = srcs[i];
  batch_copy_any(text + it.text_off, src, it.bytes);
  batch_copy_any(packed + starts[i], src, it.bytes);
}

void batch_stage_device(const uint8_t* const* srcs_dev, const BatchItem* items_dev, const uint32_t* starts_dev, uint32_t n_items, uint8_t* text,
                        uint8_t* packed) {
  if (n_items == 0) return;
  hipLaunchKernelGGL(k_batch_stage_device, dim3(n_items), dim3(256), 0, BR_STREAM, srcs_dev, items_dev, starts_dev, n_items, text, packed);
  HIP_CHECK(hipGetLastError());
}

// Kernel A behind a dictionary per item.  One workgroup per item lays out `dictionary | item` in the padded text -- the dictionary
// ends where the item starts, a 64-byte boundary -- and the item in the packed text.  A dictionary is read where it lies, by every
// item that names it; nothing is pooled.  (text_off >= dict_bytes[i] rounded up to 64: the host plan's DictRoom.)
__global__ __launch_bounds__(256) void k_batch_stage_dicts_device(const uint8_t* const* __restrict__ srcs, const uint8_t* const* __restrict__ dicts,
                                                                   const uint32_t* __restrict__ dict_bytes, const BatchItem* __restrict__ items,
                                                                   const uint32_t* __restrict__ starts, uint32_t n_items, uint8_t* __restrict__ text,
                                                                   uint8_t* __restrict__ packed) {
  const uint32_t i = blockIdx.x;
  if (i >= n_items) return;
  const BatchItem it = items[i];
  const uint32_t D = dict_bytes[i];
  const uint8_t* src = srcs[i];
  if (D <= it.text_off) batch_copy_any(text + (it.text_off - D), dicts[i], D);
  batch_copy_any(text + it.text_off, src, it.bytes);
  batch_copy_any(packed + starts[i], src, it.bytes);
}

void batch_stage_dicts_device(const uint8_t* const* srcs_dev, const uint8_t* const* dicts_dev, const uint32_t* dict_bytes_dev,
                              const BatchItem* items_dev, const uint32_t* starts_dev, uint32_t n_items, uint8_t* text, uint8_t* packed) {
  if (n_items == 0) return;
  hipLaunchKernelGGL(k_batch_stage_dicts_device, dim3(n_items), dim3(256), 0, BR_STREAM, srcs_dev, dicts_dev, dict_bytes_dev, items_dev, starts_dev,
                     n_items, text, packed);
  HIP_CHECK(hipGetLastError());
}

// one workgroup, one copy: the shared dictionary of a call (at most 65 536 bytes)
__global__ __launch_bounds__(256) void k_batch_copy_device(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t bytes) {
  batch_copy_any(dst, src, bytes);
}

void batch_copy_device(uint8_t* dst, const uint8_t* src, uint32_t bytes) {
  if (bytes == 0) return;
  hipLaunchKernelGGL(k_batch_copy_device, dim3(1), dim3(256), 0, BR_STREAM, dst, src, bytes);
  HIP_CHECK(hipGetLastError());
}

// Kernel B.  One workgroup per stream that goes out.
__global__ __launch_bounds__(256) void k_batch_deliver(const uint8_t* __restrict__ out, const BatchDeliverOp* __restrict__ ops, uint32_t n_ops) {
  const uint32_t i = blockIdx.x;
  if (i >= n_ops) return;
  const BatchDeliverOp op = ops[i];
  batch_copy_any((uint8_t*)(uintptr_t)op.dst, out + op.src_off, (uint32_t)op.bytes);
}

void batch_deliver(const uint8_t* out_dev, const BatchDeliverOp* ops_dev, uint32_t n_ops) {
  if (n_ops == 0) return;
  hipLaunchKernelGGL(k_batch_deliver, dim3(n_ops), dim3(256), 0, BR_STREAM, out_dev, ops_dev, n_ops);
  HIP_CHECK(hipGetLastError());
}

// the two text bytes in front of every follow-on meta-block of a group, one lane each
__global__ __launch_bounds__(256) void k_batch_gather_context(const uint8_t* __restrict__ packed, const uint32_t* __restrict__ at, uint32_t n,
                                                               uint8_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t a = at[k];
  if (a < 2u) return;  // (never: a follow-on meta-block starts a whole input block into its item)
  out[2u * k] = packed[a - 1u];
  out[2u * k + 1u] = packed[a - 2u];
}

void batch_gather_context(const uint8_t* packed_dev, const uint32_t* at_dev, uint32_t n, uint8_t* out_dev) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_batch_gather_context, dim3((n + 255u) / 256u), dim3(256), 0, BR_STREAM, packed_dev, at_dev, n, out_dev);
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
