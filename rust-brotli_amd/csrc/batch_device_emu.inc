// batch_device_emu.inc -- the host emulation of batch_device.h: in that build device memory is host memory.  Every copy moves
// exactly [src, src + n) to [dst, dst + n), as the kernels do: a sanitizer on buffers sized to the items judges the plan's bounds.
#include <string.h>

#include "batch_device.h"

namespace brotli_mi355x {

void batch_stage_device(const uint8_t* const* srcs, const BatchItem* items, const uint32_t* starts, uint32_t n_items, uint8_t* text, uint8_t* packed) {
  for (uint32_t i = 0; i < n_items; ++i) {
    memcpy(text + items[i].text_off, srcs[i], items[i].bytes);
    memcpy(packed + starts[i], srcs[i], items[i].bytes);
  }
}

void batch_stage_dicts_device(const uint8_t* const* srcs, const uint8_t* const* dicts, const uint32_t* dict_bytes, const BatchItem* items,
                              const uint32_t* starts, uint32_t n_items, uint8_t* text, uint8_t* packed) {
  for (uint32_t i = 0; i < n_items; ++i) {
    if (dict_bytes[i] <= items[i].text_off) memcpy(text + (items[i].text_off - dict_bytes[i]), dicts[i], dict_bytes[i]);
    memcpy(text + items[i].text_off, srcs[i], items[i].bytes);
    memcpy(packed + starts[i], srcs[i], items[i].bytes);
  }
}

void batch_copy_device(uint8_t* dst, const uint8_t* src, uint32_t bytes) { memcpy(dst, src, bytes); }

void batch_deliver(const uint8_t* out, const BatchDeliverOp* ops, uint32_t n_ops) {
  for (uint32_t i = 0; i < n_ops; ++i) memcpy((uint8_t*)(uintptr_t)ops[i].dst, out + ops[i].src_off, (size_t)ops[i].bytes);
}

void batch_gather_context(const uint8_t* packed, const uint32_t* at, uint32_t n, uint8_t* out) {
  for (uint32_t k = 0; k < n; ++k) {
    if (at[k] < 2u) continue;
    out[2u * k] = packed[at[k] - 1u];
    out[2u * k + 1u] = packed[at[k] - 2u];
  }
}

}  // namespace brotli_mi355x
