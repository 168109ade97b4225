// batch_device.h -- the device seam of BrotliMi355xCompressBatchDevice and BrotliMi355xCompressBatchWithDictionariesDevice: the items
// of a batch, and the dictionaries they lie behind, are in the caller's device memory and their streams go to the caller's device
// memory (batch_device_kernels.hip; the emulation build: batch_device_emu.inc).
//
// Both launches stand on one copy of n bytes from any address to any address.  It reads only the aligned 4-byte words that hold
// a source byte and writes exactly dst[0 .. n): the bytes around a destination belong to somebody else -- the neighbour in the
// packed text, or a caller's abutting output -- so no shared word is ever read, changed and written back.
#ifndef BROTLI_MI355X_BATCH_DEVICE_H_
#define BROTLI_MI355X_BATCH_DEVICE_H_

#include <stddef.h>
#include <stdint.h>

#include "batch_greedy.h"

namespace brotli_mi355x {

// text[items[i].text_off ..) = packed[starts[i] ..) = the items[i].bytes bytes at srcs_dev[i], for every item of a group.  `text`
// and `packed` are the group's (zero where nothing is written: the launch writes no padding), srcs_dev is an array of n_items
// device addresses, itself on the device; text_off is a multiple of 64, starts[i] and srcs_dev[i] have any alignment.
void batch_stage_device(const uint8_t* const* srcs_dev, const BatchItem* items_dev, const uint32_t* starts_dev, uint32_t n_items, uint8_t* text,
                        uint8_t* packed);

// The same behind a dictionary per item (the device mode of the four dictionary routes): text[items[i].text_off - dict_bytes[i] ..
// items[i].text_off) = the dict_bytes[i] bytes at dicts_dev[i], the dictionary's end abutting the item's first byte, and the item
// as above in both texts.  dicts_dev[i] points at the first dictionary byte IN USE (behind the reference's truncation) and has any
// alignment; several items may name one address, and a dictionary may overlap any item.  text_off is at least dict_bytes[i] rounded
// up to 64.  One launch in place of the page-locked staging, the dictionary pool and its upload, the upload of the packed text and
// lz77_batch_dict_text / lz77_batch_dicts_text.
void batch_stage_dicts_device(const uint8_t* const* srcs_dev, const uint8_t* const* dicts_dev, const uint32_t* dict_bytes_dev,
                              const BatchItem* items_dev, const uint32_t* starts_dev, uint32_t n_items, uint8_t* text, uint8_t* packed);

// dst[0 .. bytes) = src[0 .. bytes), both on the device with any alignment and not overlapping: the shared dictionary on its way to
// the call's own copy, read under the contract above
void batch_copy_device(uint8_t* dst, const uint8_t* src, uint32_t bytes);

// One stream that goes out: `bytes` bytes of the group's output from byte `src_off` (a multiple of 8) to the device address `dst`.
struct BatchDeliverOp {
  uint64_t dst;
  uint64_t src_off;
  uint64_t bytes;
};
// dst[0 .. bytes) = out_dev[src_off .. src_off + bytes) for every op; ops_dev is on the device
void batch_deliver(const uint8_t* out_dev, const BatchDeliverOp* ops_dev, uint32_t n_ops);

// The context bytes of follow-on meta-blocks: out_dev[2 * k] = packed[at_dev[k] - 1], out_dev[2 * k + 1] = packed[at_dev[k] - 2]
// for k < n; every at_dev[k] is at least 2.
void batch_gather_context(const uint8_t* packed_dev, const uint32_t* at_dev, uint32_t n, uint8_t* out_dev);

}  // namespace brotli_mi355x
#endif
