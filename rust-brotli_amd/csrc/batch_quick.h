// batch_quick.h -- the small items of a batch at qualities 2 .. 4, side by side on the device (BrotliMi355xCompressBatchEx with
// BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS).
//
// An item of at most one input block under a BasicHasher (H2 / H3 / H4) is ONE chain of br_quick_block (quick_device.h) on a
// private table and ONE meta-block: it starts on a zeroed table with the throttle books at 0, so the chain is exact on its own
// filings and nothing is speculated or repeated.  A group shares the plan of the items of qualities 5 .. 8 (batch_greedy.h): one
// padded text buffer, one parse launch (k_quick_batch: one wavefront per table, each zeroing its table before every item), the
// per-item records, the command gather (lz77_batch_gather) and one pass of the meta-block stage.  There is no key pass and there
// are no flags: a BasicHasher hashes from the text.
#ifndef BROTLI_MI355X_BATCH_QUICK_H_
#define BROTLI_MI355X_BATCH_QUICK_H_

#include <stddef.h>
#include <stdint.h>

#include "batch_greedy.h"
#include "quick_api.h"

namespace brotli_mi355x {

// ---- device seam (quick_kernels.hip; the emulation build: batch_quick_emu.inc)
struct QuickBatchJob {
  Lz77Params P;  // of a stream that starts at 0 and stays inside the first ring-buffer revolution; total_bytes is set per item
  QuickJob Q;    // the hasher; Q.table = the tables of the launch, [tables][quick_table_words(Q)] (16-byte aligned)
  const uint8_t* text;  // the group's padded text: every item at a 64-byte boundary, at least 64 zero bytes behind it
  Command* slabs;
  const BatchItem* items;
  const uint32_t* order;  // largest item first
  uint32_t n_items;
  uint32_t tables;
  uint32_t* counter;  // [1], zero: the next place of `order` to hand out
  BatchRecord* records;
  // behind a shared custom dictionary (lz77_quick_batch_parse_dict); 0 / nullptr for every other launch
  uint32_t dict_bytes;    // D: every item's text is dictionary | item, text_off names the item's first byte; positions count from
                          // the dictionary's first byte
  const uint32_t* image;  // [quick_table_words(Q)], 16-byte aligned: the table lz77_quick_init + lz77_quick_prepend leave for the
                          // dictionary (slots and books), which every chain copies over its own table in front of every item
  // behind a custom dictionary per item (lz77_quick_batch_parse_dicts); nullptr for every other launch
  const uint32_t* item_dict_bytes;  // [n_items]: item i's text is its own dictionary | item, as above; dict_bytes and image are not
                                    // looked at -- a chain files its item's dictionary into its zeroed table itself, or
  // ... copies the image the group has built of that dictionary (lz77_quick_dict_images): table image item_image[i] of `images`,
  // kBatchNoImage: none, the chain files.  item_image == nullptr: no images
  const uint32_t* images;      // [n_images][quick_table_words(Q)], 16-byte aligned
  const uint32_t* item_image;  // [n_items]
};
// The table images of a group behind a dictionary per item, in one launch: image j is what lz77_quick_init + lz77_quick_prepend
// leave for the dict_bytes[j] bytes at text + text_at[j] (the dictionary's copy in front of the first item that names it; every
// filed position hashes dictionary bytes only).  images: [n_images][quick_table_words(Q)], ZEROED by the caller -- the slots
// nothing is filed under and the books stay 0; text_at / dict_bytes: [n_images], device.
void lz77_quick_dict_images(const QuickJob& Q, const uint8_t* text, uint32_t n_images, const uint32_t* text_at_dev, const uint32_t* dict_bytes_dev,
                            uint32_t* images);
// one wavefront per table; a wavefront takes items from `counter` until none is left
void lz77_quick_batch_parse(const QuickBatchJob& J);
// the same launch for items behind a shared custom dictionary (J.dict_bytes >= 2, J.image): a chain starts on the image instead of
// a zeroed table and cuts its matches at the dictionary's end; BatchRecord::bad_commands flags the items the reference fails on
void lz77_quick_batch_parse_dict(const QuickBatchJob& J);
// the same launch for items behind a dictionary of their own (J.item_dict_bytes: 2 .. 65536 bytes each): a chain zeroes its table
// and files its item's dictionary itself (br_quick_batch_file) or copies the group's image of it (J.images), then runs as the one above
void lz77_quick_batch_parse_dicts(const QuickBatchJob& J);

// ---- items of several blocks (BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS): an item of two to kBatchLongBlocks input blocks is still
// ONE chain on a private table -- br_quick_block block after block, with the books between the blocks that the host resolver keeps
// for a one-shot call (extend_last_command, pending literals, the flush rule with the 0x2fff rule of qualities 2 and 3,
// should_compress, the saved distance cache) kept by the chain itself, as k_parse_batch_long keeps them for H5 -- and leaves up to
// kBatchLongBlocks meta-blocks, one BatchLongRecord per item.  J.records is not used; J.P.ring_mask is that of the items'
// parameters (at lgwin <= 14 such an item passes the ring buffer's first lap) and J.P.quality decides the 0x2fff rule.
// The gather is lz77_batch_gather_long.
void lz77_quick_batch_parse_long(const QuickBatchJob& J, BatchLongRecord* records);

// ---- host
// Does this item go side by side under the quick route?  `params`: the caller's parameters as set, not finalized.
bool BatchQuickEligible(const EncoderParams& params, size_t input_size);
// ... under the quick-long route: the same tests for an item of more than one and at most kBatchLongBlocks input blocks
bool BatchQuickLongEligible(const EncoderParams& params, size_t input_size);
// The streams of `count` such items.  (*demoted)[i] != 0: as for BatchLongCompress -- no stream, the caller redoes the item.
void BatchQuickLongCompress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                            std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* demoted, uint32_t* groups,
                            const BatchDeviceSink* sink = nullptr);
// The streams of `count` eligible items.  Throws std::runtime_error on a device error.  *groups: device groups run.
void BatchQuickCompress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                        std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// Behind a shared custom dictionary (BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS): does
// this item of at most one input block go side by side?  dict_size: as the caller gave it, before the reference's truncation.
bool BatchQuickDictionaryEligible(const EncoderParams& params, size_t dict_size, size_t input_size);
// The streams of `count` such items: item i is the stream of BrotliEncoderSetCustomDictionary + one FINISH.  dict, dict_use: the
// dictionary bytes in use (2 .. 65536, after the truncation).  (*reference_fails)[i] != 0: the reference itself fails on item i (a
// copy of one byte at the dictionary end); its stream stays empty.
void BatchQuickCompressWithDictionary(const EncoderParams& params, const uint8_t* dict, size_t dict_use, size_t count,
                                      const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                      std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// Behind a custom dictionary per item (BrotliMi355xCompressBatchWithDictionaries with
// BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS): item i is eligible by BatchQuickDictionaryEligible with its own dictionary.
// dicts[i] / dict_sizes[i]: the dictionary of item i as in use (2 .. 65536 bytes, after the truncation); two items share one
// where pointer and size agree.  streams, reference_fails, groups: as above.
// sink != nullptr, for both: the device mode, as for the dictionary routes of batch_greedy.h.
void BatchQuickCompressWithDictionaries(const EncoderParams& params, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                        const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                        std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);

}  // namespace brotli_mi355x
#endif
