// batch_q9.h -- quality 9 behind a custom dictionary, side by side (BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS): the host side of
// the route that BrotliMi355xCompressBatchWithDictionaryEx, BrotliMi355xCompressBatchWithDictionaries and its device form take with
// the bit set.  Item i is the stream of BrotliEncoderSetCustomDictionary + one BrotliEncoderCompressStream(FINISH) at quality 9: one
// live H9 chain that starts at position D of `dictionary | item` on a private H9 table (64 KiB of counters, 32 MiB of buckets), and
// one meta-block.  The group steps are those of the dictionary routes of qualities 5 .. 8 (batch_greedy.inc: CompressGroups,
// CompressGroupsWithDictionaries); the launch is lz77_batch_parse_h9 (batch_greedy.h), which since this route also takes a job with
// J.dict.bytes != 0 (the shared dictionary: k_parse_batch_h9_dict) or J.item_dict_bytes != nullptr (a dictionary per item:
// k_parse_batch_h9_dicts) -- batch_q9_device.h has the item code and the argument that bounds it.
#ifndef BROTLI_MI355X_BATCH_Q9_H_
#define BROTLI_MI355X_BATCH_Q9_H_

#include "batch_greedy.h"

namespace brotli_mi355x {

// Does this item go side by side behind dict_size bytes of dictionary (as the caller gave it, before the reference's truncation)?
// `params`: the caller's parameters as set (quality, lgwin, mode), not finalized.
bool BatchQ9DictionaryEligible(const EncoderParams& params, size_t dict_size, size_t input_size);
// The streams of `count` eligible items behind one dictionary (dict_size: its bytes in use, 2 .. 65536): every chain replays the
// image lz77_batch_dict_image makes once per call.  (*reference_fails)[i] != 0: the reference itself fails on item i (a copy of
// one byte at the dictionary end); its stream stays empty.  sink != nullptr: the device mode, as BatchGreedyCompressWithDictionary.
void BatchQ9CompressWithDictionary(const EncoderParams& params, const uint8_t* dict, size_t dict_size, size_t count, const uint8_t* const* inputs,
                                   const size_t* sizes, std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails,
                                   uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// ... and behind a dictionary per item (dicts[i], dict_sizes[i]: as in use), filed by the item's own chain: as
// BatchGreedyCompressWithDictionaries.
void BatchQ9CompressWithDictionaries(const EncoderParams& params, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                     const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                     std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);

}  // namespace brotli_mi355x
#endif
