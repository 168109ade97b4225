// zopfli_entry_api.h -- the device seam of the introspection entries of zopfli_entry.inc (tests/test_zopfli_parts.py).  It stands apart
// from device_api.h because lz77_kernels.hip includes that one: what a test-only seam declares is no part of the sources the LZ77
// kernels are compiled from (bench.kernel_fingerprint).
#ifndef BROTLI_MI355X_ZOPFLI_ENTRY_API_H_
#define BROTLI_MI355X_ZOPFLI_ENTRY_API_H_

#include <stdint.h>

namespace brotli_mi355x {

// ---- introspection of zopfli_device.h (zopfli_entry.inc; tests/test_zopfli_parts.py): the static dictionary search, the logarithms and
// the cost model on inputs handed in directly (zopfli_entry_kernels.hip; the emulation build: scalar loops over the same functions).
// All pointers are device memory.
// one query per lane: matches[q * 38 ..] := 38 x kZInvalidMatch, then z_find_all_dictionary_matches(text + at[q], min_length[q],
// max_length[q]); any[q] := its return value
void zopfli_debug_dictionary_matches(const uint8_t* text, uint32_t n_queries, const uint32_t* at, const uint32_t* min_length,
                                     const uint32_t* max_length, uint32_t* matches, uint32_t* any);
// one value per lane, out := the bit pattern of: mode 0 z_fast_log2(v), 1 br_fast_log2((uint32_t)v), 2 logs_16[v & 0xffff]
void zopfli_debug_fast_log2(uint32_t mode, uint32_t n, const unsigned long long* values, uint32_t* out_bits);
// one 64-lane workgroup per job, every lane with identical state as in k_zopfli_parse: job j is the lengths[j] bytes at
// data + offsets[j]; cost + offsets[j] := what z_literal_costs leaves (lengths[j] entries), prefix + offsets[j] + 2 * j := the
// literal_costs array of z_model_from_literal_costs (lengths[j] + 1 entries).  histo: 3 * 256 words per job.
void zopfli_debug_literal_costs(uint32_t n_jobs, const uint32_t* lengths, const unsigned long long* offsets, const uint8_t* data,
                                uint32_t* histo, float* cost, float* prefix);
// one job per lane: z_set_cost_from_histogram of the sizes[j] counts at histograms + offsets[j] into cost + offsets[j]
void zopfli_debug_cost_from_histogram(uint32_t n_jobs, const uint32_t* sizes, const uint32_t* literal, const unsigned long long* offsets,
                                      const uint32_t* histograms, float* cost);

// ---- the custom-dictionary prepend of the batch item at qualities 10 / 11 (batch_zopfli_device.h; tests/test_batch_dictionaries_zopfli.py)
// one 64-lane workgroup: br_zopfli_batch_reset over dict_bytes positions, then br_zopfli_batch_prepend of text[0, dict_bytes) --
// mode 0 the loop of k_zopfli_prepend on lane 0, mode 1 the wave-wide partition of the batch item -- on buckets [1 << 17] and
// forest [2 * forest slots], forest slots = min(dict_bytes rounded up to 64, 1 << lgwin)
void zopfli_debug_prepend(const uint8_t* text, uint32_t dict_bytes, uint32_t lgwin, uint32_t mode, uint32_t* buckets, uint32_t* forest);
// the shared dictionary's tree image (batch_zopfli.h: lz77_zopfli_dict_image; tests/test_batch_dictionary_zopfli.py) replayed by one
// 64-lane workgroup over a table that holds something else: br_zopfli_batch_replay in front of an item of item_bytes bytes
void zopfli_debug_replay(const uint32_t* image_buckets, const uint32_t* image_forest, uint32_t lgwin, uint32_t dict_bytes, uint32_t item_bytes,
                         uint32_t* buckets, uint32_t* forest);

}  // namespace brotli_mi355x
#endif
