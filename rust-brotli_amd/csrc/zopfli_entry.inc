// zopfli_entry.inc -- introspection entry points of the backward-reference stage of qualities 10 and 11 (zopfli_device.h): queries
// straight to z_find_all_dictionary_matches, values straight to the logarithms, blocks of bytes straight to the literal cost model and
// histogram rows straight to z_set_cost_from_histogram (k_zdebug_* in the product library, the scalar twins in the emulation build).
// Whole streams cannot steer these parts -- a row of the affix tables shows in a stream only where the text reaches it AND the
// shortest path picks it, and a cost that is off in its last bit only where two paths tie that closely -- so their parity tests
// (tests/test_zopfli_parts.py) come in here.  Every entry calls the functions the product calls; nothing is restated.  Not part of
// the public header.
#include <string.h>

#include <exception>
#include <vector>

#include "batch_zopfli.h"
#include "device_api.h"
#include "zopfli_entry_api.h"
#if defined(BROTLI_HOST_EMU)
#include "batch_zopfli_device.h"

namespace brotli_mi355x {
// the scalar twin of k_zdebug_prepend (zopfli_entry_kernels.hip): the same two functions on plain memory; mode 1 walks the 64
// key classes of the wave-wide partition one after the other
void zopfli_debug_prepend(const uint8_t* text, uint32_t dict_bytes, uint32_t lgwin, uint32_t mode, uint32_t* buckets, uint32_t* forest) {
  ZopfliParams Z{};
  Z.quality = 11;
  Z.lgwin = lgwin;
  Z.max_backward_limit = (1u << lgwin) - 16u;
  Z.ring_mask = 0xffffffffu;
  Z.dict_break = dict_bytes;
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  br_zopfli_batch_reset(B, lgwin, dict_bytes);
  br_zopfli_batch_prepend(z_hasher_of(Z, B), Z, text, dict_bytes, mode == 0);
}
void zopfli_debug_replay(const uint32_t* image_buckets, const uint32_t* image_forest, uint32_t lgwin, uint32_t dict_bytes, uint32_t item_bytes,
                         uint32_t* buckets, uint32_t* forest) {
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  br_zopfli_batch_replay(B, image_buckets, image_forest, lgwin, dict_bytes, item_bytes);
}
}  // namespace brotli_mi355x
#endif

using namespace brotli_mi355x;

namespace {
// What the product's text buffer carries behind the text (Lz77Buffers::text is total_bytes + 64, zero-filled: lz77_stage.cpp).
constexpr size_t kZEntryTextPadding = 64;
constexpr uint32_t kZEntryDictWords = 38;  // dict_matches[0 .. 37] of z_find_all_matches
}  // namespace

extern "C" {

// BrotliFindAllStaticDictionaryMatches of n_queries places of one text.  The text goes to device memory once, followed by the 64
// zero bytes the product's text buffer ends with (the search loads the four bytes at its place whatever max_length is, as the
// reference does, so up to three of them can be read).  Query q asks at text + at[q] with min_length[q] / max_length[q]; refused:
// max_length 0 or at + max_length > n_text, more than 2^20 queries, more than 16 MiB of text.  Out, per query: 38 words that start as
// kZInvalidMatch (0x0fffffff) -- entry `len` is the smallest (distance << 5 | length code) of the words that match `len` bytes --
// and out_any, the function's return value.  Returns 0, -1 for arguments it refuses (nothing is launched), -2 when the device layer
// threw.
int brotli_mi355x_debug_dictionary_matches(const uint8_t* text, uint32_t n_text, uint32_t n_queries, const uint32_t* at, const uint32_t* min_length,
                                           const uint32_t* max_length, uint32_t* out_matches, uint32_t* out_any) {
  if (n_queries == 0 || n_queries > (1u << 20) || n_text == 0 || n_text > (16u << 20)) return -1;
  if (!text || !at || !min_length || !max_length || !out_matches || !out_any) return -1;
  for (uint32_t q = 0; q < n_queries; ++q)
    if (max_length[q] == 0 || (uint64_t)at[q] + max_length[q] > n_text) return -1;
  try {
    DevMem mm;
    uint8_t* text_dev = mm.alloc<uint8_t>((size_t)n_text + kZEntryTextPadding);  // (zero-filled)
    uint32_t* at_dev = mm.alloc<uint32_t>(n_queries);
    uint32_t* min_dev = mm.alloc<uint32_t>(n_queries);
    uint32_t* max_dev = mm.alloc<uint32_t>(n_queries);
    uint32_t* matches_dev = mm.alloc<uint32_t>((size_t)n_queries * kZEntryDictWords);
    uint32_t* any_dev = mm.alloc<uint32_t>(n_queries);
    dev_h2d(text_dev, text, n_text);
    dev_h2d(at_dev, at, (size_t)n_queries * 4);
    dev_h2d(min_dev, min_length, (size_t)n_queries * 4);
    dev_h2d(max_dev, max_length, (size_t)n_queries * 4);
    zopfli_debug_dictionary_matches(text_dev, n_queries, at_dev, min_dev, max_dev, matches_dev, any_dev);
    dev_d2h(out_matches, matches_dev, (size_t)n_queries * kZEntryDictWords * 4);
    dev_d2h(out_any, any_dev, (size_t)n_queries * 4);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// The logarithms as device code has them, one value per lane: mode 0 z_fast_log2(v) (FastLog2f64: the table below 256, else the
// restated log2f of the 64-bit count as f32), mode 1 br_fast_log2((uint32_t)v) (FastLog2), mode 2 logs_16[v & 0xffff] (the table of
// the entropy sums as it sits in device memory).  Out: the bit patterns.  Refused: mode > 2, n 0 or above 2^25.
int brotli_mi355x_debug_fast_log2(uint32_t mode, uint32_t n, const uint64_t* values, uint32_t* out_bits) {
  if (mode > 2 || n == 0 || n > (1u << 25) || !values || !out_bits) return -1;
  try {
    DevMem mm;
    unsigned long long* values_dev = mm.alloc<unsigned long long>(n);
    uint32_t* out_dev = mm.alloc<uint32_t>(n);
    dev_h2d(values_dev, values, (size_t)n * 8);
    zopfli_debug_fast_log2(mode, n, values_dev, out_dev);
    dev_d2h(out_bits, out_dev, (size_t)n * 4);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// BrotliEstimateBitCostsForLiterals and the running sum of ZopfliCostModel::set_from_literal_costs of n_jobs blocks of bytes.
// lengths: n_jobs, each 1 .. 65536; data: the blocks one behind the other.  Out, the jobs one behind the other: out_cost_bits --
// per job `len` costs as z_literal_costs left them; out_prefix_bits -- per job the `len + 1` entries of the model's literal_costs
// (job j starts at its data offset + j).  Refused: n_jobs 0 or above 4096, a length out of range.
int brotli_mi355x_debug_literal_costs(uint32_t n_jobs, const uint32_t* lengths, const uint8_t* data, uint32_t* out_cost_bits, uint32_t* out_prefix_bits) {
  if (n_jobs == 0 || n_jobs > 4096 || !lengths || !data || !out_cost_bits || !out_prefix_bits) return -1;
  std::vector<unsigned long long> offsets(n_jobs);
  size_t total = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    if (lengths[j] == 0 || lengths[j] > 65536) return -1;
    offsets[j] = total;
    total += lengths[j];
  }
  try {
    DevMem mm;
    uint8_t* data_dev = mm.alloc<uint8_t>(total + kZEntryTextPadding);
    uint32_t* lengths_dev = mm.alloc<uint32_t>(n_jobs);
    unsigned long long* offsets_dev = mm.alloc<unsigned long long>(n_jobs);
    uint32_t* histo_dev = mm.alloc<uint32_t>((size_t)n_jobs * 768);
    float* cost_dev = mm.alloc<float>(total);
    float* prefix_dev = mm.alloc<float>(total + 2 * (size_t)n_jobs);  // (literal_costs is num_bytes + 2 entries per job)
    dev_h2d(data_dev, data, total);
    dev_h2d(lengths_dev, lengths, (size_t)n_jobs * 4);
    dev_h2d(offsets_dev, offsets.data(), (size_t)n_jobs * 8);
    zopfli_debug_literal_costs(n_jobs, lengths_dev, offsets_dev, data_dev, histo_dev, cost_dev, prefix_dev);
    std::vector<uint32_t> prefix(total + 2 * (size_t)n_jobs);
    dev_d2h(out_cost_bits, cost_dev, total * 4);
    dev_d2h(prefix.data(), prefix_dev, prefix.size() * 4);
    for (uint32_t j = 0; j < n_jobs; ++j)
      memcpy(out_prefix_bits + offsets[j] + j, prefix.data() + offsets[j] + 2 * (size_t)j, ((size_t)lengths[j] + 1) * 4);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// SetCost (hq.rs:1043-1071) of n_jobs histogram rows.  sizes: n_jobs, each 1 .. 1200; literal: per job, 1 for a literal histogram (no
// count added for the symbols that are missing); histograms: the rows one behind the other.  Out: the bit patterns of the costs, laid
// out like the rows.  Refused: n_jobs 0 or above 4096, a size out of range, a literal flag above 1.
int brotli_mi355x_debug_cost_from_histogram(uint32_t n_jobs, const uint32_t* sizes, const uint32_t* literal, const uint32_t* histograms,
                                            uint32_t* out_cost_bits) {
  if (n_jobs == 0 || n_jobs > 4096 || !sizes || !literal || !histograms || !out_cost_bits) return -1;
  std::vector<unsigned long long> offsets(n_jobs);
  size_t total = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    if (sizes[j] == 0 || sizes[j] > 1200 || literal[j] > 1) return -1;
    offsets[j] = total;
    total += sizes[j];
  }
  try {
    DevMem mm;
    uint32_t* sizes_dev = mm.alloc<uint32_t>(n_jobs);
    uint32_t* literal_dev = mm.alloc<uint32_t>(n_jobs);
    unsigned long long* offsets_dev = mm.alloc<unsigned long long>(n_jobs);
    uint32_t* histograms_dev = mm.alloc<uint32_t>(total);
    float* cost_dev = mm.alloc<float>(total);
    dev_h2d(sizes_dev, sizes, (size_t)n_jobs * 4);
    dev_h2d(literal_dev, literal, (size_t)n_jobs * 4);
    dev_h2d(offsets_dev, offsets.data(), (size_t)n_jobs * 8);
    dev_h2d(histograms_dev, histograms, total * 4);
    zopfli_debug_cost_from_histogram(n_jobs, sizes_dev, literal_dev, offsets_dev, histograms_dev, cost_dev);
    dev_d2h(out_cost_bits, cost_dev, total * 4);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// HasherPrependCustomDictionary for H10 as the batch item of qualities 10 / 11 runs it (batch_zopfli_device.h), on a hasher that
// br_zopfli_batch_reset has emptied: the first dict_bytes bytes of `text` are the dictionary (n_text >= dict_bytes: a Store
// compares bytes of the dictionary only, what follows is carried along as the item would be).  mode 0: the loop of k_zopfli_prepend
// on lane 0; mode 1: the batch item's wave-wide partition on one wavefront; mode 2: the tree image of the shared dictionary as the
// call builds it (lz77_zopfli_dict_image: fill, class pass, store launch of several workgroups).  Out: the buckets (1 << 17 words)
// and the forest, 2 words for each of min(dict_bytes rounded up to 64, 1 << lgwin) positions.
// mode 3: that image, built and then replayed (br_zopfli_batch_replay) in front of an item of n_text - dict_bytes bytes over buckets
// and a forest that hold 0xA5 bytes.  Out: the buckets and 2 forest words for each of min(n_text rounded up to 64, 1 << lgwin)
// positions -- the caller sizes out_forest by n_text here.
// Refused: mode > 3, lgwin outside 10 .. 24, dict_bytes > n_text or > (1 << lgwin) - 16, more than 16 MiB of text.
int brotli_mi355x_debug_zopfli_prepend(const uint8_t* text, uint32_t n_text, uint32_t dict_bytes, uint32_t lgwin, uint32_t mode, uint32_t* out_buckets,
                                       uint32_t* out_forest) {
  if (mode > 3 || lgwin < 10 || lgwin > 24 || !text || !out_buckets || !out_forest) return -1;
  if (n_text == 0 || n_text > (16u << 20) || dict_bytes > n_text || dict_bytes > (1u << lgwin) - 16u) return -1;
  const size_t slots = zopfli_dict_image_slots(dict_bytes, lgwin);
  const size_t out_slots = mode == 3 ? zopfli_dict_image_slots(n_text, lgwin) : slots;
  try {
    DevMem mm;
    uint8_t* text_dev = mm.alloc<uint8_t>((size_t)n_text + kZEntryTextPadding);  // (zero-filled)
    uint32_t* buckets_dev = mm.alloc<uint32_t>((size_t)1 << 17);
    uint32_t* forest_dev = mm.alloc<uint32_t>(2 * slots + 64);
    dev_h2d(text_dev, text, n_text);
    if (mode >= 2) {
      uint16_t* classes_dev = mm.alloc<uint16_t>((size_t)zopfli_dict_image_class_entries(dict_bytes) + 64);
      lz77_zopfli_dict_image(text_dev, dict_bytes, lgwin, classes_dev, buckets_dev, forest_dev);
    } else {
      zopfli_debug_prepend(text_dev, dict_bytes, lgwin, mode, buckets_dev, forest_dev);
    }
    if (mode == 3) {
      uint32_t* table_buckets = mm.alloc<uint32_t>((size_t)1 << 17);
      uint32_t* table_forest = mm.alloc<uint32_t>(2 * out_slots + 64);
      dev_memset(table_buckets, 0xA5, ((size_t)1 << 17) * 4);
      dev_memset(table_forest, 0xA5, (2 * out_slots + 64) * 4);
      zopfli_debug_replay(buckets_dev, forest_dev, lgwin, dict_bytes, n_text - dict_bytes, table_buckets, table_forest);
      buckets_dev = table_buckets;
      forest_dev = table_forest;
    }
    dev_d2h(out_buckets, buckets_dev, ((size_t)1 << 17) * 4);
    if (out_slots) dev_d2h(out_forest, forest_dev, 2 * out_slots * 4);
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}
}
