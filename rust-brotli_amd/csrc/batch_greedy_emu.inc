// batch_greedy_emu.inc -- host emulation of the batch seam of qualities 5 .. 8 (batch_greedy.h: lz77_batch_parse,
// lz77_batch_gather), compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu; batch_greedy.inc includes it there): the
// same item code (batch_greedy_device.h) on plain memory, one item after the other in the order of the plan, the tables taken in
// turn -- so that a table serves several items, as on the device.
#include <string.h>

#include <stdexcept>

#include "batch_greedy_device.h"
#include "batch_q9_device.h"
#include "device_api.h"

namespace brotli_mi355x {

namespace {
ChainTables EmuBatchChainTables(const BatchParseJob& J) {
  const DeviceTables& dt = dev_tables();
  ChainTables T;
  T.text = J.text;
  T.info = nullptr;
  T.sorted = nullptr;
  T.rows = nullptr;
  T.run_end = nullptr;
  T.work = nullptr;
  T.search_log = nullptr;
  T.flags_next = J.flags;
  T.cmds = J.slabs;
  T.dict_hash = dt.dict_hash;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  T.dict_size_bits_by_length = dt.dict_size_bits_by_length;
  T.dist_postfix_bits = J.P.dist_postfix_bits;
  T.num_direct_distance_codes = J.P.num_direct_distance_codes;
  T.keys = J.keys;
  T.logs.logs_16 = dt.logs_16;
  T.logs.logs_8 = dt.logs_8;
  return T;
}
}  // namespace

void lz77_batch_parse(const BatchParseJob& J) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  if (J.P.block_bits > 7) throw std::runtime_error("brotli_mi355x: the batch chains do not run the 512-deep rings");
  const ChainTables T = EmuBatchChainTables(J);
  static thread_local ChainScratchT<false, false> scratch;
  uint32_t histo[256];
  for (uint32_t place = 0; place < J.n_items; ++place) {
    if (J.dict.bytes != 0) br_batch_item<false, true>(J, T, scratch, histo, J.order[place], place % J.tables);
    else br_batch_item<false>(J, T, scratch, histo, J.order[place], place % J.tables);
  }
  *J.counter = J.n_items;
}

// a dictionary per item: the same plan, every chain filing its own dictionary
void lz77_batch_parse_dicts(const BatchParseJob& J) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  if (J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a batch group without its dictionary sizes");
  if (J.P.block_bits > 7) throw std::runtime_error("brotli_mi355x: the batch chains do not run the 512-deep rings");
  const ChainTables T = EmuBatchChainTables(J);
  static thread_local ChainScratchT<false, false> scratch;
  uint32_t histo[256];
  for (uint32_t place = 0; place < J.n_items; ++place) br_batch_item<false, true, true>(J, T, scratch, histo, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

// qualities 9 and 10: the same plan on the H9 item code and its own scratch (the 256-deep rings' candidates)
void lz77_batch_parse_h9(const BatchParseJob& J) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  if (J.P.hasher_kind != 9 || J.P.block_bits != 8 || J.P.ndist > 16) throw std::runtime_error("brotli_mi355x: not the job of an H9 batch chain");
  if (J.dict.bytes > 65536 || (J.dict.bytes != 0 && J.item_dict_bytes != nullptr) || J.P.ring_mask < (1u << 18) - 1u)
    throw std::runtime_error("brotli_mi355x: not the job of an H9 batch chain");
  const ChainTables T = EmuBatchChainTables(J);
  static thread_local ChainScratchT<true, false> scratch;
  uint32_t histo[256];
  // behind a dictionary (batch_q9_device.h): one per item, or the call's shared one
  for (uint32_t place = 0; place < J.n_items; ++place) {
    if (J.item_dict_bytes != nullptr) br_batch_item_h9_dict<true>(J, T, scratch, histo, J.order[place], place % J.tables);
    else if (J.dict.bytes != 0) br_batch_item_h9_dict<false>(J, T, scratch, histo, J.order[place], place % J.tables);
    else br_batch_item_h9(J, T, scratch, histo, J.order[place], place % J.tables);
  }
  *J.counter = J.n_items;
}

void lz77_batch_parse_long(const BatchParseJob& J, BatchLongRecord* records) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  if (J.P.block_bits > 7) throw std::runtime_error("brotli_mi355x: the batch chains do not run the 512-deep rings");
  const ChainTables T = EmuBatchChainTables(J);
  static thread_local ChainScratchT<false, false> scratch;
  uint32_t histo[256];
  for (uint32_t place = 0; place < J.n_items; ++place) br_batch_item_long<false>(J, records, T, scratch, histo, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

void lz77_batch_gather_long(const BatchParseJob& J, const BatchLongRecord* records, const uint32_t* offsets, Command* out) {
  for (uint32_t i = 0; i < J.n_items; ++i) {
    const BatchLongRecord& r = records[i];
    if (r.overflow) continue;
    for (uint32_t m = 0; m < r.n_mb && m < kBatchLongBlocks; ++m) {
      const BatchLongMetaBlock& mb = r.mb[m];
      if ((uint64_t)mb.first_cmd + mb.n_cmds > J.items[i].cmd_cap) continue;
      const uint32_t n = mb.n_cmds + (mb.trailing != 0 ? 1u : 0u);
      for (uint32_t c = 0; c < n; ++c) out[offsets[kBatchLongBlocks * i + m] + c] = br_batch_long_command(J, J.items[i], mb, c);
    }
  }
}

void lz77_batch_dict_text(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed, const uint32_t* starts, const BatchItem* items,
                          uint32_t n_items, uint8_t* text) {
  for (uint32_t i = 0; i < n_items; ++i) {
    memcpy(text + items[i].text_off - dict_bytes, dict + ((0u - dict_bytes) & 15u), dict_bytes);
    memcpy(text + items[i].text_off, packed + starts[i], items[i].bytes);
  }
}

void lz77_batch_dicts_text(const uint8_t* pool, const uint32_t* dict_off, const uint32_t* dict_bytes, const uint8_t* packed,
                           const uint32_t* starts, const BatchItem* items, uint32_t n_items, uint8_t* text) {
  for (uint32_t i = 0; i < n_items; ++i) {
    // whole 16-byte words, as the kernel moves them: the dictionary's own zero lead comes along
    const uint32_t words = (dict_bytes[i] + 15u) >> 4;
    if (items[i].text_off < 16u * words || dict_off[i] + dict_bytes[i] < 16u * words) throw std::runtime_error("brotli_mi355x: a batch item without room for its dictionary");
    memcpy(text + items[i].text_off - 16u * words, pool + (dict_off[i] + dict_bytes[i] - 16u * words), 16u * words);
    memcpy(text + items[i].text_off, packed + starts[i], items[i].bytes);
  }
}

void lz77_batch_dict_image(const Lz77Params& P, const uint16_t* keys, uint32_t dict_bytes, uint16_t* num, uint32_t* buckets,
                           uint32_t* entries, uint32_t* n_entries) {
  LiveRing lr;
  lr.num = num;
  lr.buckets = buckets;
  lr.keys = keys;
  lr.bits = P.block_bits;
  br_live_reset(lr, P.bucket_bits);
  if (dict_bytes > P.htl - 1) br_live_store(lr, 0, 1, dict_bytes - (P.htl - 1), 1, 0);  // StoreLookaheadThenStore, mod.rs:224-229
  const uint32_t depth = 1u << P.block_bits;
  uint32_t n_out = 0;
  for (uint32_t key = 0; key < (1u << P.bucket_bits); ++key) {
    const uint32_t n = num[key], visible = n < depth ? n : depth;
    for (uint32_t i = 0; i < visible; ++i, ++n_out) {
      const uint32_t slot = (key << P.block_bits) | ((n - 1u - i) & (depth - 1u));
      entries[2 * (size_t)n_out] = slot;
      entries[2 * (size_t)n_out + 1] = buckets[slot];
    }
  }
  *n_entries = n_out;
}

// the images of a group: image j filed on table j % J.tables of the job, which the parse behind it takes over, as on the device
void lz77_batch_dict_images(const BatchParseJob& J, uint32_t n_images, const BatchImagePlan* plan, uint16_t* num, uint32_t* entries,
                            uint32_t* n_entries) {
  if (n_images == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  const size_t keys_per_table = (size_t)1 << J.P.bucket_bits;
  const uint32_t depth = 1u << J.P.block_bits;
  for (uint32_t j = 0; j < n_images; ++j) {
    const uint32_t b = j % J.tables, D = plan[j].bytes;
    LiveRing lr;
    lr.num = J.num + (size_t)b * keys_per_table;
    lr.buckets = J.buckets + (((size_t)b * keys_per_table) << J.P.block_bits);
    lr.keys = J.keys + plan[j].text_at;
    lr.bits = J.P.block_bits;
    br_live_reset(lr, J.P.bucket_bits);
    if (D > J.P.htl - 1) br_live_store(lr, 0, 1, D - (J.P.htl - 1), 1, 0);  // StoreLookaheadThenStore, mod.rs:224-229
    uint32_t* out = entries + 2 * (size_t)plan[j].entries_at;
    uint32_t n_out = 0;
    for (uint32_t key = 0; key < keys_per_table; ++key) {
      const uint32_t n = lr.num[key], visible = n < depth ? n : depth;
      num[(size_t)j * keys_per_table + key] = (uint16_t)n;
      for (uint32_t i = 0; i < visible && n_out < D; ++i, ++n_out) {
        const uint32_t slot = (key << J.P.block_bits) | ((n - 1u - i) & (depth - 1u));
        out[2 * (size_t)n_out] = slot;
        out[2 * (size_t)n_out + 1] = lr.buckets[slot];
      }
    }
    n_entries[j] = n_out;
  }
}

void lz77_batch_gather(const BatchParseJob& J, const uint32_t* offsets, Command* out) {
  for (uint32_t i = 0; i < J.n_items; ++i) {
    const BatchRecord& r = J.records[i];
    if (r.overflow || r.n_cmds > J.items[i].cmd_cap) continue;
    for (uint32_t c = 0; c < r.n_cmds; ++c) out[offsets[i] + c] = br_batch_command(J, J.items[i], r, c);
  }
}

}  // namespace brotli_mi355x
