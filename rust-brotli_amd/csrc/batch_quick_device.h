// batch_quick_device.h -- the item code of k_quick_batch (batch_quick.h): one item of a batch at quality 2 .. 4, parsed by one
// chain of br_quick_block on a table of its own and closed as the one meta-block of a stream of one block.  Shared by the gfx950
// kernel (quick_kernels.hip) and the host emulation (batch_quick_emu.inc).
#ifndef BROTLI_MI355X_BATCH_QUICK_DEVICE_H_
#define BROTLI_MI355X_BATCH_QUICK_DEVICE_H_

#include "batch_quick.h"
#include "quick_device.h"

namespace brotli_mi355x {

// A fresh hasher on a table that the item in front has used: every slot 0 -- the reference relies on zeroed slots
// (encode.rs:1147), a zero slot is the candidate "position 0" -- and the two throttle books behind the slots 0 / 0.  The whole
// wavefront writes 16 bytes per lane and step; the chain reads its table through device-scope loads (q_get), so the fill is
// made visible at device scope and the wavefront waits for it before the first of them.
BR_DEV void br_quick_batch_zero(uint32_t* table, uint32_t words /* a multiple of 16 */) {
  BR_SYNC();
#if BR_SCALAR
  memset(table, 0, (size_t)words * 4);
#else
  uint4* w = (uint4*)table;
  const uint32_t quads = words >> 2;
  for (uint32_t i = (uint32_t)BR_LANE; i < quads; i += BR_NLANES) w[i] = make_uint4(0u, 0u, 0u, 0u);
  __threadfence();
#endif
  BR_SYNC();
}

// The hasher as HasherPrependCustomDictionary left it, on a table that the item in front has used: the image of the call
// (QuickBatchJob::image -- what the prepend leaves hangs on the dictionary alone) goes over ALL words of the table, the books
// included.  16 bytes per lane and step, four steps in flight: the loads of a round are issued together, then its stores.  The
// image is read-only for the launch (plain loads; it stays in the L2); the copy is made visible as the zero fill is.
BR_DEV void br_quick_batch_prime(uint32_t* table, const uint32_t* image, uint32_t words /* a multiple of 16 */) {
  BR_SYNC();
#if BR_SCALAR
  memcpy(table, image, (size_t)words * 4);
#else
  uint4* w = (uint4*)table;
  const uint4* src = (const uint4*)image;
  const uint32_t quads = words >> 2;
  for (uint32_t i = (uint32_t)BR_LANE; i < quads; i += 4u * BR_NLANES) {
    const uint32_t i1 = i + BR_NLANES, i2 = i + 2u * BR_NLANES, i3 = i + 3u * BR_NLANES;
    const uint4 v0 = src[i];
    const uint4 v1 = src[i1 < quads ? i1 : i];
    const uint4 v2 = src[i2 < quads ? i2 : i];
    const uint4 v3 = src[i3 < quads ? i3 : i];
    w[i] = v0;
    if (i1 < quads) w[i1] = v1;
    if (i2 < quads) w[i2] = v2;
    if (i3 < quads) w[i3] = v3;
  }
  __threadfence();
#endif
  BR_SYNC();
}

// T: the static-dictionary tables; logs: should_compress; histo: 256 words and exit_slot: one SegExit, both the wavefront's own
// (LDS on the device).
// kDict: the item's text starts with J.dict_bytes bytes of custom dictionary (BrotliMi355xCompressBatchWithDictionaryEx) and its
// chain starts on J.image.
template <bool kDict = false>
BR_DEV void br_quick_batch_item(const QuickBatchJob& J, const QuickTables& T, const EntropyTables& logs, uint32_t* histo, SegExit* exit_slot,
                                uint32_t index, uint32_t table) {
  BatchItem it = J.items[index];
  it.text_off = BR_UNIFORM(it.text_off);
  it.bytes = BR_UNIFORM(it.bytes);
  it.cmd_base = BR_UNIFORM(it.cmd_base);
  it.cmd_cap = BR_UNIFORM(it.cmd_cap);
  QuickJob Q = J.Q;
  const uint32_t words = quick_table_words(Q);
  Q.table = J.Q.table + (size_t)table * words;
  if constexpr (kDict) {
    br_quick_batch_prime(Q.table, J.image, words);
  } else {
    br_quick_batch_zero(Q.table, words);
  }
  // item-local coordinates: position 0 is the item's first byte, so no distance reaches a neighbour and max_backward is what
  // the reference computes for a stream that starts at 0.  The last searched position is bytes - 9 (its lazy successor
  // bytes - 8): the 8-byte loads of q_key end inside the item, the 16-byte loads of br_match_len_wide inside its padding.
  // (with a dictionary: position 0 is the dictionary's first byte and the item starts at D, as in the reference's ring buffer;
  // D + bytes stays inside the first lap of the ring: D < 1 << lgwin, bytes <= 1 << lgblock, the ring has 1 + max of the two bits)
  const uint32_t D = kDict ? BR_UNIFORM(J.dict_bytes) : 0u;
  Lz77Params P = J.P;
  P.total_bytes = D + it.bytes;
  // known here, whatever the job says: without kDict no custom dictionary in front of an item, the literal-spree window of
  // qualities below 9, five hashed bytes (H2, H3, H4) -- constants the compiler folds, registers the chain does not hold
  // (with a dictionary matches may not straddle its end: q_fix_len; br_quick_block counts the copies of one byte that leaves)
  P.prefix_bytes = P.dict_break = D;
  P.spree_window = 64;
  Q.hash_len = 5;
  const uint8_t* text = J.text + it.text_off - D;
  Segment seg;
  seg.start = seg.blk_start = D;
  seg.end = seg.blk_end = D + it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
  SegEntry entry;
  entry.pos = D;
  entry.apply = P.spree_window;
  entry.cache[0] = 4;
  entry.cache[1] = 11;
  entry.cache[2] = 15;
  entry.cache[3] = 16;
  entry.insert_len = 0;
  entry.ext_allowed = 0;
  entry.dict_lookups = entry.dict_matches = 0;
  entry.ext_max_distance = 0;
  entry.dict_exact = 1;
  entry.head_kind = kHeadNone;
  entry.head_base = entry.head_p1 = 0;
  entry.pad = 0;
  // (with a dictionary br_quick_block files the last three dictionary positions itself: StitchToPreviousBlock, mod.rs:210-222)
  br_quick_block(Q, P, T, text, seg, entry, J.slabs + (size_t)it.cmd_base, exit_slot);
  BR_SYNC();  // (lane 0 wrote the exit)
  // ---- Lz77Stage::Resolve for the only block of a stream: the pending literals become the trailing insert-only command, and
  // should_compress (encode.rs:1325-1354) gives the verdict
  const uint32_t bytes = it.bytes;
  const uint32_t trailing = BR_UNIFORM(exit_slot->insert_len);
  const uint32_t raw_cmds = BR_UNIFORM(exit_slot->n_cmds), raw_lits = BR_UNIFORM(exit_slot->n_lits);
  const uint32_t cmds_all = raw_cmds + (trailing != 0 ? 1u : 0u), lits_all = raw_lits + trailing;
  bool compress = true;
  if (cmds_all < (bytes >> 8) + 2 && (float)lits_all > 0.99f * (float)bytes) {
    BR_SYNC();
    for (uint32_t i = BR_LANE; i < 256; i += BR_NLANES) histo[i] = 0;
    BR_SYNC();
    for (uint32_t q = 13u * (uint32_t)BR_LANE; q < bytes; q += 13u * BR_NLANES) BR_ATOMIC_INC(&histo[text[D + q]]);
    BR_SYNC();
    const float threshold = (float)bytes * 7.92f / 13.0f;
    compress = !(br_bits_entropy(logs, histo, 256) > threshold);
  }
  if (BR_LANE == 0) {
    BatchRecord r;
    r.n_cmds = cmds_all;
    r.n_lits = lits_all;
    r.trailing = trailing;
    r.uncompressed = compress ? 0u : 1u;
    r.overflow = cmds_all > it.cmd_cap ? 1u : 0u;
    r.bad_commands = 0;
    if constexpr (kDict) {
      // a copy of one byte: the reference cannot encode it (GetCopyLengthCode, command.rs:91-93) and neither do the tables behind
      // br_finish_command -- the item is handed on as literals only and flagged, as br_batch_item does
      r.bad_commands = exit_slot->bad_commands;
      if (r.bad_commands != 0) {
        r.n_cmds = 1;
        r.n_lits = r.trailing = bytes;
        r.uncompressed = 1;
        r.overflow = 0;
      }
    }
    r.pad[0] = r.pad[1] = 0;
    J.records[index] = r;
  }
  BR_SYNC();
}

// ---- items of several blocks (k_quick_batch_long) -------------------------------------------------------------------------------
// One item of two to kBatchLongBlocks input blocks: br_quick_block for every block of a stream that starts at 0, on the item's own
// table, and between the blocks the books of the host resolver (Lz77Stage::Resolve under RunQuick).  They are br_batch_item_long's,
// line by line, reading the SegExit where that code reads a BlockTail (a copy, not a shared helper: that function is inlined into
// k_parse_batch_long, whose code generation this leaves alone).  What differs: br_quick_block stitches to the block in front and
// extends the last command itself (there is no kSegTailStitched and no br_live_store), the dictionary books travel in the table,
// and below quality 4 a meta-block is also closed once it holds 0x2fff literals + commands (encode.rs:2458-2459) -- counted as the
// flush rule counts them, in front of the trailing insert-only command: literals pending behind the last command do not count yet.
BR_DEV void br_quick_batch_item_long(const QuickBatchJob& J, BatchLongRecord* records, const QuickTables& T, const EntropyTables& logs, uint32_t* histo,
                                     SegExit* exit_slot, uint32_t index, uint32_t table) {
  BatchItem it = J.items[index];
  it.text_off = BR_UNIFORM(it.text_off);
  it.bytes = BR_UNIFORM(it.bytes);
  it.cmd_base = BR_UNIFORM(it.cmd_base);
  it.cmd_cap = BR_UNIFORM(it.cmd_cap);
  QuickJob Q = J.Q;
  const uint32_t words = quick_table_words(Q);
  Q.table = J.Q.table + (size_t)table * words;
  br_quick_batch_zero(Q.table, words);
  // item-local coordinates, as in br_quick_batch_item.  P.ring_mask stays the job's: at lgwin <= 14 an item of three or four blocks
  // passes the ring buffer's first lap, where q_byte reads the byte of one lap earlier and StoreRange files ring-buffer indices
  Lz77Params P = J.P;
  P.total_bytes = it.bytes;
  P.prefix_bytes = P.dict_break = 0;
  P.spree_window = 64;
  Q.hash_len = 5;
  const uint8_t* text = J.text + it.text_off;
  Command* slab = J.slabs + (size_t)it.cmd_base;
  SegEntry entry;
  entry.pos = 0;
  entry.apply = P.spree_window;
  entry.cache[0] = 4;
  entry.cache[1] = 11;
  entry.cache[2] = 15;
  entry.cache[3] = 16;
  entry.insert_len = 0;
  entry.ext_allowed = 0;
  entry.dict_lookups = entry.dict_matches = 0;
  entry.ext_max_distance = 0;
  entry.dict_exact = 1;
  entry.head_kind = kHeadNone;
  entry.head_base = entry.head_p1 = 0;
  entry.pad = 0;
  // the books of the open meta-block and of the slab
  uint32_t mb_start = 0, mb_cmds = 0, mb_lits = 0, mb_first_cmd = 0;
  uint32_t last_valid = 0, last_dist_code = 0, last_copy_len = 0;
  int32_t saved_cache[4] = {4, 11, 15, 16};  // the distance cache at the start of the open meta-block
  uint32_t carry = 0;                        // literals pending at the entry of the block
  uint32_t used = 0;                         // raw commands in the slab so far
  uint32_t n_mb = 0, overflow = 0;
  const uint32_t max_mb = P.max_metablock_bytes, limit = max_mb / 8;
  const bool count_rule = P.quality < 4;  // MIN_QUALITY_FOR_BLOCK_SPLIT
  for (uint32_t bs = 0; bs < it.bytes && n_mb < kBatchLongBlocks;) {
    const uint32_t be = it.bytes - bs > P.block_bytes ? bs + P.block_bytes : it.bytes;
    const bool last = be == it.bytes;
    Segment seg;
    seg.start = seg.blk_start = bs;
    seg.end = seg.blk_end = be;
    seg.flags = kSegFirstInBlock | kSegLastInBlock;
    seg.cmd_base = it.cmd_base + used;
    seg.block_index = 0;
    seg.cmd_cap = it.cmd_cap - used;
    // (a block of n bytes leaves at most n / 2 commands; the slab holds bytes / 2 + 8, so the block's commands fit whatever the
    // blocks in front left -- `overflow` below is the check of that, made before anything reads them)
    br_quick_block(Q, P, T, text, seg, entry, slab + used, exit_slot);
    BR_SYNC();  // (lane 0 wrote the exit)
    const uint32_t x_cmds = BR_UNIFORM(exit_slot->n_cmds), x_lits = BR_UNIFORM(exit_slot->n_lits);
    const uint32_t x_insert = BR_UNIFORM(exit_slot->insert_len), x_ext = BR_UNIFORM(exit_slot->ext_len);
    const uint32_t x_dist_code = BR_UNIFORM(exit_slot->last_dist_code), x_copy_len = BR_UNIFORM(exit_slot->last_copy_len);
    int32_t next_cache[4];
    for (int i = 0; i < 4; ++i) next_cache[i] = (int32_t)BR_UNIFORM((uint32_t)exit_slot->cache[i]);
    if (x_cmds > seg.cmd_cap) {
      overflow = 1;
      break;
    }
    // ---- the books, as in br_batch_item_long; the fix-ups go into the slab
    if (BR_LANE == 0) {
      if (x_ext != 0 && last_valid) slab[used - 1].copy_len_ += x_ext;  // (its copy code is its length: no dictionary word is extended)
      if (x_cmds != 0 && carry != 0) slab[used].insert_len_ += carry;
    }
    if (x_ext != 0 && last_valid) last_copy_len += x_ext;
    mb_cmds += x_cmds;
    mb_lits += x_lits;
    if (x_cmds != 0) {
      mb_lits += carry;
      carry = x_insert;
      last_valid = 1;
      last_dist_code = x_dist_code;
      last_copy_len = x_copy_len;
    } else {
      carry += x_insert;
    }
    used += x_cmds;
    const bool should_flush = count_rule && mb_lits + mb_cmds >= 0x2fffu;
    const bool next_fits = (uint64_t)(be - mb_start) + P.block_bytes <= (uint64_t)max_mb && !should_flush;
    if (last || !(next_fits && mb_lits < limit && mb_cmds < limit)) {  // the meta-block is closed here
      const uint32_t bytes = be - mb_start;
      const uint32_t cmds_all = mb_cmds + (carry != 0 ? 1u : 0u), lits_all = mb_lits + carry;  // with the trailing insert-only command
      bool compress = true;
      if (cmds_all < (bytes >> 8) + 2 && (float)lits_all > 0.99f * (float)bytes) {
        BR_SYNC();
        for (uint32_t i = BR_LANE; i < 256; i += BR_NLANES) histo[i] = 0;
        BR_SYNC();
        for (uint32_t q = mb_start + 13u * (uint32_t)BR_LANE; q < be; q += 13u * BR_NLANES) BR_ATOMIC_INC(&histo[text[q]]);
        BR_SYNC();
        const float threshold = (float)bytes * 7.92f / 13.0f;
        compress = !(br_bits_entropy(logs, histo, 256) > threshold);
      }
      if (BR_LANE == 0) {
        BatchLongMetaBlock m;
        m.start = mb_start;
        m.bytes = bytes;
        m.first_cmd = mb_first_cmd;
        m.n_cmds = mb_cmds;
        m.n_lits = lits_all;
        m.trailing = carry;
        m.uncompressed = compress ? 0u : 1u;
        m.pad = 0;
        records[index].mb[n_mb] = m;
      }
      ++n_mb;
      // a stored meta-block hands the distance cache of its START to the next one (encode.rs:1994)
      if (!compress)
        for (int i = 0; i < 4; ++i) next_cache[i] = saved_cache[i];
      for (int i = 0; i < 4; ++i) saved_cache[i] = next_cache[i];
      mb_start = be;
      mb_cmds = mb_lits = 0;
      mb_first_cmd = used;
      last_valid = 0;
      carry = 0;  // (pending literals went into its trailing insert-only command)
    }
    // ---- the entry of the next block
    entry.pos = be;
    for (int i = 0; i < 4; ++i) entry.cache[i] = next_cache[i];
    entry.insert_len = carry;
    entry.ext_allowed = 0;
    if (mb_cmds != 0 && carry == 0 && last_valid) {
      const uint64_t cmd_dist = (uint64_t)(int64_t)next_cache[0];
      if (last_dist_code < 16 || (uint64_t)last_dist_code - 15 == cmd_dist) {
        const uint64_t lpp = (uint64_t)be - last_copy_len;
        const uint64_t max_distance = lpp < P.max_backward_limit ? lpp : P.max_backward_limit;
        if (cmd_dist <= max_distance) entry.ext_allowed = 1;
      }
    }
    BR_SYNC();  // (the exit slot is read; the next block writes it again)
    bs = be;
  }
  if (BR_LANE == 0) {
    records[index].n_mb = n_mb;
    records[index].overflow = overflow;
    records[index].bad_commands = 0;
    records[index].pad = 0;
  }
  BR_SYNC();
}

}  // namespace brotli_mi355x
#endif
