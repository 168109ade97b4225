// batch_greedy_device.h -- the item code of k_parse_batch (batch_greedy.h): one item of a batch, parsed by one live chain on a
// table of its own and closed as the one meta-block of a stream of one block.  Shared by the gfx950 kernel and the host emulation.
#ifndef BROTLI_MI355X_BATCH_GREEDY_DEVICE_H_
#define BROTLI_MI355X_BATCH_GREEDY_DEVICE_H_

#include "batch_greedy.h"
#include "lz77_chain.h"
#include "batch_item_device.h"

namespace brotli_mi355x {

// Replays the dictionary image on the table of a chain (BatchDictImage): the ring counters of the image go over ALL the counters of
// the table, then every entry they cover is written to its slot -- independent stores, through the device-scope macros the chain
// reads back through.  A table is reused by the next item of its wavefront, and the buckets keep what the item in front filed;
// none of it can be reached: a walk reads the min(counter, depth) slots in front of a key's counter and nothing else, every counter
// is the image's after the first loop, and the image's list holds exactly those slots of every key.  (What the chain files
// afterwards moves a counter one slot at a time and writes that slot first, br_live_insert / br_live_store.)
BR_DEV void br_batch_replay_dictionary(const LiveRing& lr, const BatchDictImage& d, uint32_t bucket_bits) {
  BR_SYNC();
  const uint32_t words = 1u << (bucket_bits - 1);  // two counters per 32-bit word
  const uint32_t* img = (const uint32_t*)d.num;
  uint32_t* w = (uint32_t*)lr.num;
  for (uint32_t i = BR_LANE; i < words; i += BR_NLANES) BR_LIVE_ST32(w + i, img[i]);
  uint32_t n = BR_UNIFORM(*d.n_entries);
  if (n > d.bytes) n = d.bytes;  // (at most one entry per filed position: the list's capacity)
  // four entries per lane and step: the loads of a step are in flight together, and so are its stores
  for (uint32_t i = 4u * (uint32_t)BR_LANE; i < n; i += 4u * BR_NLANES) {
    uint32_t slot[4], pos[4];
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t e = i + k < n ? i + k : i;
      slot[k] = d.entries[2 * (size_t)e];
      pos[k] = d.entries[2 * (size_t)e + 1];
    }
    for (uint32_t k = 0; k < 4; ++k)
      if (i + k < n) BR_LIVE_ST32(lr.buckets + slot[k], pos[k]);
  }
  BR_SYNC();
}

// A dictionary per item: the image item `index` replays, or kBatchNoImage -- its chain files its dictionary itself.  The same for
// every lane, so the item code branches wave-uniformly.
BR_DEV uint32_t br_batch_item_image(const BatchParseJob& J, uint32_t index) {
  return J.item_image != nullptr ? BR_UNIFORM(J.item_image[index]) : kBatchNoImage;
}
template <typename T>
BR_DEV const T* br_batch_uniform_ptr(const T* p) {
#if BR_SCALAR
  return p;
#else
  const uint64_t v = (uint64_t)(uintptr_t)p;
  return (const T*)(uintptr_t)(((uint64_t)BR_UNIFORM((uint32_t)(v >> 32)) << 32) | (uint64_t)BR_UNIFORM((uint32_t)v));
#endif
}
// image `image` of the group's array, its fields the same in every lane
BR_DEV BatchDictImage br_batch_load_image(const BatchDictImage* images, uint32_t image) {
  BatchDictImage d = images[image];
  d.bytes = BR_UNIFORM(d.bytes);
  d.num = br_batch_uniform_ptr(d.num);
  d.entries = br_batch_uniform_ptr(d.entries);
  d.n_entries = br_batch_uniform_ptr(d.n_entries);
  return d;
}

// Item-local coordinates on table `table`: position 0 of t.text / t.keys / t.flags_next lies D bytes in front of the item, and lr
// is the table's bucket rings.  D == 0: position 0 is the item's first byte, so no distance reaches a neighbour and max_backward
// is what the reference computes for a stream that starts at 0.  With a dictionary position 0 is the dictionary's first byte and
// the item starts at D, as in the reference's ring buffer.
BR_DEV void br_batch_item_tables(const BatchParseJob& J, const Lz77Params& P, const BatchItem& it, uint32_t D, uint32_t table, ChainTables& t, LiveRing& lr) {
  t.text = J.text + it.text_off - D;
  t.keys = J.keys + it.text_off - D;
  t.flags_next = J.flags + it.text_off - D;
  t.cmds = J.slabs;
  const size_t keys_per_table = (size_t)1 << P.bucket_bits;
  lr.num = J.num + (size_t)table * keys_per_table;
  lr.buckets = J.buckets + (((size_t)table * keys_per_table) << P.block_bits);
  lr.keys = t.keys;
  lr.bits = P.block_bits;
}

// T: the job's tables with text / keys / flags / cmds still pointing at the group's arrays.
// kDict: the item's text starts with J.dict.bytes bytes of custom dictionary (BrotliMi355xCompressBatchWithDictionary).
// kDicts (with kDict): a dictionary per item (BrotliMi355xCompressBatchWithDictionaries) -- the item's text starts with
// J.item_dict_bytes[index] bytes of its own dictionary, J.dict is not looked at, and the chain replays the image of that
// dictionary (J.images[J.item_image[index]], built for the group: lz77_batch_dict_images) or, where the dictionary has none, files
// it itself.  A parameter of the template, not a test of J.item_dict_bytes, so that the instances of the other calls stay what
// they were.
//
// One table serves replayed and self-filed items in turn, behind dictionaries of any two lengths, and it served as the scratch of
// an image build before the first of them.  Whatever was there cannot be reached, because both starts leave EVERY counter of the
// table defined and every slot a counter covers written by this item's own start: the replay writes all 1 << bucket_bits counters
// from the image and then exactly the min(counter, depth) slots in front of each (the image's list, also where it is empty: a
// dictionary shorter than the hashed length has all counters 0); the reset zeroes all counters, and the filing behind it writes
// its slot before it moves its counter.  From there on the chain does the same, whichever start it had.
//
// The table under kDicts is reused by the next item of its wavefront with only its counters emptied (br_live_reset), and that item's
// dictionary may be shorter or longer than the one in front -- 2 bytes behind 65 536, say.  Nothing the item in front left can be
// reached, by the argument above br_batch_replay_dictionary and br_batch_item_h9: a walk over a key reads the min(counter, depth)
// slots in front of the key's counter and nothing else; every counter is 0 after the reset, and every filing -- the dictionary's
// by br_live_store, the three stitched positions, the chain's own -- writes its slot before it moves the counter on by one.  So
// every slot in reach was written by THIS item, whatever the length of its dictionary or of the one before.  (A key filed 65 536
// times wraps its u16 counter to 0 with the whole ring written by this item: br_batch_item_h9.  Dictionary + item stay below that.)
template <bool kRows, bool kDict = false, bool kDicts = false>
BR_DEV void br_batch_item(const BatchParseJob& J, const ChainTables& T, ChainScratchT<false, kRows>& s, uint32_t* histo /* 256 words */,
                          uint32_t index, uint32_t table) {
  static_assert(kDict || !kDicts, "a dictionary per item is a dictionary");
  const BatchItem it = br_batch_load_item(J.items, index);
  const uint32_t D = kDicts ? BR_UNIFORM(J.item_dict_bytes[index]) : (kDict ? BR_UNIFORM(J.dict.bytes) : 0u);
  Lz77Params P = J.P;
  P.total_bytes = D + it.bytes;
  if constexpr (kDict) P.prefix_bytes = P.dict_break = D;
  ChainTables t = T;
  LiveRing lr;
  br_batch_item_tables(J, P, it, D, table, t, lr);
  // an empty hasher: the ring counters at 0 (a walk never reads a slot its counter does not cover: `buckets` needs no fill)
  if constexpr (kDict) {
    // the hasher as HasherPrependCustomDictionary left it, then StitchToPreviousBlock of the first block (mod.rs:210-222): the
    // last three dictionary positions, whose four bytes reach into the item
    const uint32_t image = kDicts ? br_batch_item_image(J, index) : kBatchNoImage;  // (wave-uniform)
    if (!kDicts && J.dict.entries != nullptr) {
      br_batch_replay_dictionary(lr, J.dict, P.bucket_bits);
    } else if (kDicts && image != kBatchNoImage) {
      br_batch_replay_dictionary(lr, br_batch_load_image(J.images, image), P.bucket_bits);
    } else {
      // (the A/B of DESIGN.md section 10, BROTLI_MI355X_BATCH_DICT_SELF_FILE, and the items of kDicts whose dictionary has no
      // image: the chain files the dictionary itself, wave-wide, in the reference's order)
      br_live_reset(lr, P.bucket_bits);
      if (D > P.htl - 1) br_live_store(lr, 0, 1, D - (P.htl - 1), 1, 0);
    }
    if (it.bytes >= P.htl - 1 && D >= 3) br_live_store(lr, D - 3u, 1, 3, 1, 0);
  } else {
    br_live_reset(lr, P.bucket_bits);
  }
  Segment seg;
  seg.start = seg.blk_start = D;
  seg.end = seg.blk_end = D + it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
  SegEntry entry = br_stream_start_entry(P.spree_window);
  entry.pos = D;
  SegExit left;
  SegEntry next;
  BlockTail tail;
  br_parse_segment<false, kRows, true>(P, t, s, seg, entry, left, next, &lr, &tail);
  // (lane 0 holds the exit)
  br_batch_close_record(J.records + index, t.logs, histo, t.text, D, it, tail.n_cmds, tail.n_lits, tail.insert_len, kDict ? left.bad_commands : 0u);
}

#if !BR_SCALAR
// the group's arrays and the device's static-dictionary and entropy tables as a batch chain takes them (lz77_kernels.hip)
ChainTables batch_chain_tables(const BatchParseJob& J);
#endif

// ---- qualities 9 and 10 (k_parse_batch_h9,BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS) --------------------------------------------------
// br_batch_item without a dictionary on the H9 hasher: 1 << 15 keys, rings 256 deep, sixteen cache distances, the H9 scores, the
// static dictionary behind H9's own throttle.  The chain is the first br_parse_segment<true, false, true>: it reads the rings of its
// private table (probe_pair's non-rows live path: every ring entry in reach has its text looked at, the table keeps no tags) and
// files with plain Store in ascending order -- J.P.masked_from is kNeverMasked, so br_live_store_copy masks nothing.
//
// The table is reused by the next item of its wavefront with only its counters emptied (br_live_reset).  What the item in front
// left in the buckets cannot be reached, at this depth and with u16 counters as at the others: a walk over key k reads the
// min(num[k], 256) slots in front of num[k] and nothing else; num[k] is 0 after the reset and every filing writes slot num[k] & 255
// before it moves the counter on by one, so while the counter has not wrapped those slots are the item's own last filings.  A counter
// that wraps at 65 536 filings (one key filed that often: a run of one byte) comes back to 0 with all 256 slots of the ring
// written by this item, 256 times over, and goes on from there exactly as after the reset -- the reference's own u16 arithmetic,
// under which such a key shows no candidate until it is filed again.  Either way a walk never sees a slot this item did not write.
BR_DEV void br_batch_item_h9(const BatchParseJob& J, const ChainTables& T, ChainScratchT<true, false>& s, uint32_t* histo /* 256 words */,
                             uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  Lz77Params P = J.P;
  P.total_bytes = it.bytes;
  ChainTables t = T;
  LiveRing lr;
  br_batch_item_tables(J, P, it, 0, table, t, lr);
  br_live_reset(lr, P.bucket_bits);
  Segment seg;
  seg.start = seg.blk_start = 0;
  seg.end = seg.blk_end = it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
  const SegEntry entry = br_stream_start_entry(P.spree_window);
  SegExit left;
  SegEntry next;
  BlockTail tail;
  br_parse_segment<true, false, true>(P, t, s, seg, entry, left, next, &lr, &tail);
  br_batch_close_record(J.records + index, t.logs, histo, t.text, 0, it, tail.n_cmds, tail.n_lits, tail.insert_len, 0u);
}

// command i of item `index` as the meta-block stage wants it
BR_DEV Command br_batch_command(const BatchParseJob& J, const BatchItem& it, const BatchRecord& r, uint32_t i) {
  if (r.trailing != 0 && i + 1 == r.n_cmds) return br_insert_only_command(r.trailing);
  return br_finish_command(J.slabs[(size_t)it.cmd_base + i], J.P.num_direct_distance_codes, J.P.dist_postfix_bits);
}

// ---- items of several blocks (k_parse_batch_long) -------------------------------------------------------------------------------
// One item of two to kBatchLongBlocks input blocks: what br_parse_live does for the blocks [0, n) of a stream that starts at 0, and at
// the item's end what br_batch_item does for its only block.  The chain is the only writer of its slab, so extend_last_command
// and the literals pending at a block's entry are applied to its own raw commands in place (the host resolver's CmdPatch kinds 0
// and 2), a block's commands start where the block in front stopped, and every meta-block the flush rule closes leaves a record.
// The books between the blocks are the steps of BatchLongBooks (batch_item_device.h: br_books_take, br_books_close, br_books_next,
// br_books_finish), written out here in that order: behind the shared steps k_parse_batch_long<false> compiled to 92 VGPRs
// instead of 107 and ran 1 to 2 % slower on 128 and 256 KiB items (profiles/r18_batch_item_code.json), so
// this call site stays as it was.  A rule changed there is changed here.
template <bool kRows>
BR_DEV void br_batch_item_long(const BatchParseJob& J, BatchLongRecord* records, const ChainTables& T, ChainScratchT<false, kRows>& s,
                               uint32_t* histo /* 256 words */, uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  Lz77Params P = J.P;
  P.total_bytes = it.bytes;
  ChainTables t = T;
  t.text = J.text + it.text_off;
  t.keys = J.keys + it.text_off;
  t.flags_next = J.flags + it.text_off;
  t.cmds = J.slabs;
  LiveRing lr;
  const size_t keys_per_table = (size_t)1 << P.bucket_bits;
  lr.num = J.num + (size_t)table * keys_per_table;
  lr.buckets = J.buckets + (((size_t)table * keys_per_table) << P.block_bits);
  lr.keys = t.keys;
  lr.bits = P.block_bits;
  br_live_reset(lr, P.bucket_bits);
  Command* slab = J.slabs + (size_t)it.cmd_base;
  SegEntry entry = br_stream_start_entry(P.spree_window);
  // the books of the open meta-block (LiveBlockState) and of the slab
  uint32_t mb_start = 0, mb_cmds = 0, mb_lits = 0, mb_first_cmd = 0;
  uint32_t last_valid = 0, last_dist_code = 0, last_copy_len = 0;
  int32_t saved_cache[4] = {4, 11, 15, 16};  // the distance cache at the start of the open meta-block
  uint32_t carry = 0;                        // literals pending at the entry of the block
  uint32_t used = 0;                         // raw commands in the slab so far
  uint32_t n_mb = 0, overflow = 0;
  const uint32_t max_mb = P.max_metablock_bytes, limit = max_mb / 8;
  for (uint32_t bs = 0; bs < it.bytes && n_mb < kBatchLongBlocks;) {
    const uint32_t be = it.bytes - bs > P.block_bytes ? bs + P.block_bytes : it.bytes;
    const bool last = be == it.bytes;
    // StitchToPreviousBlockInternal (mod.rs:210-222) of the block behind this one: what kSegTailStitched stands for
    const bool stitched = !last && it.bytes - be >= P.htl - 1 && be >= 3;
    Segment seg;
    seg.start = seg.blk_start = bs;
    seg.end = seg.blk_end = be;
    seg.flags = kSegFirstInBlock | kSegLastInBlock | (stitched ? kSegTailStitched : 0u);
    seg.cmd_base = it.cmd_base + used;
    seg.block_index = 0;
    seg.cmd_cap = it.cmd_cap - used;
    SegExit left;
    SegEntry next;
    BlockTail tail;
    br_parse_segment<false, kRows, true>(P, t, s, seg, entry, left, next, &lr, &tail);
    if (tail.n_cmds > seg.cmd_cap) {
      overflow = 1;
      break;
    }
    if (stitched) br_live_store(lr, be - 3u, 1, 3, 1, 0);
    // ---- the books, as in br_parse_live; the fix-ups go into the slab
    if (BR_LANE == 0) {
      if (tail.ext_len != 0 && last_valid) slab[used - 1].copy_len_ += tail.ext_len;  // (its copy code is its length: no dictionary word is extended)
      if (tail.n_cmds != 0 && carry != 0) slab[used].insert_len_ += carry;
    }
    if (tail.ext_len != 0 && last_valid) last_copy_len += tail.ext_len;
    mb_cmds += tail.n_cmds;
    mb_lits += tail.n_lits;
    if (tail.n_cmds != 0) {
      mb_lits += carry;
      carry = tail.insert_len;
      last_valid = 1;
      last_dist_code = tail.last_dist_code;
      last_copy_len = tail.last_copy_len;
    } else {
      carry += tail.insert_len;
    }
    used += tail.n_cmds;
    const bool next_fits = (uint64_t)(be - mb_start) + P.block_bytes <= (uint64_t)max_mb;
    if (last || !(next_fits && mb_lits < limit && mb_cmds < limit)) {  // the meta-block is closed here
      const uint32_t bytes = be - mb_start;
      const uint32_t cmds_all = mb_cmds + (carry != 0 ? 1u : 0u), lits_all = mb_lits + carry;  // with the trailing insert-only command
      const bool compress = br_should_compress(t.logs, histo, t.text, mb_start, be, cmds_all, lits_all);
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
        for (int i = 0; i < 4; ++i) next.cache[i] = saved_cache[i];
      for (int i = 0; i < 4; ++i) saved_cache[i] = next.cache[i];
      mb_start = be;
      mb_cmds = mb_lits = 0;
      mb_first_cmd = used;
      last_valid = 0;
      carry = 0;  // (pending literals went into its trailing insert-only command)
    }
    // ---- the entry of the next block
    const uint32_t was_exact = entry.dict_exact;
    entry = next;
    entry.pos = be;
    entry.insert_len = carry;
    entry.dict_exact = was_exact;
    entry.head_kind = kHeadNone;
    entry.head_base = entry.head_p1 = 0;
    entry.ext_allowed = 0;
    if (mb_cmds != 0 && carry == 0 && last_valid) {
      const uint64_t cmd_dist = (uint64_t)(int64_t)next.cache[0];
      if (last_dist_code < 16 || (uint64_t)last_dist_code - 15 == cmd_dist) {
        const uint64_t lpp = (uint64_t)be - last_copy_len;
        const uint64_t max_distance = lpp < P.max_backward_limit ? lpp : P.max_backward_limit;
        if (cmd_dist <= max_distance) entry.ext_allowed = 1;
      }
    }
    BR_SYNC();
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

// command i of meta-block m of an item, as the meta-block stage wants it: its raw commands, then its trailing insert-only command
BR_DEV Command br_batch_long_command(const BatchParseJob& J, const BatchItem& it, const BatchLongMetaBlock& m, uint32_t i) {
  if (i >= m.n_cmds) return br_insert_only_command(m.trailing);
  return br_finish_command(J.slabs[(size_t)it.cmd_base + m.first_cmd + i], J.P.num_direct_distance_codes, J.P.dist_postfix_bits);
}

}  // namespace brotli_mi355x
#endif
