// batch_quick_device.h -- the item code of k_quick_batch (batch_quick.h): one item of a batch at quality 2 .. 4, parsed by one
// chain of br_quick_block on a table of its own and closed as the one meta-block of a stream of one block.  Shared by the gfx950
// kernel (quick_kernels.hip) and the host emulation (batch_quick_emu.inc).
#ifndef BROTLI_MI355X_BATCH_QUICK_DEVICE_H_
#define BROTLI_MI355X_BATCH_QUICK_DEVICE_H_

#include "batch_quick.h"
#include "quick_device.h"
#include "batch_item_device.h"

namespace brotli_mi355x {

// A fresh hasher on a table that the item in front has used: every slot 0 -- the reference relies on zeroed slots
// (encode.rs:1147), a zero slot is the candidate "position 0" -- and the two throttle books behind the slots 0 / 0.  The whole
// wavefront writes 16 bytes per lane and step; the chain reads its table through device-scope loads (q_get), so the fill is
// made visible at device scope and the wavefront waits for it before the first of them.
BR_DEV void br_quick_batch_zero(uint32_t* table, uint32_t words /* a multiple of 16 */) {
  BR_SYNC();
  br_batch_fill16(table, words >> 2, 0u);
#if !BR_SCALAR
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

// The hasher as HasherPrependCustomDictionary leaves it for a dictionary of the item's own (text: its D bytes), on a table that
// br_quick_batch_zero has just emptied: the prepend files the positions 0 .. D - kQuickHtl in ascending order, so what a slot ends
// up with is the LARGEST position filed under it (k_quick_prepend relies on the same).  The wavefront files 64 consecutive
// positions per step, one per lane, with a device-scope atomic maximum whose result nobody reads; lanes of one step that meet in a
// slot (runs, periodic text) are settled by the maximum, whatever their order.  Every 8-byte load ends inside the dictionary.
// Made visible like the zero fill: q_get and the book loads of br_quick_block are device-scope loads.
BR_DEV void br_quick_batch_file(const QuickJob& Q, const uint8_t* text, uint32_t D) {
#if BR_SCALAR
  br_quick_prepend(Q, text, D);
#else
  if (D >= kQuickHtl) {
    const uint32_t count = D - (kQuickHtl - 1u);
    for (uint32_t i = (uint32_t)BR_LANE; i < count; i += BR_NLANES) {
      const uint64_t v = (br_load64(text + i) << (64u - 8u * Q.hash_len)) * kQuickHashMul64;
      const uint32_t key = (uint32_t)(v >> (64u - Q.bucket_bits));
      atomicMax(Q.table + key + ((i >> 3) & (Q.sweep - 1u)), i);
    }
  }
  __threadfence();
#endif
  BR_SYNC();
}

// The job of one item on table `table`, in item-local coordinates: position 0 is the item's first byte (D == 0), so no distance
// reaches a neighbour and max_backward is what the reference computes for a stream that starts at 0; behind a custom dictionary
// position 0 is the dictionary's first byte and the item starts at D, as in the reference's ring buffer.  Known here, whatever
// the job says: D bytes of custom dictionary in front of the item and no other prefix (matches may not straddle its end:
// q_fix_len), the literal-spree window of qualities below 9, five hashed bytes (H2, H3, H4) -- constants the compiler folds,
// registers the chain does not hold.  P.ring_mask stays the job's: at lgwin <= 14 an item of three or four blocks passes the ring
// buffer's first lap, where q_byte reads the byte of one lap earlier and StoreRange files ring-buffer indices.
BR_DEV void br_quick_batch_job(const QuickBatchJob& J, uint32_t table, uint32_t D, uint32_t bytes, QuickJob& Q, Lz77Params& P) {
  Q = J.Q;
  Q.table = J.Q.table + (size_t)table * quick_table_words(J.Q);
  Q.hash_len = 5;
  P = J.P;
  P.total_bytes = D + bytes;
  P.prefix_bytes = P.dict_break = D;
  P.spree_window = 64;
}

// T: the static-dictionary tables; logs: should_compress; histo: 256 words and exit_slot: one SegExit, both the wavefront's own
// (LDS on the device).
// kDict: the item's text starts with J.dict_bytes bytes of custom dictionary (BrotliMi355xCompressBatchWithDictionaryEx) and its
// chain starts on J.image.
// kDicts (with kDict): the dictionary is the item's own, J.item_dict_bytes[index] bytes (BrotliMi355xCompressBatchWithDictionaries);
// J.dict_bytes and J.image are not looked at.  The chain copies the image the group built of that dictionary
// (J.images, J.item_image[index]) over its table, or, where the dictionary has none, zeroes its table and files the dictionary itself.
template <bool kDict = false, bool kDicts = false>
BR_DEV void br_quick_batch_item(const QuickBatchJob& J, const QuickTables& T, const EntropyTables& logs, uint32_t* histo, SegExit* exit_slot,
                                uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  // (D + bytes stays inside the first lap of the ring: D < 1 << lgwin, bytes <= 1 << lgblock, the ring has 1 + max of the two bits)
  const uint32_t D = kDicts ? BR_UNIFORM(J.item_dict_bytes[index]) : (kDict ? BR_UNIFORM(J.dict_bytes) : 0u);
  QuickJob Q;
  Lz77Params P;
  br_quick_batch_job(J, table, D, it.bytes, Q, P);
  if constexpr (kDicts) {
    static_assert(kDict || !kDicts, "kDicts goes with kDict");
    // One table takes both starts in turn, behind dictionaries of any two lengths: the prime writes ALL words of the table, the
    // zero fill all of them too, so neither start sees a word of the item in front (or of another image).
    const uint32_t image = J.item_image != nullptr ? BR_UNIFORM(J.item_image[index]) : kBatchNoImage;  // (wave-uniform)
    if (image != kBatchNoImage) {
      br_quick_batch_prime(Q.table, J.images + (size_t)image * quick_table_words(Q), quick_table_words(Q));
    } else {
      br_quick_batch_zero(Q.table, quick_table_words(Q));
      br_quick_batch_file(Q, J.text + it.text_off - D, D);
    }
  } else if constexpr (kDict) {
    br_quick_batch_prime(Q.table, J.image, quick_table_words(Q));
  } else {
    br_quick_batch_zero(Q.table, quick_table_words(Q));
  }
  // The last searched position is bytes - 9 (its lazy successor bytes - 8): the 8-byte loads of q_key end inside the item, the
  // 16-byte loads of br_match_len_wide inside its padding.
  const uint8_t* text = J.text + it.text_off - D;
  Segment seg;
  seg.start = seg.blk_start = D;
  seg.end = seg.blk_end = D + it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
  SegEntry entry = br_stream_start_entry(P.spree_window);
  entry.pos = D;
  // (with a dictionary br_quick_block files the last three dictionary positions itself: StitchToPreviousBlock, mod.rs:210-222,
  // and counts the copies of one byte that a match cut at the dictionary's end leaves)
  br_quick_block(Q, P, T, text, seg, entry, J.slabs + (size_t)it.cmd_base, exit_slot);
  BR_SYNC();  // (lane 0 wrote the exit)
  br_batch_close_record(J.records + index, logs, histo, text, D, it, BR_UNIFORM(exit_slot->n_cmds), BR_UNIFORM(exit_slot->n_lits),
                        BR_UNIFORM(exit_slot->insert_len), kDict ? exit_slot->bad_commands : 0u);
}

// ---- items of several blocks (k_quick_batch_long) -------------------------------------------------------------------------------
// One item of two to kBatchLongBlocks input blocks: br_quick_block for every block of a stream that starts at 0, on the item's own
// table, and between the blocks the books of the host resolver (Lz77Stage::Resolve under RunQuick), kept by BatchLongBooks
// (batch_item_device.h).  What is this route's own: the outcome of a block is read from its SegExit behind a barrier,
// br_quick_block stitches to the block in front and extends the last command itself (there is no kSegTailStitched and no
// br_live_store), the dictionary books travel in the table, and below quality 4 the flush rule counts literals + commands.
BR_DEV void br_quick_batch_item_long(const QuickBatchJob& J, BatchLongRecord* records, const QuickTables& T, const EntropyTables& logs, uint32_t* histo,
                                     SegExit* exit_slot, uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  QuickJob Q;
  Lz77Params P;
  br_quick_batch_job(J, table, 0, it.bytes, Q, P);
  br_quick_batch_zero(Q.table, quick_table_words(Q));
  const uint8_t* text = J.text + it.text_off;
  Command* slab = J.slabs + (size_t)it.cmd_base;
  SegEntry entry = br_stream_start_entry(P.spree_window);
  BatchLongBooks b = br_books_open();
  for (uint32_t bs = 0; br_books_more(b, it, bs);) {
    const uint32_t be = br_books_block_end(P, it, bs);
    Segment seg;
    seg.start = seg.blk_start = bs;
    seg.end = seg.blk_end = be;
    seg.flags = kSegFirstInBlock | kSegLastInBlock;
    seg.cmd_base = it.cmd_base + b.used;
    seg.block_index = 0;
    seg.cmd_cap = it.cmd_cap - b.used;
    // (a block of n bytes leaves at most n / 2 commands; the slab holds bytes / 2 + 8, so the block's commands fit whatever the
    // blocks in front left -- br_books_take checks that before anything reads them)
    br_quick_block(Q, P, T, text, seg, entry, slab + b.used, exit_slot);
    BR_SYNC();  // (lane 0 wrote the exit)
    BatchBlockOutcome x;
    x.n_cmds = BR_UNIFORM(exit_slot->n_cmds);
    x.n_lits = BR_UNIFORM(exit_slot->n_lits);
    x.insert_len = BR_UNIFORM(exit_slot->insert_len);
    x.ext_len = BR_UNIFORM(exit_slot->ext_len);
    x.last_dist_code = BR_UNIFORM(exit_slot->last_dist_code);
    x.last_copy_len = BR_UNIFORM(exit_slot->last_copy_len);
    for (int i = 0; i < 4; ++i) x.cache[i] = (int32_t)BR_UNIFORM((uint32_t)exit_slot->cache[i]);
    if (!br_books_take(b, slab, it, x)) break;
    br_books_close(b, P, logs, histo, text, it, be, /*count_rule=*/P.quality < 4 /* MIN_QUALITY_FOR_BLOCK_SPLIT */, x.cache, records + index);
    br_books_next(b, P, be, x.cache, entry);  // (the rest of the entry stays the stream's first)
    BR_SYNC();  // (the exit slot is read; the next block writes it again)
    bs = be;
  }
  br_books_finish(b, records + index);
}

}  // namespace brotli_mi355x
#endif

