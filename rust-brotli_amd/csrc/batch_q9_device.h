// batch_q9_device.h -- the item code of BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (batch_greedy.h): one item of a batch at
// quality 9 behind a custom dictionary, parsed by one live H9 chain that starts at position D of `dictionary | item` on a private
// H9 table.  Shared by the gfx950 kernels (batch_q9_kernels.hip: k_parse_batch_h9_dict, k_parse_batch_h9_dicts) and the host
// emulation (batch_greedy_emu.inc).  A header of its own: batch_greedy_device.h and lz77_chain.h, which the parse kernels of
// lz77_kernels.hip include, stay what they were.
#ifndef BROTLI_MI355X_BATCH_Q9_DEVICE_H_
#define BROTLI_MI355X_BATCH_Q9_DEVICE_H_

#include "batch_greedy_device.h"

namespace brotli_mi355x {

// br_batch_item_h9 (batch_greedy_device.h) behind a dictionary: the hasher as HasherPrependCustomDictionary left it, then
// StitchToPreviousBlock of the first block, then br_parse_segment<true, false, true> from entry.pos = D with
// P.prefix_bytes = P.dict_break = D -- the order of br_batch_item<.., true, true>, on 1 << 15 keys with rings 256 deep.
//
// kDicts == false: the shared dictionary of the call (J.dict).  With an image (J.dict.entries != nullptr) the chain replays it over
// its table, br_batch_replay_dictionary; without one (BROTLI_MI355X_BATCH_DICT_SELF_FILE) it files the dictionary itself.
// kDicts == true: J.item_dict_bytes[index] bytes of the item's own dictionary.  Where the group has built an image of it
// (J.item_image[index], lz77_batch_dict_images) the chain replays that one; otherwise it files the dictionary wave-wide with
// br_live_store in the reference's order (ascending positions; lanes of one key take consecutive slots in position order).  A
// table takes both starts in turn: the paragraph on reuse below covers each, and neither relies on what the other left.
//
// Why a chain that starts at D on an H9 table is the reference's stream.  The host admits an item only with D <= 65536 and
// bytes <= 65536 (BatchQ9DictionaryEligible), and the ring buffer of a quality 9 stream has 1 << (1 + max(lgwin, lgblock)) >= 1 << 18
// bytes.  So D + bytes <= 131072, the first half of the smallest ring buffer:
//  - every position the prepend, the stitch or the chain files is its own ring-buffer index, P.masked_from is kNeverMasked and
//    nothing is filed masked; fix_unbroken_len's test on (prev & ring_mask) is the test on prev;
//  - H9's ring-end case (SearchResult::stored == false, br_fold_probe / br_search in lz77_chain.h) needs
//    (cur & ring_mask) + best_len > ring_mask.  best_len <= blk_end - cur and blk_end = D + bytes <= 131072 <= ring_mask, so
//    the case cannot come up, behind a dictionary no more than for the items of k_parse_batch_h9 that start at 0.  (The comment in
//    br_search that calls k_parse_batch_h9 the one kH9 live chain predates these two; this is the argument for them.)
//  - max_backward of a search at cur is min(cur, max_backward_limit) with cur counted from the dictionary's first byte, as in
//    the reference after the prepend; position 0 of t.text is that byte (br_batch_item_tables), so no distance reaches a neighbour.
//
// The table is reused by the next item of its wavefront, which lies behind another dictionary (kDicts) or the same image.  Nothing
// the item in front left can be reached.  A walk over key k reads the min(num[k], 256) slots in front of num[k] and nothing
// else.  kDicts / self-filing: num[k] is 0 after br_live_reset, and every filing -- the dictionary's by br_live_store, the three
// stitched positions, the chain's own -- writes slot num[k] & 255 before it moves the counter on by one, so the slots in reach
// are this item's own last filings, whatever the length of the dictionary in front.  The image: after the replay's first loop every
// counter is the image's, and the image lists exactly the min(num[k], 256) slots each counter covers; D <= 65536 files at most
// 65 533 positions, so no u16 counter of an image has wrapped and min(num[k], 256) is what the reference sees.
// The one way a counter wraps: a key filed 65 536 times within dictionary + item, which takes a run of one byte (65 536 equal
// bytes of dictionary file the key 65 533 times, the stitch three more, the item's first positions the rest).  The counter comes
// back to 0 with all 256 slots of the ring written by this item, 256 times over, and goes on exactly as after the reset: the
// reference's own u16 arithmetic, under which such a key shows no candidate until it is filed again.  65 536 is a multiple of
// 256, so slot (n + rank) & 255 of the wave-wide store is the slot the one-by-one store takes across the wrap.
template <bool kDicts>
BR_DEV void br_batch_item_h9_dict(const BatchParseJob& J, const ChainTables& T, ChainScratchT<true, false>& s, uint32_t* histo /* 256 words */,
                                  uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  const uint32_t D = kDicts ? BR_UNIFORM(J.item_dict_bytes[index]) : BR_UNIFORM(J.dict.bytes);
  Lz77Params P = J.P;
  P.total_bytes = D + it.bytes;
  P.prefix_bytes = P.dict_break = D;
  ChainTables t = T;
  LiveRing lr;
  br_batch_item_tables(J, P, it, D, table, t, lr);
  const uint32_t image = kDicts ? br_batch_item_image(J, index) : kBatchNoImage;  // (wave-uniform)
  if (!kDicts && J.dict.entries != nullptr) {
    br_batch_replay_dictionary(lr, J.dict, P.bucket_bits);
  } else if (kDicts && image != kBatchNoImage) {
    br_batch_replay_dictionary(lr, br_batch_load_image(J.images, image), P.bucket_bits);
  } else {
    br_live_reset(lr, P.bucket_bits);
    if (D > P.htl - 1) br_live_store(lr, 0, 1, D - (P.htl - 1), 1, 0);  // StoreLookaheadThenStore, mod.rs:224-229
  }
  // StitchToPreviousBlock (mod.rs:210-222): the last three dictionary positions, whose four bytes reach into the item
  if (it.bytes >= P.htl - 1 && D >= 3) br_live_store(lr, D - 3u, 1, 3, 1, 0);
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
  br_parse_segment<true, false, true>(P, t, s, seg, entry, left, next, &lr, &tail);
  // (lane 0 holds the exit; bad_commands: a match cut to one byte at the dictionary's end -- the reference fails on this item)
  br_batch_close_record(J.records + index, t.logs, histo, t.text, D, it, tail.n_cmds, tail.n_lits, tail.insert_len, left.bad_commands);
}

}  // namespace brotli_mi355x
#endif
