// batch_zopfli_device.h -- the item code of k_zopfli_batch (batch_zopfli.h): one item of a batch at quality 11, parsed by one
// sequential walk of br_zopfli_parse on H10 trees of its own and closed as the one meta-block of a stream of one block.  Shared by
// the gfx950 kernel (batch_zopfli_kernels.hip) and the host emulation (batch_zopfli_emu.inc).
#ifndef BROTLI_MI355X_BATCH_ZOPFLI_DEVICE_H_
#define BROTLI_MI355X_BATCH_ZOPFLI_DEVICE_H_

#include "batch_zopfli.h"
#include "zopfli_device.h"
#include "batch_item_device.h"

namespace brotli_mi355x {

static_assert(sizeof(ZNode) == 20 && sizeof(Command) == 16 && sizeof(ZBlockCtl) <= 64 && sizeof(SegExit) <= 256, "zopfli_batch_layout sizes a table by these");

BR_DEV ZopfliParams br_zopfli_batch_params(const ZopfliBatchJob& J) {
  ZopfliParams Z;
  Z.quality = J.quality;
  Z.lgwin = J.lgwin;
  Z.max_backward_limit = J.P.max_backward_limit;
  Z.ring_mask = J.P.ring_mask;
  Z.dict_break = 0;  // no custom dictionary in front of an item
  Z.use_dictionary = J.use_dictionary;
  Z.dist_max_distance = J.P.dist_max_distance;
  Z.dist_alphabet_size = J.dist_alphabet_size;
  Z.ndirect = J.P.num_direct_distance_codes;
  Z.npostfix = J.P.dist_postfix_bits;
  return Z;
}

BR_DEV ZopfliBuffers br_zopfli_batch_buffers(const ZopfliBatchJob& J, uint32_t table) {
  uint8_t* base = J.table_mem + (size_t)table * J.table_bytes;
  ZopfliBuffers B;
  B.buckets = (uint32_t*)base;
  B.forest = (uint32_t*)(base + J.off_forest);
  B.nodes = (ZNode*)(base + J.off_nodes);
  B.literal_costs = (float*)(base + J.off_literal_costs);
  B.cost_dist = (float*)(base + J.off_cost_dist);
  B.cost_cmd = (float*)(base + J.off_cost_cmd);
  B.matches = (unsigned long long*)(base + J.off_matches);
  B.num_matches = (uint32_t*)(base + J.off_num_matches);
  B.tmp_cmds = (Command*)(base + J.off_tmp_cmds);
  B.histo = (uint32_t*)(base + J.off_histo);
  return B;
}


// A fresh H10 hasher (InitializeH10, hash_to_binary_tree.rs:149-190; what lz77_zopfli_init leaves) on a table that the item in
// front has used: every bucket the invalid position 0 - window_mask, and the forest slots this item can reach 0 -- the children of
// position p live at 2 * (p & window_mask), p < bytes.  The whole wavefront writes 16 bytes per lane and step; the fill is made
// visible and the wavefront waits for it before the first search reads a bucket.
BR_DEV void br_zopfli_batch_reset(const ZopfliBuffers& B, uint32_t lgwin, uint32_t bytes) {
  const uint32_t invalid = 0u - ((1u << lgwin) - 1u);
  const uint32_t rounded = (bytes + 63u) & ~63u;
  const uint32_t slots = rounded < (1u << lgwin) ? rounded : (1u << lgwin);  // (a multiple of 64 either way: lgwin >= 10)
  BR_SYNC();
  br_batch_fill16(B.buckets, (1u << kZBucketBits) / 4u, invalid);
  br_batch_fill16(B.forest, slots / 2u, 0u);
#if !BR_SCALAR
  __threadfence();
#endif
  BR_SYNC();
}

// ---- a custom dictionary in front of the item (k_zopfli_batch_dicts) ------------------------------------------------------------
// HasherPrependCustomDictionary for H10 (encode.rs:1163-1194; what k_zopfli_prepend does on one lane): Store of every position i
// with i + 127 < D, in ascending order.  The trees of different hash keys touch disjoint memory -- buckets[key] and the children of
// the positions of that key -- and D <= (1 << lgwin) - 16, so no two dictionary positions share a forest slot: lanes that own
// disjoint classes of keys, each walking its positions in ascending order, leave exactly what the one loop leaves
// (k_zopfli_matches stands on the same argument).  A lane owns the keys whose low six bits are its number.
static constexpr uint32_t kZPrependClasses = 64;
BR_DEV uint32_t br_zopfli_prepend_class(const uint8_t* text, uint32_t i) {
  return ((br_load32(text + i) * 0x1e35a7bdu) >> (32 - kZBucketBits)) & (kZPrependClasses - 1u);
}
// the first position of [i, end) whose key is of class `cls`; end: none
BR_DEV uint32_t br_zopfli_prepend_next(const uint8_t* text, uint32_t i, uint32_t end, uint32_t cls) {
  while (i < end && br_zopfli_prepend_class(text, i) != cls) ++i;
  return i;
}
// the positions of one class, in ascending order (the scalar build runs the 64 classes one after the other)
BR_DEV void br_zopfli_prepend_class_walk(const ZH10& h, const ZopfliParams& Z, const uint8_t* text, uint32_t end, uint32_t cls) {
  for (uint32_t i = br_zopfli_prepend_next(text, 0, end, cls); i < end; i = br_zopfli_prepend_next(text, i + 1, end, cls)) z_h10_store(h, Z, text, i);
}
// lane0: the one loop of k_zopfli_prepend on lane 0 instead (the measured alternative, ZopfliBatchJob::prepend_lane0).  The stores
// are made visible and the wavefront waits for them before the first search reads a bucket, as behind br_zopfli_batch_reset.
BR_DEV void br_zopfli_batch_prepend(const ZH10& h, const ZopfliParams& Z, const uint8_t* text, uint32_t D, bool lane0) {
  const uint32_t end = D >= kZMaxTreeCompLength ? D - (kZMaxTreeCompLength - 1u) : 0u;  // (StoreLookahead() - 1 bytes behind the last one stored)
  if (lane0) {
    if (BR_LANE == 0)
      for (uint32_t i = 0; i < end; ++i) z_h10_store(h, Z, text, i);
  } else {
#if BR_SCALAR
    for (uint32_t cls = 0; cls < kZPrependClasses; ++cls) br_zopfli_prepend_class_walk(h, Z, text, end, cls);
#else
    // every lane keeps a cursor of its own and stores while the others store: the loop ends when no lane has a position left
    static_assert(kZPrependClasses == BR_NLANES, "a class per lane");
    const uint32_t cls = (uint32_t)BR_LANE;
    uint32_t i = br_zopfli_prepend_next(text, 0, end, cls);
    while (__any(i < end)) {
      if (i < end) {
        z_h10_store(h, Z, text, i);
        i = br_zopfli_prepend_next(text, i + 1, end, cls);
      }
    }
#endif
  }
#if !BR_SCALAR
  __threadfence();
#endif
  BR_SYNC();
}

// histo: 256 words and fast: the node window, the cost tables and the queue, all the wavefront's own (LDS on the device; the
// emulation passes an array and an empty ZFast).
// kDicts: the item's text starts with J.item_dict_bytes[index] bytes of custom dictionary of its own
// (BrotliMi355xCompressBatchWithDictionaries under BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS): position 0 is the
// dictionary's first byte, the item starts at D, and the chain files the dictionary itself.
template <bool kDicts = false>
BR_DEV void br_zopfli_batch_item(const ZopfliBatchJob& J, const ZopfliTables& T, uint32_t* histo, const ZFast& fast, uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  if constexpr (kDicts) {
    const uint32_t D = BR_UNIFORM(J.item_dict_bytes[index]);
    // (never: the plan sizes the forest by the group's largest dictionary + item, and a dictionary in use ends 16 bytes below the window)
    const bool fits = it.bytes <= J.cap && (D + it.bytes <= J.span || J.span == (1u << J.lgwin)) && D + 16u <= (1u << J.lgwin);
    if (!fits) {
      if (BR_LANE == 0) {
        BatchRecord r{};
        r.overflow = 1;
        J.records[index] = r;
      }
      BR_SYNC();
      return;
    }
    ZopfliParams Z = br_zopfli_batch_params(J);
    Z.dict_break = D;  // (ring_buffer_break: D + bytes stays inside the first lap of the ring, so the ring index is the position)
    const ZopfliBuffers B = br_zopfli_batch_buffers(J, table);
    uint8_t* base = J.table_mem + (size_t)table * J.table_bytes;
    ZBlockCtl* ctl = (ZBlockCtl*)(base + J.off_ctl);
    SegExit* exit_slot = (SegExit*)(base + J.off_exit);
    const uint8_t* text = J.text + it.text_off - D;
    br_zopfli_batch_reset(B, J.lgwin, D + it.bytes);
    const ZH10 h = z_hasher_of(Z, B);
    br_zopfli_batch_prepend(h, Z, text, D, J.prepend_lane0 != 0);
    // StitchToPreviousBlockH10 as br_zopfli_begin runs it for a block behind a prefix (all lanes, identical state); a fresh
    // stream has no last command to extend
    z_h10_stitch(h, Z, text, it.bytes, D);
    Segment seg;
    seg.start = seg.blk_start = D;
    seg.end = seg.blk_end = D + it.bytes;
    seg.flags = kSegFirstInBlock | kSegLastInBlock;
    seg.cmd_base = it.cmd_base;
    seg.block_index = 0;
    seg.cmd_cap = it.cmd_cap;
    SegEntry entry = br_stream_start_entry(0);
    entry.pos = D;
    ctl->position = D;
    ctl->num_bytes = it.bytes;
    ctl->ext_len = 0;
    ctl->event = 0;
    BR_SYNC();
    br_zopfli_parse(Z, T, B, text, seg, entry, ctl, /*precomputed=*/false, J.slabs + (size_t)it.cmd_base, exit_slot, fast);
    BR_SYNC();  // (the exit is written)
    const uint32_t trailing = BR_UNIFORM(exit_slot->insert_len);
    const uint32_t raw_cmds = BR_UNIFORM(exit_slot->n_cmds), raw_lits = BR_UNIFORM(exit_slot->n_lits);
    br_batch_close_record(J.records + index, T.logs, histo, text, D, it, raw_cmds, raw_lits, trailing, BR_UNIFORM(exit_slot->bad_commands));
    // the dictionary's last two bytes (D >= 2): ChooseContextMode's UTF-8 census reads the ring buffer two bytes in front of the
    // stream (metablock_hq.h, hq_census_byte), and the meta-block stage sees the items back to back, without their dictionaries
    if (BR_LANE == 0) J.records[index].pad[0] = (uint32_t)text[D - 2] | ((uint32_t)text[D - 1] << 8);
    BR_SYNC();
    return;
  }
  if (it.bytes > J.cap) {  // (never: the plan sizes a table by the group's largest item)
    if (BR_LANE == 0) {
      BatchRecord r{};
      r.overflow = 1;
      J.records[index] = r;
    }
    BR_SYNC();
    return;
  }
  const ZopfliParams Z = br_zopfli_batch_params(J);
  const ZopfliBuffers B = br_zopfli_batch_buffers(J, table);
  uint8_t* base = J.table_mem + (size_t)table * J.table_bytes;
  ZBlockCtl* ctl = (ZBlockCtl*)(base + J.off_ctl);
  SegExit* exit_slot = (SegExit*)(base + J.off_exit);
  br_zopfli_batch_reset(B, J.lgwin, it.bytes);
  // item-local coordinates: position 0 is the item's first byte, so no distance reaches a neighbour and max_distance is what the
  // reference computes for a stream that starts at 0.  Match lengths are bounded by the bytes left in the item; the 4-byte hash
  // loads of the last searched positions and the dictionary probes end inside the item or its padding.
  const uint8_t* text = J.text + it.text_off;
  Segment seg;
  seg.start = seg.blk_start = 0;
  seg.end = seg.blk_end = it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
  const SegEntry entry = br_stream_start_entry(0);
  // (what br_zopfli_begin leaves for a block at 0 without extend_last_command: nothing to stitch to)
  ctl->position = 0;
  ctl->num_bytes = it.bytes;
  ctl->ext_len = 0;
  ctl->event = 0;
  BR_SYNC();
  br_zopfli_parse(Z, T, B, text, seg, entry, ctl, /*precomputed=*/false, J.slabs + (size_t)it.cmd_base, exit_slot, fast);
  BR_SYNC();  // (the exit is written)
  // (bad_commands: where the reference panics, kZopfliReferencePanics)
  const uint32_t trailing = BR_UNIFORM(exit_slot->insert_len);
  const uint32_t raw_cmds = BR_UNIFORM(exit_slot->n_cmds), raw_lits = BR_UNIFORM(exit_slot->n_lits);
  br_batch_close_record(J.records + index, T.logs, histo, text, 0, it, raw_cmds, raw_lits, trailing, BR_UNIFORM(exit_slot->bad_commands));
}

}  // namespace brotli_mi355x
#endif
