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

// ---- one dictionary that every item names: its tree image, built once per call (lz77_zopfli_dict_image) ---------------------------
// The argument above holds for any number of lanes, so the build spreads the keys over the lanes of SEVERAL wavefronts: a lane owns
// the keys whose low ten bits are its number in the launch (kZImageClasses lanes).  No two lanes touch one word -- buckets[key] and
// the children of the positions of that key -- and a lane reads only words that it or the fill launch in front has written, so the
// workgroups exchange nothing: no atomics, no fences, no order between them.
// How a lane finds its positions: with 16 times the classes, br_zopfli_prepend_next's dependent 4-byte load and multiply per
// position would be the build's cost (every lane looks at every position).  A pass in front writes the class of every stored
// position once, coalesced, as 16-bit entries; a lane then tests 16 positions per step -- two 16-byte loads that every lane near
// the same cursor shares in the L1 -- and only the bit scan depends on them.
static constexpr uint32_t kZImageClasses = 1024;
static constexpr uint32_t kZImageNoClass = 0xffffu;  // the entries behind the last stored position
BR_DEV ZopfliParams br_zopfli_image_params(uint32_t lgwin, uint32_t D) {
  ZopfliParams Z{};  // what a Store looks at: it compares 128 bytes inside the dictionary, so no length is cut at dict_break
  Z.quality = 11;
  Z.lgwin = lgwin;
  Z.max_backward_limit = (1u << lgwin) - 16u;
  Z.ring_mask = 0xffffffffu;
  Z.dict_break = D;
  return Z;
}
// the fill: element `at` of `stride` -- every bucket the invalid position, the forest 0, 16 bytes per element
BR_DEV void br_zopfli_image_fill(uint32_t* buckets, uint32_t* forest, uint32_t lgwin, uint32_t slots, uint32_t at, uint32_t stride) {
  const uint32_t invalid = 0u - ((1u << lgwin) - 1u);
  const uint32_t bucket_quads = (1u << kZBucketBits) / 4u, quads = bucket_quads + slots / 2u;
  for (uint32_t q = at; q < quads; q += stride) {
    uint32_t* w = q < bucket_quads ? buckets + 4u * (size_t)q : forest + 4u * (size_t)(q - bucket_quads);
    const uint32_t v = q < bucket_quads ? invalid : 0u;
    w[0] = v;
    w[1] = v;
    w[2] = v;
    w[3] = v;
  }
}
// the class pass: entry i of [0, entries), entries = zopfli_dict_image_class_entries(D)
BR_DEV void br_zopfli_image_class_entry(const uint8_t* text, uint32_t end, uint16_t* classes, uint32_t i) {
  classes[i] = (uint16_t)(i < end ? ((br_load32(text + i) * 0x1e35a7bdu) >> (32 - kZBucketBits)) & (kZImageClasses - 1u) : kZImageNoClass);
}
// the first position of [i, end) of class `cls`; end: none.  Reads whole groups of 16 entries: [i & ~15, ...) up to `end` rounded up.
BR_DEV uint32_t br_zopfli_image_next(const uint16_t* classes, uint32_t i, uint32_t end, uint32_t cls) {
  while (i < end) {
    const uint32_t base = i & ~15u;
    uint32_t w[8];
#if BR_SCALAR
    memcpy(w, classes + base, 32);
#else
    const uint4 a = ((const uint4*)(classes + base))[0], b = ((const uint4*)(classes + base))[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
#endif
    uint32_t hits = 0;
    for (uint32_t k = 0; k < 8; ++k) hits |= ((w[k] & 0xffffu) == cls ? 1u << (2 * k) : 0u) | ((w[k] >> 16) == cls ? 2u << (2 * k) : 0u);
    hits &= 0xffffffffu << (i & 15u);
    if (hits != 0) return base + (uint32_t)__builtin_ctz(hits);  // (below end: the entries behind it are of no class)
    i = base + 16u;
  }
  return end;
}
// the positions of one class, in ascending order: one lane of the store launch (the scalar build runs the classes one after the other)
BR_DEV void br_zopfli_image_store_class(const ZH10& h, const ZopfliParams& Z, const uint8_t* text, const uint16_t* classes, uint32_t end, uint32_t cls) {
  for (uint32_t i = br_zopfli_image_next(classes, 0, end, cls); i < end; i = br_zopfli_image_next(classes, i + 1, end, cls)) z_h10_store(h, Z, text, i);
}

// p[0 .. 4 * quads) = src[0 .. 4 * quads) by the whole wavefront, 16 bytes per lane and step, four steps in flight: the loads of a
// round are issued together, then its stores (the loop of br_quick_batch_prime, batch_quick_device.h).  Both 16-byte aligned; `src` is read-only for the launch
// (plain loads).  Barriers and fence are the caller's, as around a fill.
BR_DEV void br_batch_copy16(uint32_t* p, const uint32_t* src, uint32_t quads) {
#if BR_SCALAR
  for (uint32_t i = 0; i < 4u * quads; ++i) p[i] = src[i];
#else
  uint4* w = (uint4*)p;
  const uint4* s = (const uint4*)src;
  for (uint32_t i = (uint32_t)BR_LANE; i < quads; i += 4u * BR_NLANES) {
    const uint32_t i1 = i + BR_NLANES, i2 = i + 2u * BR_NLANES, i3 = i + 3u * BR_NLANES;
    const uint4 v0 = s[i];
    const uint4 v1 = s[i1 < quads ? i1 : i];
    const uint4 v2 = s[i2 < quads ? i2 : i];
    const uint4 v3 = s[i3 < quads ? i3 : i];
    w[i] = v0;
    if (i1 < quads) w[i1] = v1;
    if (i2 < quads) w[i2] = v2;
    if (i3 < quads) w[i3] = v3;
  }
#endif
}

// The hasher as br_zopfli_batch_reset(B, lgwin, D + bytes) and the prepend of the D dictionary bytes leave it, on a table that
// the item in front has used: the image's buckets go over ALL buckets, its forest over the slots of the positions below D rounded
// up to 64, and the slots from there to the item's end are zeroed.  Wave-wide, 16 bytes per lane and step; the image is read-only
// for the launch (plain loads).  Made visible, and waited for, as the reset is.
BR_DEV void br_zopfli_batch_replay(const ZopfliBuffers& B, const uint32_t* image_buckets, const uint32_t* image_forest, uint32_t lgwin, uint32_t D,
                                   uint32_t bytes) {
  const uint32_t s_dict = zopfli_dict_image_slots(D, lgwin), s_all = zopfli_dict_image_slots(D + bytes, lgwin);
  BR_SYNC();
  br_batch_copy16(B.buckets, image_buckets, (1u << kZBucketBits) / 4u);
  br_batch_copy16(B.forest, image_forest, s_dict / 2u);
  br_batch_fill16(B.forest + 2u * (size_t)s_dict, (s_all - s_dict) / 2u, 0u);
#if !BR_SCALAR
  __threadfence();
#endif
  BR_SYNC();
}

// histo: 256 words and fast: the node window, the cost tables and the queue, all the wavefront's own (LDS on the device; the
// emulation passes an array and an empty ZFast).
// kDict: the item's text starts with D bytes of custom dictionary: position 0 is the dictionary's first byte, the item starts at D.
//   kZBatchItemDicts  a dictionary of the item's own, D = J.item_dict_bytes[index] (BrotliMi355xCompressBatchWithDictionaries under
//                     BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS): the chain files it itself
//   kZBatchSharedDict the call's one dictionary, D = J.dict_bytes: the chain replays the call's image of it
enum : int { kZBatchNoDict = 0, kZBatchItemDicts = 1, kZBatchSharedDict = 2 };
template <int kDict = kZBatchNoDict>
BR_DEV void br_zopfli_batch_item(const ZopfliBatchJob& J, const ZopfliTables& T, uint32_t* histo, const ZFast& fast, uint32_t index, uint32_t table) {
  const BatchItem it = br_batch_load_item(J.items, index);
  if constexpr (kDict != kZBatchNoDict) {
    const uint32_t D = kDict == kZBatchSharedDict ? J.dict_bytes : BR_UNIFORM(J.item_dict_bytes[index]);
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
    const ZH10 h = z_hasher_of(Z, B);
    if constexpr (kDict == kZBatchSharedDict) {
      br_zopfli_batch_replay(B, J.image_buckets, J.image_forest, J.lgwin, D, it.bytes);
    } else {
      br_zopfli_batch_reset(B, J.lgwin, D + it.bytes);
      br_zopfli_batch_prepend(h, Z, text, D, J.prepend_lane0 != 0);
    }
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
