// batch_greedy_device.h -- the item code of k_parse_batch (batch_greedy.h): one item of a batch, parsed by one live chain on a
// table of its own and closed as the one meta-block of a stream of one block.  Shared by the gfx950 kernel and the host emulation.
#ifndef BROTLI_MI355X_BATCH_GREEDY_DEVICE_H_
#define BROTLI_MI355X_BATCH_GREEDY_DEVICE_H_

#include "batch_greedy.h"
#include "lz77_chain.h"

namespace brotli_mi355x {

// T: the job's tables with text / keys / flags / cmds still pointing at the group's arrays.
template <bool kRows>
BR_DEV void br_batch_item(const BatchParseJob& J, const ChainTables& T, ChainScratchT<false, kRows>& s, uint32_t* histo /* 256 words */,
                          uint32_t index, uint32_t table) {
  BatchItem it = J.items[index];
  it.text_off = BR_UNIFORM(it.text_off);
  it.bytes = BR_UNIFORM(it.bytes);
  it.cmd_base = BR_UNIFORM(it.cmd_base);
  it.cmd_cap = BR_UNIFORM(it.cmd_cap);
  // item-local coordinates: position 0 is the item's first byte, so no distance reaches a neighbour and max_backward is what
  // the reference computes for a stream that starts at 0
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
  // an empty hasher: the ring counters at 0 (a walk never reads a slot its counter does not cover: `buckets` needs no fill)
  br_live_reset(lr, P.bucket_bits);
  Segment seg;
  seg.start = seg.blk_start = 0;
  seg.end = seg.blk_end = it.bytes;
  seg.flags = kSegFirstInBlock | kSegLastInBlock;
  seg.cmd_base = it.cmd_base;
  seg.block_index = 0;
  seg.cmd_cap = it.cmd_cap;
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
  SegExit left;
  SegEntry next;
  BlockTail tail;
  br_parse_segment<false, kRows, true>(P, t, s, seg, entry, left, next, &lr, &tail);
  // ---- Lz77Stage::Resolve for the only block of a stream: the pending literals become the trailing insert-only command, and
  // should_compress (encode.rs:1325-1354) gives the verdict
  const uint32_t bytes = it.bytes;
  const uint32_t trailing = tail.insert_len;
  const uint32_t cmds_all = tail.n_cmds + (trailing != 0 ? 1u : 0u), lits_all = tail.n_lits + trailing;
  bool compress = true;
  if (cmds_all < (bytes >> 8) + 2 && (float)lits_all > 0.99f * (float)bytes) {
    BR_SYNC();
    for (uint32_t i = BR_LANE; i < 256; i += BR_NLANES) histo[i] = 0;
    BR_SYNC();
    for (uint32_t q = 13u * (uint32_t)BR_LANE; q < bytes; q += 13u * BR_NLANES) BR_ATOMIC_INC(&histo[t.text[q]]);
    BR_SYNC();
    const float threshold = (float)bytes * 7.92f / 13.0f;
    compress = !(br_bits_entropy(t.logs, histo, 256) > threshold);
  }
  if (BR_LANE == 0) {
    BatchRecord r;
    r.n_cmds = cmds_all;
    r.n_lits = lits_all;
    r.trailing = trailing;
    r.uncompressed = compress ? 0u : 1u;
    r.overflow = cmds_all > it.cmd_cap ? 1u : 0u;
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    J.records[index] = r;
  }
  BR_SYNC();
}

// command i of item `index` as the meta-block stage wants it
BR_DEV Command br_batch_command(const BatchParseJob& J, const BatchItem& it, const BatchRecord& r, uint32_t i) {
  if (r.trailing != 0 && i + 1 == r.n_cmds) {
    // Command::init_insert, command.rs:38-44
    Command c;
    c.insert_len_ = r.trailing;
    c.copy_len_ = 4u << 25;
    c.dist_extra_ = 0;
    c.dist_prefix_ = (uint16_t)((1u << 10) | 16u);
    c.cmd_prefix_ = br_combine_length_codes(br_insert_length_code(r.trailing), br_copy_length_code(4), false);
    return c;
  }
  return br_finish_command(J.slabs[(size_t)it.cmd_base + i], J.P.num_direct_distance_codes, J.P.dist_postfix_bits);
}

}  // namespace brotli_mi355x
#endif
