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

// T: the static-dictionary tables; logs: should_compress; histo: 256 words and exit_slot: one SegExit, both the wavefront's own
// (LDS on the device).
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
  br_quick_batch_zero(Q.table, words);
  // item-local coordinates: position 0 is the item's first byte, so no distance reaches a neighbour and max_backward is what
  // the reference computes for a stream that starts at 0.  The last searched position is bytes - 9 (its lazy successor
  // bytes - 8): the 8-byte loads of q_key end inside the item, the 16-byte loads of br_match_len_wide inside its padding.
  Lz77Params P = J.P;
  P.total_bytes = it.bytes;
  // known here, whatever the job says: no custom dictionary in front of an item, the literal-spree window of qualities below 9,
  // five hashed bytes (H2, H3, H4) -- constants the compiler folds, registers the chain does not hold
  P.prefix_bytes = P.dict_break = 0;
  P.spree_window = 64;
  Q.hash_len = 5;
  const uint8_t* text = J.text + it.text_off;
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
    for (uint32_t q = 13u * (uint32_t)BR_LANE; q < bytes; q += 13u * BR_NLANES) BR_ATOMIC_INC(&histo[text[q]]);
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
    r.pad[0] = r.pad[1] = 0;
    J.records[index] = r;
  }
  BR_SYNC();
}

}  // namespace brotli_mi355x
#endif
