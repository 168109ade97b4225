// batch_item_device.h -- what the item code of every batch route has in common (batch_greedy_device.h, batch_quick_device.h,
// batch_zopfli_device.h): loading an item, the entry a stream starts with, the should_compress verdict, the close of a one-block
// item, and the books between the blocks of an item of several blocks.  BR_DEV code for the gfx950 kernels and the host emulation
// alike; include after the BR_DEV macros and the command helpers (lz77_chain.h, which every item header has through its parser).
//
// A reference rule that touches one of these steps is written here, once.  The one exception is br_parse_live (lz77_chain.h), which
// keeps its own copy of the books and of the verdict: it is inlined into k_parse_live, the kernel the benchmark runs, and its books
// live in LiveBlockState records that the host resolver reads back -- sharing code with it would move the code generation of that
// kernel for no gain here.  A second, measured one is br_batch_item_long (batch_greedy_device.h), which uses everything here but
// BatchLongBooks: its kernel ran slower behind the shared steps, so it keeps them written out.  Whoever changes a rule of the books
// below looks at these two as well.
#ifndef BROTLI_MI355X_BATCH_ITEM_DEVICE_H_
#define BROTLI_MI355X_BATCH_ITEM_DEVICE_H_

#include "batch_greedy.h"
#include "entropy_device.h"
#include "lz77_types.h"

namespace brotli_mi355x {

#if !BR_SCALAR
// The persistent loop of a batch kernel, one wavefront per table: takes the next place of `order` (largest item first) from the
// device counter.  False when none is left.
__device__ __forceinline__ bool br_batch_next_index(uint32_t* counter, const uint32_t* order, uint32_t n_items, uint32_t& index) {
  uint32_t mine = 0;
  if (threadIdx.x == 0) mine = atomicAdd(counter, 1u);
  const uint32_t place = BR_UNIFORM(mine);
  if (place >= n_items) return false;
  index = BR_UNIFORM(order[place]);
  return index < n_items;  // (always: the plan's order is a permutation)
}
#endif

// the item with its four fields made wave-uniform
BR_DEV BatchItem br_batch_load_item(const BatchItem* items, uint32_t index) {
  BatchItem it = items[index];
  it.text_off = BR_UNIFORM(it.text_off);
  it.bytes = BR_UNIFORM(it.bytes);
  it.cmd_base = BR_UNIFORM(it.cmd_base);
  it.cmd_cap = BR_UNIFORM(it.cmd_cap);
  return it;
}

// The entry of a stream's first block, at position 0: the distance cache a stream starts with, nothing pending, exact (empty)
// dictionary books.  apply: apply_random_heuristics at the start (SegEntry::apply).
BR_DEV SegEntry br_stream_start_entry(uint32_t apply) {
  SegEntry entry;
  entry.pos = 0;
  entry.apply = apply;
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
  return entry;
}

// Command::init_insert, command.rs:38-44: the trailing insert-only command of a meta-block
BR_DEV Command br_insert_only_command(uint32_t n) {
  Command c;
  c.insert_len_ = n;
  c.copy_len_ = 4u << 25;
  c.dist_extra_ = 0;
  c.dist_prefix_ = (uint16_t)((1u << 10) | 16u);
  c.cmd_prefix_ = br_combine_length_codes(br_insert_length_code(n), br_copy_length_code(4), false);
  return c;
}

// should_compress (encode.rs:1325-1354) over the meta-block text[from, to) with cmds_all commands and lits_all literals, the
// trailing insert-only command included: few commands, nearly all literals, and an every-13th-byte histogram whose f32 entropy
// says "incompressible" send it out uncompressed.  Collective: the whole wavefront calls it with the same arguments and gets the
// same answer; histo is 256 words of its own (LDS on the device).
BR_DEV bool br_should_compress(const EntropyTables& logs, uint32_t* histo, const uint8_t* text, uint32_t from, uint32_t to, uint32_t cmds_all,
                               uint32_t lits_all) {
  const uint32_t bytes = to - from;
  if (!(cmds_all < (bytes >> 8) + 2 && (float)lits_all > 0.99f * (float)bytes)) return true;
  BR_SYNC();
  for (uint32_t i = BR_LANE; i < 256; i += BR_NLANES) histo[i] = 0;
  BR_SYNC();
  for (uint32_t q = from + 13u * (uint32_t)BR_LANE; q < to; q += 13u * BR_NLANES) BR_ATOMIC_INC(&histo[text[q]]);
  BR_SYNC();
  const float threshold = (float)bytes * 7.92f / 13.0f;
  return !(br_bits_entropy(logs, histo, 256) > threshold);
}

// Lz77Stage::Resolve for the only block of a stream, text[from, from + it.bytes): the pending literals become the trailing
// insert-only command, should_compress gives the verdict, and lane 0 leaves the record.  bad_commands (lane 0's value counts;
// routes without one pass 0): the reference fails on this item -- a copy of one byte, which it cannot encode (GetCopyLengthCode,
// command.rs:91-93) and neither do the tables behind br_finish_command, or one of its own panics -- so the item is handed on as
// literals only and flagged; its stream is dropped by the host.
BR_DEV void br_batch_close_record(BatchRecord* record, const EntropyTables& logs, uint32_t* histo, const uint8_t* text, uint32_t from, const BatchItem& it,
                                  uint32_t raw_cmds, uint32_t raw_lits, uint32_t trailing, uint32_t bad_commands) {
  const uint32_t cmds_all = raw_cmds + (trailing != 0 ? 1u : 0u), lits_all = raw_lits + trailing;
  const bool compress = br_should_compress(logs, histo, text, from, from + it.bytes, cmds_all, lits_all);
  if (BR_LANE == 0) {
    BatchRecord r;
    r.n_cmds = cmds_all;
    r.n_lits = lits_all;
    r.trailing = trailing;
    r.uncompressed = compress ? 0u : 1u;
    r.overflow = cmds_all > it.cmd_cap ? 1u : 0u;
    r.bad_commands = bad_commands;
    if (bad_commands != 0) {
      r.n_cmds = 1;
      r.n_lits = r.trailing = it.bytes;
      r.uncompressed = 1;
      r.overflow = 0;
    }
    r.pad[0] = r.pad[1] = 0;
    *record = r;
  }
  BR_SYNC();
}

// p[0 .. 4 * quads) = v by the whole wavefront, 16 bytes per lane and step.  The barriers around a fill and the fence that makes
// it visible at device scope are the caller's.
BR_DEV void br_batch_fill16(uint32_t* p, uint32_t quads, uint32_t v) {
#if BR_SCALAR
  for (uint32_t i = 0; i < 4u * quads; ++i) p[i] = v;
#else
  uint4* w = (uint4*)p;
  for (uint32_t i = (uint32_t)BR_LANE; i < quads; i += BR_NLANES) w[i] = make_uint4(v, v, v, v);
#endif
}

// ---- items of several blocks: the books between the blocks -----------------------------------------------------------------------
// One chain walks an item of two to kBatchLongBlocks input blocks from block to block and does between them what
// Lz77Stage::Resolve does for a stream that starts at 0.  The chain is the only writer of its slab, so extend_last_command and the
// literals pending at a block's entry are applied to its own raw commands in place (the host resolver's CmdPatch kinds 0 and 2), a
// block's commands start where the block in front stopped, and every meta-block the flush rule closes leaves a record.  A caller:
//
//   BatchLongBooks b = br_books_open();
//   for (uint32_t bs = 0; br_books_more(b, it, bs);) {
//     const uint32_t be = br_books_block_end(P, it, bs);
//     ... parse [bs, be) from `entry` into slab + b.used, with it.cmd_cap - b.used commands of room; fill a BatchBlockOutcome x ...
//     if (!br_books_take(b, slab, it, x)) break;
//     br_books_close(b, P, logs, histo, text, it, be, count_rule, x.cache, record);
//     br_books_next(b, P, be, x.cache, entry);
//     BR_SYNC();
//     bs = be;
//   }
//   br_books_finish(b, record);

// what the books need of a block's parse: BlockTail + the entry handed on (live chains), or the SegExit (qualities 2 .. 4)
struct BatchBlockOutcome {
  uint32_t n_cmds, n_lits, insert_len, ext_len, last_dist_code, last_copy_len;
  int32_t cache[4];  // the distance cache behind the block
};

struct BatchLongBooks {
  uint32_t mb_start, mb_cmds, mb_lits, mb_first_cmd;  // the open meta-block (LiveBlockState); mb_first_cmd: in the slab
  uint32_t last_valid, last_dist_code, last_copy_len;  // its last command
  int32_t saved_cache[4];                              // the distance cache at its start
  uint32_t carry;                                      // literals pending at the entry of the block
  uint32_t used;                                       // raw commands in the slab so far
  uint32_t n_mb, overflow;
};

BR_DEV BatchLongBooks br_books_open() {
  BatchLongBooks b;
  b.mb_start = b.mb_cmds = b.mb_lits = b.mb_first_cmd = 0;
  b.last_valid = b.last_dist_code = b.last_copy_len = 0;
  b.saved_cache[0] = 4;
  b.saved_cache[1] = 11;
  b.saved_cache[2] = 15;
  b.saved_cache[3] = 16;
  b.carry = b.used = 0;
  b.n_mb = b.overflow = 0;
  return b;
}

// is there a block at bs?  (n_mb: never the bound -- a meta-block is at least one block -- but the record has no more room)
BR_DEV bool br_books_more(const BatchLongBooks& b, const BatchItem& it, uint32_t bs) { return bs < it.bytes && b.n_mb < kBatchLongBlocks; }
BR_DEV uint32_t br_books_block_end(const Lz77Params& P, const BatchItem& it, uint32_t bs) {
  return it.bytes - bs > P.block_bytes ? bs + P.block_bytes : it.bytes;
}

// Takes the outcome of the block that was parsed into slab + b.used: false (and `overflow`) if its commands did not fit -- the
// check is made before anything reads them.  Lane 0 applies the fix-ups to the slab.
BR_DEV bool br_books_take(BatchLongBooks& b, Command* slab, const BatchItem& it, const BatchBlockOutcome& x) {
  if (x.n_cmds > it.cmd_cap - b.used) {
    b.overflow = 1;
    return false;
  }
  if (BR_LANE == 0) {
    if (x.ext_len != 0 && b.last_valid) slab[b.used - 1].copy_len_ += x.ext_len;  // (its copy code is its length: no dictionary word is extended)
    if (x.n_cmds != 0 && b.carry != 0) slab[b.used].insert_len_ += b.carry;
  }
  if (x.ext_len != 0 && b.last_valid) b.last_copy_len += x.ext_len;
  b.mb_cmds += x.n_cmds;
  b.mb_lits += x.n_lits;
  if (x.n_cmds != 0) {
    b.mb_lits += b.carry;
    b.carry = x.insert_len;
    b.last_valid = 1;
    b.last_dist_code = x.last_dist_code;
    b.last_copy_len = x.last_copy_len;
  } else {
    b.carry += x.insert_len;
  }
  b.used += x.n_cmds;
  return true;
}

// The flush rule (encode.rs:2454-2477) behind the block that ends at be: closes the open meta-block if the item ends there, if the
// next block does not fit, or if it holds an eighth of MaxMetablockSize in literals or commands; with count_rule (below
// MIN_QUALITY_FOR_BLOCK_SPLIT) also once it holds 0x2fff literals + commands (encode.rs:2458-2459) -- counted as the reference
// counts them, in front of the trailing insert-only command: literals pending behind the last command do not count yet.  A closed
// meta-block gets its verdict (collective) and its entry in the record; `cache`, the distance cache handed to the next block, is
// the one of the meta-block's START behind a stored one (encode.rs:1994).
BR_DEV void br_books_close(BatchLongBooks& b, const Lz77Params& P, const EntropyTables& logs, uint32_t* histo, const uint8_t* text, const BatchItem& it,
                           uint32_t be, bool count_rule, int32_t* cache, BatchLongRecord* record) {
  const uint32_t max_mb = P.max_metablock_bytes, limit = max_mb / 8;
  const bool should_flush = count_rule && b.mb_lits + b.mb_cmds >= 0x2fffu;
  const bool next_fits = (uint64_t)(be - b.mb_start) + P.block_bytes <= (uint64_t)max_mb && !should_flush;
  if (!(be == it.bytes || !(next_fits && b.mb_lits < limit && b.mb_cmds < limit))) return;
  const uint32_t cmds_all = b.mb_cmds + (b.carry != 0 ? 1u : 0u), lits_all = b.mb_lits + b.carry;  // with the trailing insert-only command
  const bool compress = br_should_compress(logs, histo, text, b.mb_start, be, cmds_all, lits_all);
  if (BR_LANE == 0) {
    BatchLongMetaBlock m;
    m.start = b.mb_start;
    m.bytes = be - b.mb_start;
    m.first_cmd = b.mb_first_cmd;
    m.n_cmds = b.mb_cmds;
    m.n_lits = lits_all;
    m.trailing = b.carry;
    m.uncompressed = compress ? 0u : 1u;
    m.pad = 0;
    record->mb[b.n_mb] = m;
  }
  ++b.n_mb;
  if (!compress)
    for (int i = 0; i < 4; ++i) cache[i] = b.saved_cache[i];
  for (int i = 0; i < 4; ++i) b.saved_cache[i] = cache[i];
  b.mb_start = be;
  b.mb_cmds = b.mb_lits = 0;
  b.mb_first_cmd = b.used;
  b.last_valid = 0;
  b.carry = 0;  // (pending literals went into its trailing insert-only command)
}

// What the books give the entry of the block at be: position, distance cache, pending literals, and whether extend_last_command
// may run (encode.rs:2435-2437) -- there is a last command in the open meta-block, nothing is pending behind it and its distance
// is the last distance, within reach.  Everything else of the entry is the caller's.
BR_DEV void br_books_next(const BatchLongBooks& b, const Lz77Params& P, uint32_t be, const int32_t* cache, SegEntry& entry) {
  entry.pos = be;
  for (int i = 0; i < 4; ++i) entry.cache[i] = cache[i];
  entry.insert_len = b.carry;
  entry.ext_allowed = 0;
  if (b.mb_cmds != 0 && b.carry == 0 && b.last_valid) {
    const uint64_t cmd_dist = (uint64_t)(int64_t)cache[0];
    if (b.last_dist_code < 16 || (uint64_t)b.last_dist_code - 15 == cmd_dist) {
      const uint64_t lpp = (uint64_t)be - b.last_copy_len;
      const uint64_t max_distance = lpp < P.max_backward_limit ? lpp : P.max_backward_limit;
      if (cmd_dist <= max_distance) entry.ext_allowed = 1;
    }
  }
}

// the record tail, behind the item's last block (or the overflow)
BR_DEV void br_books_finish(const BatchLongBooks& b, BatchLongRecord* record) {
  if (BR_LANE == 0) {
    record->n_mb = b.n_mb;
    record->overflow = b.overflow;
    record->bad_commands = 0;
    record->pad = 0;
  }
  BR_SYNC();
}

}  // namespace brotli_mi355x
#endif
