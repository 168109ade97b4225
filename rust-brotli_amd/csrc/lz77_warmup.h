// lz77_warmup.h -- from the exits of the dry runs to the entries of round 0: the item code, shared by the host driver
// (Lz77Stage::WarmupEnd, the forecast of RunRounds), the gfx950 kernels (lz77_kernels.hip: k_warmup_*) and their emulation
// (lz77_warmup_emu.inc).
//
// A dry run parses the last warmup_bytes of segment k from a cold state; the state it ends in is the guess for the entry of
// segment k + 1.  Three things in that guess hang on other segments:
//   * the distance cache: the pushes of the dry run, on top of the guess for the segment it ran in.  One dry run is the map
//     "push these np <= 4 distances" (WarmupOp); maps compose associatively, so the guesses are an inclusive scan of the ops
//     over the segments, applied to the cache the stream starts with;
//   * the phase of a literal spree: a dry run that found no command ends in the state of a spree begun at its own start; the
//     real one began where the last copy ended.  warmup_predict_literal_run carries an entry through a segment without
//     commands in closed form; a run of such segments inside a block is walked by the thread of its first segment;
//   * the forecast of where the static dictionary is switched off: running sums of the lookups and matches the dry runs saw,
//     scaled to whole segments.  The sums are exact 64-bit integers (in units of 1 / warmup_bytes), so that they do not
//     depend on the order of summation and every segment can test the criterion by itself.
#ifndef BROTLI_MI355X_LZ77_WARMUP_H_
#define BROTLI_MI355X_LZ77_WARMUP_H_

#include <math.h>
#include <stdint.h>

#include "lz77_types.h"

#if defined(__HIPCC__)
#define BR_HD __host__ __device__ inline
#else
#define BR_HD inline
#endif

namespace brotli_mi355x {

// first guess of the throttle counters of a chain whose true ones are not known (DictTracker, lz77_stage.cpp)
static constexpr uint32_t kWarmDeadL = 0x40000000u, kWarmDeadM = 0, kWarmAliveL = 0, kWarmAliveM = 0x01000000u;
static constexpr uint32_t kWarmupTile = 256;  // segments per tile of the scan

struct WarmupShape {
  uint32_t num_segments;
  uint32_t warmup_bytes;
  uint32_t segment_bytes;
  uint32_t spree_guess;  // carry the phase of a literal spree through segments without commands
};

// the dry run of segment g: its tail, entered cold
BR_HD Segment warmup_segment(Segment g, uint32_t warmup_bytes) {
  if (g.end - g.start > warmup_bytes) g.start = g.end - warmup_bytes;
  g.flags = (g.flags & kSegTailStitched) | kSegWarmup;
  return g;
}
BR_HD SegEntry warmup_entry(SegEntry e, const Segment& dry, uint32_t spree_window, bool dict_dead) {
  e.pos = dry.start;
  e.apply = dry.start + spree_window;
  e.dict_lookups = dict_dead ? kWarmDeadL : kWarmAliveL;
  e.dict_matches = dict_dead ? kWarmDeadM : kWarmAliveM;
  return e;
}

struct WarmupOp {
  uint32_t np;      // pushes, saturated at 4
  int32_t d[4];     // the last np distances pushed, newest first
  uint64_t sl, sm;  // lookups / matches of the dry run x (bytes of the segment, at least warmup_bytes)
};
BR_HD WarmupOp warmup_identity() {
  WarmupOp o;
  o.np = 0;
  o.d[0] = o.d[1] = o.d[2] = o.d[3] = 0;
  o.sl = o.sm = 0;
  return o;
}
// seg: the whole segment; entered: the counters the dry run started from
BR_HD WarmupOp warmup_op(const Segment& seg, const SegExit& x, uint32_t entered_lookups, uint32_t entered_matches, uint32_t warmup_bytes) {
  WarmupOp o;
  o.np = x.n_pushes < 4 ? x.n_pushes : 4;
  for (uint32_t c = 0; c < 4; ++c) o.d[c] = c < o.np ? x.cache[c] : 0;
  const uint32_t len = seg.end - seg.start;
  const uint64_t weight = len <= warmup_bytes ? warmup_bytes : len;
  o.sl = (uint64_t)(x.dict_lookups - entered_lookups) * weight;
  o.sm = (uint64_t)(x.dict_matches - entered_matches) * weight;
  return o;
}
// a, then b
BR_HD WarmupOp warmup_combine(const WarmupOp& a, const WarmupOp& b) {
  WarmupOp o;
  o.np = a.np + b.np < 4 ? a.np + b.np : 4;
  for (uint32_t c = 0; c < 4; ++c) o.d[c] = c < b.np ? b.d[c] : (c - b.np < a.np ? a.d[c - b.np] : 0);
  o.sl = a.sl + b.sl;
  o.sm = a.sm + b.sm;
  return o;
}
BR_HD void warmup_apply_cache(const WarmupOp& o, const int32_t base[4], int32_t out[4]) {
  int32_t r[4];
  for (uint32_t c = 0; c < 4; ++c) r[c] = c < o.np ? o.d[c] : base[c - o.np];
  for (uint32_t c = 0; c < 4; ++c) out[c] = r[c];
}

// Has the throttle (matches < lookups >> 7, mod.rs:1957-1960) tripped by the end of a segment with these running sums?  Three
// standard deviations of the sampled match count on the late side (see RunRounds).
BR_HD bool warmup_dictionary_dies(uint64_t sl, uint64_t sm, uint32_t warmup_bytes, uint32_t segment_bytes) {
  const double sample = (double)warmup_bytes / (double)segment_bytes;
  const double L = (double)sl / (double)warmup_bytes, M = (double)sm / (double)warmup_bytes;
  const double ms = M * sample;
  const double sigma = sqrt(ms > 1.0 ? ms : 1.0) / sample;
  return L >= 256.0 && M + 3.0 * sigma < L / 128.0;
}

// What the exit x of the dry run of segment `seg` says about the entry e of the segment `next` behind it (everything but the
// distance cache).
BR_HD void warmup_entry_from_exit(const Segment& seg, const Segment& next, const SegExit& x, uint32_t max_backward_limit, SegEntry* e) {
  if (!(next.flags & kSegFirstInBlock)) {
    e->pos = x.pos;
    e->apply = x.apply;
    e->head_kind = x.tail_kind;
    e->head_base = x.tail_base;
    e->head_p1 = x.tail_p1;
  } else {
    // will extend_last_command run at the start of the next block (encode.rs:2435-2437, 360-400)?  Same test as in
    // Resolve(), on the dry run's last command.  A wrong guess is caught there.
    e->ext_allowed = 0;
    // (the dry run is not told that its segment ends the block, so it does not add the unsearched tail of the block to
    // its pending literals: only a copy that reaches the very end of the block leaves nothing pending)
    if (x.n_cmds > 0 && x.insert_len == 0 && x.pos >= seg.blk_end) {
      const uint64_t cmd_dist = (uint64_t)(int64_t)x.cache[0];
      if (x.last_dist_code < 16 || (uint64_t)x.last_dist_code - 15 == cmd_dist) {
        const uint64_t lpp = (uint64_t)next.blk_start - x.last_copy_len;
        if (cmd_dist <= (lpp < max_backward_limit ? lpp : (uint64_t)max_backward_limit)) e->ext_allowed = 1;
      }
    }
  }
}

// Where a chain that finds no match at all leaves segment `seg` when it enters it in state `e`: the stepping of the parse loop
// (br_parse_segment) through a literal spree -- every position, then every 9th, then every 17th (mod.rs:2529-2546) -- in closed
// form.  (The loop itself, step by step: PredictLiteralRunStepwise, lz77_stage.cpp; BROTLI_MI355X_SELFTEST compares the two.)
BR_HD void warmup_predict_literal_run(uint32_t htl_, uint32_t spree_window, const Segment& seg, const SegEntry& e, SegExit* x) {
  const uint64_t pos_end = seg.blk_end, htl = htl_, window = spree_window;
  const uint64_t margin = htl - 1 > 4 ? htl - 1 : 4;
  uint64_t position = e.pos;
  const uint64_t apply = e.apply;
  uint32_t tail_kind = e.head_kind;
  uint64_t tail_base = e.head_base;
  // the loop runs while position < stop
  uint64_t stop = pos_end > htl ? pos_end - htl : 0;
  if (seg.end < stop) stop = seg.end;
  // one position at a time up to `apply`
  if (position < stop && position < apply) position = stop < apply ? stop : apply;
  // strides: a step from p looks at p' = p + 1.  p' + 16 >= pos_end - margin ends the block; p' <= apply + 4 * window
  // jumps 8 on (stride 9), anything later 16 (stride 17).
  const uint64_t block_tail = pos_end > margin + 16 ? pos_end - margin - 16 : 0;  // p' >= block_tail: the end-of-block step
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const uint64_t step = pass == 0 ? 9 : 17;
    const uint64_t p_limit = pass == 0 ? apply + 4 * window : ~0ull >> 1;
    if (!(position < stop)) break;
    if (pass == 1 && !(position + 1 > apply + 4 * window)) break;
    // steps from positions p = position, position + step, ... while p < stop, p + 1 < block_tail and p + 1 <= p_limit
    uint64_t bound = stop;                                   // p < bound
    const uint64_t bt = block_tail > 0 ? block_tail - 1 : 0;  // p + 1 < block_tail
    if (bt < bound) bound = bt;
    if (p_limit < bound) bound = p_limit;                    // p + 1 <= p_limit  <=>  p < p_limit
    if (position >= bound) continue;
    const uint64_t n = (bound - position + step - 1) / step;
    tail_kind = pass == 0 ? (uint32_t)kHeadEven4 : (uint32_t)kHeadVec4;
    tail_base = position + (n - 1) * step + 1;
    position += n * step;
  }
  if (position < stop && position + 1 >= block_tail && position + 1 > apply) {
    tail_kind = kHeadUnstored;
    tail_base = position + 1;
    position = pos_end;
  }
  if (seg.flags & kSegLastInBlock) position = pos_end;
  x->pos = (uint32_t)position;
  x->apply = (uint32_t)apply;
  x->insert_len = (uint32_t)position - e.pos;
  x->tail_kind = position > seg.end ? tail_kind : (uint32_t)kHeadNone;
  x->tail_base = position > seg.end ? (uint32_t)tail_base : 0u;
  x->tail_p1 = position > seg.end ? e.head_p1 : 0u;
}

// Is the phase of a spree carried through segment `seg` into `next` (whose entry is then warmup_spree_step of seg's entry)?
// e: the entry guessed for seg, x: the exit of seg's dry run.
BR_HD bool warmup_spree_carries(const Segment& seg, const Segment& next, const SegEntry& e, const SegExit& x) {
  if (x.n_cmds != 0) return false;
  if (next.flags & kSegFirstInBlock) return false;
  if ((seg.flags & kSegFirstInBlock) && e.ext_allowed) return false;  // (how far extend_last_command gets is not known yet)
  return true;
}
BR_HD void warmup_spree_step(uint32_t htl, uint32_t spree_window, const Segment& seg, SegEntry from, SegEntry* e) {
  if (seg.flags & kSegFirstInBlock) {
    from.pos = seg.blk_start;
    from.apply = from.pos + spree_window;
    from.head_kind = kHeadNone;
    from.head_base = from.head_p1 = 0;
  }
  SegExit x;
  warmup_predict_literal_run(htl, spree_window, seg, from, &x);
  e->pos = x.pos;
  e->apply = x.apply;
  e->head_kind = x.tail_kind;
  e->head_base = x.tail_base;
  e->head_p1 = x.tail_p1;
}

}  // namespace brotli_mi355x
#endif
