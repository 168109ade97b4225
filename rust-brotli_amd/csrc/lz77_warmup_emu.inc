// lz77_warmup_emu.inc -- host emulation of the seam that composes the entries of round 0 from the dry runs on the device
// (device_api.h: lz77_warmup_prepare, lz77_warmup_compose), compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu;
// lz77_stage.cpp includes it there): the same item code (lz77_warmup.h) in the same tile structure as the kernels
// (lz77_kernels.hip, k_warmup_*) -- aggregates per tile of kWarmupTile dry runs, a carry across the tiles, the scan inside every
// tile once more on top of its carry, and one walk per run of segments without commands, begun at the run's first segment.

namespace brotli_mi355x {

void lz77_warmup_prepare(const Lz77Params& P, const Lz77Buffers& B, const WarmupShape& S, const WarmupBuffers& W, const int32_t base_cache[4]) {
  for (uint32_t k = 0; k < S.num_segments; ++k) {
    if (k == 0) W.fc_death[0] = S.num_segments;
    const Segment g = B.segments[k];
    SegEntry e{};
    e.pos = g.start;
    e.apply = g.start + P.spree_window;
    for (int c = 0; c < 4; ++c) e.cache[c] = base_cache[c];
    if (k != 0) {
      e.dict_lookups = kWarmAliveL;
      e.dict_matches = kWarmAliveM;
    }
    B.entries[k] = e;
    if (k + 1 < S.num_segments) {
      const Segment dry = warmup_segment(g, S.warmup_bytes);
      W.segs[k] = dry;
      W.entries[k] = warmup_entry(e, dry, P.spree_window, false);
    }
  }
}

void lz77_warmup_compose(const Lz77Params& P, const Lz77Buffers& B, const WarmupShape& S, const WarmupBuffers& W) {
  if (S.num_segments < 2) return;
  const uint32_t count = S.num_segments - 1;
  const uint32_t tiles = (count + kWarmupTile - 1) / kWarmupTile;
  auto op_of = [&](uint32_t i) { return warmup_op(B.segments[i], W.exits[i], W.entries[i].dict_lookups, W.entries[i].dict_matches, S.warmup_bytes); };
  // k_warmup_tile_ops
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    WarmupOp acc = warmup_identity();
    for (uint32_t i = tile * kWarmupTile; i < count && i < (tile + 1) * kWarmupTile; ++i) acc = warmup_combine(acc, op_of(i));
    W.tile_ops[tile] = acc;
  }
  // k_warmup_tile_carry
  WarmupOp carry = warmup_identity();
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    W.tile_ops[tiles + tile] = carry;
    carry = warmup_combine(carry, W.tile_ops[tile]);
  }
  // k_warmup_entries
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    WarmupOp upto = W.tile_ops[tiles + tile];
    for (uint32_t i = tile * kWarmupTile; i < count && i < (tile + 1) * kWarmupTile; ++i) {
      upto = warmup_combine(upto, op_of(i));
      SegEntry e = B.entries[i + 1];
      warmup_apply_cache(upto, B.entries[0].cache, e.cache);
      warmup_entry_from_exit(B.segments[i], B.segments[i + 1], W.exits[i], P.max_backward_limit, &e);
      B.entries[i + 1] = e;
      if (P.use_dictionary && warmup_dictionary_dies(upto.sl, upto.sm, S.warmup_bytes, S.segment_bytes) && i < W.fc_death[0]) W.fc_death[0] = i;
    }
  }
  // k_warmup_finish
  auto carries = [&](uint32_t j) { return warmup_spree_carries(B.segments[j], B.segments[j + 1], B.entries[j], W.exits[j]); };
  for (uint32_t k = 0; k < S.num_segments; ++k) {
    if (P.use_dictionary && k > W.fc_death[0]) {
      B.entries[k].dict_lookups = kWarmDeadL;
      B.entries[k].dict_matches = kWarmDeadM;
    }
  }
  for (uint32_t k = 0; k < count && S.spree_guess; ++k) {
    if (!carries(k) || (k > 0 && carries(k - 1))) continue;
    SegEntry cur = B.entries[k];
    for (uint32_t j = k; j < count && (j == k || carries(j)); ++j) {
      SegEntry next{};
      warmup_spree_step(P.htl, P.spree_window, B.segments[j], cur, &next);
      B.entries[j + 1].pos = next.pos;
      B.entries[j + 1].apply = next.apply;
      B.entries[j + 1].head_kind = next.head_kind;
      B.entries[j + 1].head_base = next.head_base;
      B.entries[j + 1].head_p1 = next.head_p1;
      cur = next;
    }
  }
}

}  // namespace brotli_mi355x
