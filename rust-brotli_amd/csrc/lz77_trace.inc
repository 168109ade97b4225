// lz77_trace.inc -- introspection entry point: runs only the backward-reference stage and returns the
// commands and meta-block plan (for parity tests against the oracle's command trace).
#include <string.h>

#include <stdexcept>
#include <vector>

#include "encoder_params.h"
#include "lz77_stage.h"
#include "encoder.h"

using namespace brotli_mi355x;

extern "C" {

struct BrotliMi355xMetaBlockInfo {
  uint32_t start, end, cmd_offset, n_cmds, n_literals, uncompressed, is_last, pad;
  int32_t dist_cache_after[4];
};

// Returns the number of commands (or -1 on error; message in err).  cmds_out may be NULL to query.
// test hook: when set, the final stored/searched flags of the next trace call are copied here (prefix included)
static uint8_t* g_flag_dump = nullptr;
static size_t g_flag_dump_size = 0;
void brotli_mi355x_debug_set_flag_dump(uint8_t* buf, size_t size) {
  g_flag_dump = buf;
  g_flag_dump_size = size;
}

long brotli_mi355x_lz77_trace(int quality, int lgwin, uint32_t size_hint, int catable, const uint8_t* prefix,
                              uint32_t prefix_bytes, const uint8_t* input, uint32_t input_bytes,
                              uint32_t segment_bytes, Command* cmds_out, size_t cmds_capacity,
                              BrotliMi355xMetaBlockInfo* mb_out, size_t mb_capacity, size_t* n_metablocks,
                              uint32_t* stats_out /* [12]: rounds, segments_parsed, searches, total_cmds, then us per phase */, char* err,
                              size_t err_len) {
  try {
    EncoderParams p;
    SetParameter(&p, kParamQuality, (uint32_t)quality);
    SetParameter(&p, kParamLgwin, (uint32_t)lgwin);
    SetParameter(&p, kParamSizeHint, size_hint);
    if (catable) SetParameter(&p, kParamCatable, 1);
    if (prefix_bytes) p.use_dictionary = false;
    FinalizeParams(&p);
    ChooseHasher(&p);
    const char* why = nullptr;
    if (!IsAccelerated(p, &why)) throw std::runtime_error(why);
    const uint32_t M = prefix_bytes + input_bytes;
    DevBlocks tmp;
    uint8_t* text = tmp.zeroed<uint8_t>((size_t)M + 64);
    if (prefix_bytes) dev_h2d(text, prefix, prefix_bytes);
    dev_h2d(text + prefix_bytes, input, input_bytes);
    Lz77Stage stage;
    uint32_t raw_head = catable ? (input_bytes < 2 ? input_bytes : 2) : 0;
    stage.Setup(p, text, prefix_bytes, input_bytes, raw_head, segment_bytes ? segment_bytes : ChooseSegmentBytes(input_bytes));  // (0: as EncodeStream cuts it)
    stage.Run();
    if (g_flag_dump) stage.DumpFlags(g_flag_dump, g_flag_dump_size);
    const size_t n = stage.num_commands();
    if (cmds_out) {
      if (n > cmds_capacity) throw std::runtime_error("command buffer too small");
      dev_d2h(cmds_out, stage.commands_dev(), n * sizeof(Command));
    }
    const auto& mbs = stage.metablocks();
    if (n_metablocks) *n_metablocks = mbs.size();
    if (mb_out) {
      for (size_t i = 0; i < mbs.size() && i < mb_capacity; ++i) {
        mb_out[i].start = mbs[i].start;
        mb_out[i].end = mbs[i].end;
        mb_out[i].cmd_offset = mbs[i].cmd_offset;
        mb_out[i].n_cmds = mbs[i].n_cmds;
        mb_out[i].n_literals = mbs[i].n_literals;
        mb_out[i].uncompressed = mbs[i].uncompressed;
        mb_out[i].is_last = mbs[i].is_last;
        memcpy(mb_out[i].dist_cache_after, mbs[i].dist_cache_after, 16);
      }
    }
    if (stats_out) {
      stats_out[0] = stage.stats().rounds;
      stats_out[1] = (uint32_t)stage.stats().segments_parsed;
      stats_out[2] = (uint32_t)stage.stats().searches;
      stats_out[3] = (uint32_t)stage.stats().total_commands;
      const Lz77Stats& st = stage.stats();
      const double ms[8] = {st.ms_keys, st.ms_sort, st.ms_init, st.ms_rank, st.ms_parse, st.ms_resolve, st.ms_gather, st.ms_total};
      for (int i = 0; i < 8; ++i) stats_out[4 + i] = (uint32_t)(ms[i] * 1000.0);  // microseconds
    }
    tmp.clear();
    return (long)n;
  } catch (const std::exception& e) {
    if (err && err_len) {
      strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return -1;
  }
}

// Test hook for lz77_check_cache (one segment [seg_start, seg_end) of `text`, `flags` = stored / searched bits per
// position): returns 1 when none of the ndist candidate distances derived from `cache` matches two bytes at a searched
// position, 0 when one does, -1 on error.
int brotli_mi355x_debug_check_cache(const uint8_t* text, const uint8_t* flags, uint32_t n, uint32_t seg_start, uint32_t seg_end,
                                    const int32_t* cache, uint32_t ndist, uint32_t max_backward_limit) {
  try {
    Lz77Params P{};
    P.total_bytes = n;
    P.ndist = ndist;
    P.max_backward_limit = max_backward_limit;
    Lz77Buffers B{};
    DevBlocks tmp;
    B.text = tmp.zeroed<uint8_t>((size_t)n + 64);
    B.flags[0] = tmp.zeroed<uint8_t>((size_t)n + 64);
    B.segments = tmp.zeroed<Segment>(sizeof(Segment));
    CacheCheck* item_dev = tmp.zeroed<CacheCheck>(sizeof(CacheCheck));
    uint8_t* ok_dev = tmp.zeroed<uint8_t>(64);
    Segment seg{};
    seg.start = seg_start;
    seg.end = seg_end;
    seg.blk_start = 0;
    seg.blk_end = n;
    CacheCheck item{};
    item.segment = 0;
    memcpy(item.cache, cache, sizeof(item.cache));
    dev_h2d(B.text, text, n);
    dev_h2d(B.flags[0], flags, n);
    dev_h2d(B.segments, &seg, sizeof(seg));
    dev_h2d(item_dev, &item, sizeof(item));
    lz77_check_cache(P, B, 0, item_dev, 1, ok_dev);
    uint8_t ok = 0;
    dev_d2h(&ok, ok_dev, 1);
    return ok ? 1 : 0;
  } catch (const std::exception&) {
    return -1;
  }
}
}
