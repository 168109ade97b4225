// metablock_kernels.hip -- gfx950 kernels of the meta-block stage: per-granule histograms, greedy block
// splitting (one workgroup per splitter, strictly ordered f32 entropy sums), Huffman code construction
// (one wavefront per histogram), header serialisation (one wavefront per meta-block: the prefix beside the code jobs, the
// serialised trees appended behind them) and the parallel symbol
// emission (bit length per symbol -> prefix sums -> pieces ORed together per wavefront in LDS -> 64-bit atomic OR per stream
// word).  Integer/byte work, no MFMA.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <exception>

#include "device_api.h"
#include "device_scan.h"
#include "metablock_api.h"
#include "metablock_hq.h"

namespace brotli_mi355x {

size_t mb_scan_scratch_bytes(size_t n) { return scan_scratch_words(n) * 4 * 3 + 256; }  // (three arrays at once: exclusive_scan3_u32)

template <typename F>
__global__ __launch_bounds__(256) void k_for_each(uint32_t n, F f) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f(i);
}
template <typename F>
static void for_each(uint32_t n, F f) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_for_each<F>, dim3((n + 255) / 256), dim3(256), 0, BR_STREAM, n, f);
}

// out[m] = src[descs[m].cmd_offset] for every meta-block, out[n_mb] = src[n_cmds]: the per-meta-block boundaries of an
// exclusive scan over the commands, fetched with one copy instead of one per meta-block
void mb_gather_at_metablock_starts(const MbBuffers& B, const uint32_t* src, uint32_t* out_dev) {
  const MbBuffers b = B;
  for_each(b.n_mb + 1, [b, src, out_dev] __device__(uint32_t m) { out_dev[m] = src[m < b.n_mb ? b.descs[m].cmd_offset : b.n_cmds]; });
  HIP_CHECK(hipGetLastError());
}

void mb_gather_bytes(const uint8_t* text, const uint32_t* positions_dev, uint32_t n, uint8_t* out_dev) {
  for_each(n, [text, positions_dev, out_dev] __device__(uint32_t i) {
    const uint32_t p = positions_dev[i];
    out_dev[i] = p == 0xffffffffu ? (uint8_t)0 : text[p];
  });
  HIP_CHECK(hipGetLastError());
}

// ---- exclusive prefix sums of three uint32 arrays of one length (in place), with the tiling of exclusive_scan_u32 (device_scan.h):
// a workgroup takes the same tile of all three, the tile sums are three arrays again.  The three command scans are one pass of
// 5 launches at 64 MiB instead of three passes of 5.
struct ScanTriple {
  uint32_t* a[3];
};
__global__ __launch_bounds__(256) void k_scan3_tiles(ScanTriple data, uint32_t n, ScanTriple tile_sums, uint32_t want_sums) {
  __shared__ uint32_t wave_sum[3][4];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t v[3][4], local[3], x[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[q][j] = (base + j < n) ? data.a[q][base + j] : 0;
    local[q] = v[q][0] + v[q][1] + v[q][2] + v[q][3];
    x[q] = local[q];
    // inclusive scan across the wavefront
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x[q], off, 64);
      if (lane >= off) x[q] += y;
    }
    if (lane == 63) wave_sum[q][w] = x[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    uint32_t wave_off = 0;
    for (int i = 0; i < w; ++i) wave_off += wave_sum[q][i];
    uint32_t excl = wave_off + x[q] - local[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (base + j < n) data.a[q][base + j] = excl;
      excl += v[q][j];
    }
    if (threadIdx.x == 255 && want_sums) tile_sums.a[q][blockIdx.x] = wave_off + x[q];
  }
}
__global__ __launch_bounds__(256) void k_scan3_add(ScanTriple data, uint32_t n, ScanTriple tile_offsets) {
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint32_t add = tile_offsets.a[q][blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (base + j < n) data.a[q][base + j] += add;
  }
}
// scratch: three times what exclusive_scan_u32 wants for n
static void exclusive_scan3_u32(const ScanTriple& data, uint32_t n, uint32_t* scratch) {
  if (n == 0) return;
  const uint32_t tiles = (n + kScanTile - 1) / kScanTile;
  const ScanTriple sums = {{scratch, scratch + tiles, scratch + 2 * (size_t)tiles}};
  hipLaunchKernelGGL(k_scan3_tiles, dim3(tiles), dim3(256), 0, BR_STREAM, data, n, sums, tiles > 1 ? 1u : 0u);
  if (tiles > 1) {
    exclusive_scan3_u32(sums, tiles, scratch + 3 * (size_t)tiles);
    hipLaunchKernelGGL(k_scan3_add, dim3(tiles), dim3(256), 0, BR_STREAM, data, n, sums);
  }
}
// C-ABI test entry (tests/test_header_prefix_gpu.py): the three arrays of n words each, back to back in `host`, scanned in place
extern "C" int brotli_mi355x_debug_scan3(uint32_t* host, uint32_t n) {
  if (!host || n == 0 || n > (1u << 26)) return -1;
  try {
    DevBlocks tmp;
    uint32_t* dev = tmp.uninit<uint32_t>(((size_t)n + 4) * 3 * 4);
    uint32_t* scratch = tmp.uninit<uint32_t>(mb_scan_scratch_bytes(n));
    const size_t stride = ((size_t)n + 3) & ~(size_t)3;
    for (int q = 0; q < 3; ++q) dev_h2d(dev + q * stride, host + (size_t)q * n, (size_t)n * 4);
    exclusive_scan3_u32(ScanTriple{{dev, dev + stride, dev + 2 * stride}}, n, scratch);
    HIP_CHECK(hipGetLastError());
    for (int q = 0; q < 3; ++q) dev_d2h(host + (size_t)q * n, dev + q * stride, (size_t)n * 4);
    tmp.clear();
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

void mb_command_scans(const MbBuffers& B, void* scan_scratch) {
  const MbBuffers b = B;
  // (element [K] = 0 so that the exclusive scans leave the totals there)
  for_each(b.n_cmds + 1, [b] __device__(uint32_t c) {
    if (c < b.n_cmds) {
      mb_item_command_counts(b, c);
    } else {
      b.cmd_lit_start[c] = 0;
      b.cmd_pos[c] = 0;
      b.cmd_dist_index[c] = 0;
    }
  });
  exclusive_scan3_u32(ScanTriple{{b.cmd_lit_start, b.cmd_pos, b.cmd_dist_index}}, b.n_cmds + 1, (uint32_t*)scan_scratch);
  HIP_CHECK(hipGetLastError());
}

void mb_literal_map(const MbBuffers& B) {
  const MbBuffers b = B;
  for_each(b.n_lits, [b] __device__(uint32_t i) { mb_item_literal_map(b, i); });
  HIP_CHECK(hipGetLastError());
}

// sampled context statistics (encode.rs:1802-1927): a 64-byte sample every 4096 bytes of the meta-block.  One wavefront per sample,
// lane k holds byte k (one coalesced load) and takes its two predecessors from the lanes below; the workgroups of a meta-block
// share its samples and add their counters to its row of `stats` (zeroed by the caller; integer sums, so the order is free).
static constexpr uint32_t kStatsChunks = 64;  // workgroups per meta-block: 2048 samples of an 8 MiB meta-block are 8 per wavefront
__global__ __launch_bounds__(256) void k_context_stats(MbBuffers B, uint32_t* stats) {
  __shared__ uint32_t s[kContextStatsWords];
  const uint32_t m = blockIdx.y;
  const MbDesc d = B.descs[m];
  const uint32_t length = d.end - d.start;
  const uint32_t n_strides = length >= 64 ? (length - 64) / 4096 + 1 : 0;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = kStatsChunks * 4;
  if (blockIdx.x * 4 >= n_strides) return;  // (the whole workgroup)
  for (uint32_t j = threadIdx.x; j < kContextStatsWords; j += blockDim.x) s[j] = 0;
  __syncthreads();
  const uint8_t* text = B.text + d.start + lane;
  constexpr uint32_t kBatch = 4;  // loads in flight per wavefront
  for (uint32_t t0 = blockIdx.x * 4 + wave; t0 < n_strides; t0 += n_waves * kBatch) {
    uint32_t bytes[kBatch];
    for (uint32_t u = 0; u < kBatch; ++u) {
      const uint32_t t = t0 + u * n_waves;
      bytes[u] = t < n_strides ? text[(size_t)t * 4096] : 0u;
    }
    for (uint32_t u = 0; u < kBatch; ++u) {
      if (t0 + u * n_waves >= n_strides) break;  // (wave-uniform)
      const uint32_t literal = bytes[u];
      const uint32_t prev1 = (uint32_t)__shfl_up((int)literal, 1, 64), prev2 = (uint32_t)__shfl_up((int)literal, 2, 64);
      // simple bigram-prefix histogram (encode.rs:1885-1918): nine counters, counted across the lanes
      {
        const uint32_t lut = 0x90u;  // {0, 0, 1, 2}, two bits each
        const uint32_t bin = ((lut >> ((prev1 >> 6) * 2)) & 3u) * 3u + ((lut >> ((literal >> 6) * 2)) & 3u);
        uint32_t mine = 0;
        for (uint32_t b = 0; b < 9; ++b) {
          const uint32_t count = (uint32_t)__popcll(__ballot(lane >= 1 && bin == b));
          if (lane == b) mine = count;
        }
        if (mine) atomicAdd(&s[lane], mine);
      }
      // complex context statistics (encode.rs:1820-1842); the combined histogram [16..48) is the sum of the per-context ones
      // and the total [480] is 62 per sample: both are filled in when the counters leave the workgroup
      if (lane >= 2) {
        const uint32_t context = br_static_context_map(3, br_context(B.utf8_lut, B.signed_lut, (uint8_t)prev1, (uint8_t)prev2, 2));
        atomicAdd(&s[48 + context * 32 + (literal >> 3)], 1u);
      }
      if (lane == 0) atomicAdd(&s[480], 62u);
    }
  }
  __syncthreads();
  uint32_t* row = stats + (size_t)m * kContextStatsWords;
  for (uint32_t j = threadIdx.x; j < kContextStatsWords; j += blockDim.x) {
    uint32_t v = s[j];
    if (j >= 16 && j < 48)
      for (uint32_t c = 0; c < 13; ++c) v += s[48 + c * 32 + (j - 16)];
    if (v) atomicAdd(&row[j], v);
  }
}

void mb_context_stats(const MbBuffers& B, uint32_t* stats_dev) {
  if (B.n_mb == 0) return;
  // (a grid dimension holds 65 535 meta-blocks)
  for (uint32_t first = 0; first < B.n_mb; first += 32768) {
    MbBuffers b = B;
    b.descs += first;
    const uint32_t n = B.n_mb - first < 32768 ? B.n_mb - first : 32768;
    hipLaunchKernelGGL(k_context_stats, dim3(kStatsChunks, n), dim3(256), 0, BR_STREAM, b, stats_dev + (size_t)first * kContextStatsWords);
  }
  HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_granule_histograms(MbBuffers B, uint32_t kind) {
  __shared__ uint32_t lds[kMaxStaticContexts * 256];
  mb_item_granule_histogram(B, kind, blockIdx.x, lds);
}

void mb_granule_histograms(const MbBuffers& B) {
  const MbBuffers b = B;
  if (b.n_granules[kSplitLiteral]) hipLaunchKernelGGL(k_granule_histograms, dim3(b.n_granules[kSplitLiteral]), dim3(256), 0, BR_STREAM, b, (uint32_t)kSplitLiteral);
  if (b.n_granules[kSplitCommand]) hipLaunchKernelGGL(k_granule_histograms, dim3(b.n_granules[kSplitCommand]), dim3(256), 0, BR_STREAM, b, (uint32_t)kSplitCommand);
  if (b.n_granules[kSplitDistance]) {
    dev_memset(b.gran_hist[kSplitDistance], 0, (size_t)b.n_granules[kSplitDistance] * kNumDistanceHistoSymbols * 2);
    for_each(b.n_cmds, [b] __device__(uint32_t c) { mb_item_distance_count(b, c); });
  }
  HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(1024) void k_split_chains(MbBuffers B) {
  __shared__ SplitScratch S;
  mb_item_split_chain(B, blockIdx.x / 3, blockIdx.x % 3, S);
}

// `wide`: some meta-block models its literals with the 13-context map (39 histogram rows per decision instead of 3-9):
// 16 waves per chain take them side by side; otherwise 4 waves are enough and synchronise faster.
void mb_split_chains(const MbBuffers& B, bool wide) {
  if (B.n_mb == 0) return;
  hipLaunchKernelGGL(k_split_chains, dim3(B.n_mb * 3), dim3(wide ? 1024 : 256), 0, BR_STREAM, B);
  HIP_CHECK(hipGetLastError());
}

// The Huffman construction is sequential, data-dependent control flow: 64 different histograms in the lanes of one
// wavefront would serialise on every divergent branch.  One histogram per wavefront (lane 0 works) puts the jobs
// on different SIMDs instead, where they really run concurrently.
// everything the sequential builder touches is staged in LDS (its loads/stores are dependent, so their latency is
// what the job costs); the 64 lanes only help with the copies
struct CodeJobLds {
  HuffmanScratch sc;
  uint32_t h[704];
  uint16_t bits[704];
  uint8_t depth[704];
  uint64_t words[kTreeBitsWords];
  uint32_t nbits;
};
// The prefix of a meta-block's header (everything in front of the serialised trees, mb_item_header_prefix) is a sequential bit
// string that hangs on the splitter's results alone: one lane composes it -- in LDS, where a read-modify-write of the word under
// the cursor costs a few cycles instead of a trip to L2 -- beside the code jobs, in workgroups of their launch.
static constexpr uint32_t kHeaderPrefixWords = 2560;  // 20 KiB: the 160 Kibit bound for everything but the trees (a 16 Ki-entry context map)
struct HeaderPrefixLds {
  uint64_t window[kHeaderPrefixWords];
  HuffmanScratch sc;  // (the scratch of the small trees -- block-split codes, context map)
  MbSplitPrepared prep;
  uint32_t bits;
};
union BuildCodesLds {
  CodeJobLds code;
  HeaderPrefixLds prefix;
};

__device__ __forceinline__ void mb_code_job(const MbBuffers& B, const CodeJob& j, CodeJobLds& S) {
  const uint32_t row = kRowLen[j.kind];
  uint32_t* gh = B.histo[j.kind] + (size_t)j.row_index * row;
  for (uint32_t k = threadIdx.x; k < row; k += 64) S.h[k] = gh[k];
  __syncthreads();
  {
    const uint32_t nb = mb_build_code_core(j.kind, j.num_distance_symbols, S.h, S.depth, S.bits, S.words, &S.sc, true, j.mode);
    if (threadIdx.x == 0) S.nbits = nb;
  }
  __syncthreads();
  uint8_t* gd = B.depth[j.kind] + (size_t)j.row_index * row;
  uint16_t* gb = B.bits[j.kind] + (size_t)j.row_index * row;
  uint64_t* gw = B.tree_bits[j.kind] + (size_t)j.row_index * kTreeBitsWords;
  for (uint32_t k = threadIdx.x; k < row; k += 64) {
    gh[k] = S.h[k];
    gd[k] = S.depth[k];
    gb[k] = S.bits[k];
  }
  for (uint32_t k = threadIdx.x; k < kTreeBitsWords; k += 64) gw[k] = S.words[k];
  if (threadIdx.x == 0) B.tree_nbits[j.kind][j.row_index] = S.nbits;
}

// The block-split codes (BuildAndStoreBlockSplitCode) walk all blocks of a kind twice -- the histograms of the type and length
// codes, then the switch command of every block: a block per lane in front of and behind the one lane that composes the prefix
// (a meta-block of a mix has thousands of blocks: 4.8 ms of a 256 MiB Silesia-like call were this walk in one lane).
__device__ __forceinline__ void mb_header_prefix_job(const MbBuffers& B, uint32_t m, HeaderPrefixLds& S) {
  const MbDesc d = B.descs[m];
  if (d.uncompressed) {  // (the whole workgroup)
    if (threadIdx.x == 0) B.header_prefix_bits[m] = 0;
    return;
  }
  for (uint32_t i = threadIdx.x; i < kHeaderPrefixWords; i += 64) S.window[i] = 0;
  for (uint32_t i = threadIdx.x; i < 3 * (258 + 26); i += 64) (&S.prep.histograms[0][0])[i] = 0;
  __syncthreads();
  for (uint32_t kind = 0; kind < 3; ++kind) {
    const uint8_t* types = B.block_types[kind] + d.block_base[kind];
    const uint32_t* lengths = B.block_lengths[kind] + d.block_base[kind];
    const uint32_t nb = B.results[m].num_blocks[kind];
    for (uint32_t i = threadIdx.x; i < nb; i += 64) {
      if (i != 0) atomicAdd(&S.prep.histograms[kind][br_block_type_code_at(types, i)], 1u);
      atomicAdd(&S.prep.histograms[kind][258 + br_block_length_prefix_code(lengths[i])], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) S.bits = mb_item_header_prefix(B, m, &S.sc, S.window, &S.prep);
  __syncthreads();
  for (uint32_t kind = 0; kind < 3; ++kind) {
    if (B.results[m].num_types[kind] <= 1) continue;
    const uint8_t* types = B.block_types[kind] + d.block_base[kind];
    const uint32_t* lengths = B.block_lengths[kind] + d.block_base[kind];
    uint64_t* switch_bits = B.switch_bits[kind] + d.block_base[kind];
    uint8_t* switch_nbits = B.switch_nbits[kind] + d.block_base[kind];
    const uint32_t nb = B.results[m].num_blocks[kind];
    for (uint32_t i = 1 + threadIdx.x; i < nb; i += 64) {
      uint32_t nbits;
      switch_bits[i] = br_block_switch_bits(S.prep.code[kind], br_block_type_code_at(types, i), lengths[i], false, &nbits);
      switch_nbits[i] = (uint8_t)nbits;
    }
  }
  uint64_t* global_words = B.header_words + (size_t)m * B.header_stride;
  const uint32_t words = (S.bits + 63) / 64;
  for (uint32_t i = threadIdx.x; i < words && i < kHeaderPrefixWords; i += 64) global_words[i] = S.window[i];
}

// workgroups [0, n_jobs): a code job each; the workgroups behind them: the header prefix of meta-block blockIdx.x - n_jobs.
// (The branches are workgroup-uniform, so is every return: no barrier is reached by a part of a workgroup.)
__global__ __launch_bounds__(64) void k_build_codes(MbBuffers B, const CodeJob* jobs, uint32_t n_jobs) {
  __shared__ BuildCodesLds S;
  const uint32_t i = blockIdx.x;
  if (i >= n_jobs) {
    if (i - n_jobs < B.n_mb) mb_header_prefix_job(B, i - n_jobs, S.prefix);
    return;
  }
  const CodeJob j = jobs[i];
  if (j.mb_plus_1 != 0 && j.slot >= B.results[j.mb_plus_1 - 1].num_histos[j.kind]) return;  // a pool slot the splitter left empty
  mb_code_job(B, j, S.code);
}

void mb_build_codes(const MbBuffers& B, const CodeJob* jobs_dev, uint32_t n_jobs) {
  if (n_jobs + B.n_mb == 0) return;
  hipLaunchKernelGGL(k_build_codes, dim3(n_jobs + B.n_mb), dim3(64), 0, BR_STREAM, B, jobs_dev, n_jobs);
  HIP_CHECK(hipGetLastError());
#if defined(BR_CODES_PROFILE)
  {
    unsigned long long h[32];
    HIP_CHECK(hipStreamSynchronize(BR_STREAM));
    HIP_CHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_codes_prof), sizeof(h)));
    fprintf(stderr, "codes profile (%u jobs), cycles sum / slowest job:", n_jobs);
    for (int i = 0; i < 16; ++i) fprintf(stderr, " [%d] %llu / %llu", i, h[i], h[16 + i]);
    fprintf(stderr, "\n");
    unsigned long long z[32] = {0};
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_codes_prof), z, sizeof(z)));
  }
#endif
}

// Behind the code jobs and the header prefixes: the serialised trees appended to every prefix.  One lane appends -- in LDS,
// as the prefix was composed -- and the wave brings the prefix in and the finished words out.  Headers that do not fit the
// LDS buffer (hundreds of literal histograms) are finished in global memory.
// lds_bits: the longest header (prefix + trees) that is staged in LDS, at most the buffer's kHeaderLdsWords * 64
static constexpr uint32_t kHeaderLdsWords = 5120;  // 40 KiB
__global__ __launch_bounds__(64) void k_write_headers(MbBuffers B, uint32_t lds_bits) {
  constexpr uint32_t kLdsWords = kHeaderLdsWords;
  __shared__ uint64_t lw[kLdsWords];
  __shared__ uint32_t s_bits;
  const uint32_t m = blockIdx.x;
  if (m >= B.n_mb) return;
  const MbDesc d = B.descs[m];
  if (d.uncompressed) {
    if (threadIdx.x == 0) B.results[m].header_bits = 0;
    return;
  }
  uint64_t* global_words = B.header_words + (size_t)m * B.header_stride;
  uint32_t trees = 0;
  for (uint32_t kind = 0; kind < 3; ++kind)
    for (uint32_t i = threadIdx.x; i < B.results[m].num_histos[kind]; i += 64) trees += B.tree_nbits[kind][d.histo_base[kind] + i];
  for (int off = 32; off > 0; off >>= 1) trees += __shfl_down(trees, off, 64);
  trees = (uint32_t)__shfl((int)trees, 0, 64);
  const uint32_t prefix_bits = B.header_prefix_bits[m];
  const uint64_t all_bits = (uint64_t)prefix_bits + trees;
  const bool in_lds = all_bits <= (uint64_t)lds_bits;
  // the words the header ends in (and one behind them, which the bit writer may OR a zero into), inside the staging
  const uint32_t limit = in_lds ? kLdsWords : B.header_stride;
  const uint32_t all_words = all_bits / 64 + 2 < limit ? (uint32_t)(all_bits / 64 + 2) : limit;
  const uint32_t prefix_words = (prefix_bits + 63) / 64;
  uint64_t* stage = in_lds ? lw : global_words;
  if (in_lds)
    for (uint32_t i = threadIdx.x; i < prefix_words; i += 64) lw[i] = global_words[i];
  for (uint32_t i = prefix_words + threadIdx.x; i < all_words; i += 64) stage[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    mb_item_header_trees(B, m, stage, prefix_bits);
    s_bits = B.results[m].header_bits;
  }
  __syncthreads();
  if (in_lds) {
    const uint32_t words = (s_bits + 63) / 64;
    for (uint32_t i = prefix_bits / 64 + threadIdx.x; i < words && i < kLdsWords; i += 64) global_words[i] = lw[i];
  }
}

void mb_write_headers(const MbBuffers& B) {
  if (B.n_mb == 0) return;
  // BROTLI_MI355X_TEST_HEADER_LDS_BITS (tests): a lower line between the two stagings -- a header past the buffer's 327 680 bits
  // takes hundreds of prefix codes of every kind, more than a quick test can bring about
  static const uint32_t lds_bits = [] {
    const char* e = getenv("BROTLI_MI355X_TEST_HEADER_LDS_BITS");
    const unsigned long v = e ? strtoul(e, nullptr, 10) : kHeaderLdsWords * 64ul;
    return (uint32_t)(v < kHeaderLdsWords * 64ul ? v : kHeaderLdsWords * 64ul);
  }();
  hipLaunchKernelGGL(k_write_headers, dim3(B.n_mb), dim3(64), 0, BR_STREAM, B, lds_bits);
  HIP_CHECK(hipGetLastError());
#if defined(BR_CODES_PROFILE)
  {
    unsigned long long h[16];
    HIP_CHECK(hipStreamSynchronize(BR_STREAM));
    HIP_CHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_header_prof), sizeof(h)));
    fprintf(stderr, "header profile (%u meta-blocks), cycles sum / slowest meta-block: block-split codes %llu / %llu, context maps %llu / %llu, trees %llu / %llu\n",
            B.n_mb, h[0], h[8], h[1], h[9], h[2], h[10]);
    unsigned long long z[16] = {0};
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_header_prof), z, sizeof(z)));
  }
#endif
}

void mb_symbol_bits(const MbBuffers& B, void* scan_scratch) {
  const MbBuffers b = B;
  for_each(b.n_lits, [b] __device__(uint32_t i) { mb_item_literal_nbits(b, i); });
  dev_memset(b.lit_nbits + b.n_lits, 0, 4);
  exclusive_scan_u32(b.lit_nbits, b.n_lits + 1, (uint32_t*)scan_scratch);
  for_each(b.n_cmds, [b] __device__(uint32_t c) { mb_item_command_nbits(b, c); });
  dev_memset(b.cmd_nbits + b.n_cmds, 0, 4);
  exclusive_scan_u32(b.cmd_nbits, b.n_cmds + 1, (uint32_t*)scan_scratch);
  HIP_CHECK(hipGetLastError());
}

// ---- emission.  An item's pieces are a few bits each, and neighbouring items write neighbouring bits: a wavefront takes 64
// consecutive items and collects their pieces in a window of kWords 64-bit words of workgroup memory that starts at the stream word
// of its first item, then ORs every non-zero word of the window into the stream once.  A piece that does not lie wholly inside the
// window -- behind a long literal run, behind the header of the next meta-block, across the window's end -- goes to the stream by
// itself, as every piece does with MbAtomicSink.  Everything is an OR into zero-filled words, so no order is assumed anywhere.
template <uint32_t kWords>
struct MbWindowSink {
  uint64_t* words;            // the stream
  unsigned long long* window; // kWords words of workgroup memory, this wavefront's own
  uint64_t first_word;        // stream word of window[0]
  __device__ __forceinline__ void put(uint64_t pos, uint32_t nbits, uint64_t bits) const {
    if (nbits == 0) return;
    const uint32_t sh = (uint32_t)(pos & 63u);
    const uint64_t at = (pos >> 6) - first_word;  // (a word in front of the window: a huge number)
    const bool two = sh + nbits > 64;
    if (at < kWords && (!two || at + 1 < kWords)) {
      atomicOr(window + at, (unsigned long long)(bits << sh));
      if (two) atomicOr(window + at + 1, (unsigned long long)(bits >> (64 - sh)));
    } else {
      mb_put_bits_atomic(words, pos, nbits, bits);
    }
  }
};

// 64 commands of text are about 25 words, 64 literals and the commands between them about 15.  Measured on the 64 MiB text
// workload, k_emit_commands takes the same 0.100 ms with windows of 64, 128 and 256 words.
static constexpr uint32_t kEmitCommandWindow = 128;
static constexpr uint32_t kEmitLiteralWindow = 64;

// first(i, &bit): where item i starts in the stream, false if it has nothing to emit; emit(i, bit, sink): its pieces
template <uint32_t kWords, typename First, typename Emit>
__device__ __forceinline__ void mb_emit_wave(const MbBuffers& B, uint32_t n, unsigned long long* windows, First first, Emit emit) {
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long* window = windows + (threadIdx.x >> 6) * kWords;
  for (uint32_t j = lane; j < kWords; j += 64) window[j] = 0;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t bit = 0;
  const bool mine = i < n && first(i, &bit);
  // the window starts at the first item of the wavefront that emits anything
  const unsigned long long emitting = __ballot(mine);
  uint64_t first_word = 0;
  if (emitting) first_word = (uint64_t)__shfl((unsigned long long)(bit >> 6), __ffsll(emitting) - 1, 64);
  __syncthreads();
  if (mine) emit(i, bit, MbWindowSink<kWords>{B.out_words, window, first_word});
  __syncthreads();
  // (a non-zero word holds a piece of the stream, so it lies inside out_words)
  for (uint32_t j = lane; j < kWords; j += 64) {
    const unsigned long long v = window[j];
    if (v) atomicOr((unsigned long long*)B.out_words + first_word + j, v);
  }
}

__global__ __launch_bounds__(256) void k_emit_commands(MbBuffers B) {
  __shared__ unsigned long long windows[4 * kEmitCommandWindow];
  uint32_t m = 0;  // (each lane's own: set by first, read by emit)
  mb_emit_wave<kEmitCommandWindow>(
      B, B.n_cmds, windows, [&](uint32_t c, uint64_t* bit) { return mb_command_base(B, c, &m, bit); },
      [&](uint32_t c, uint64_t bit, const MbWindowSink<kEmitCommandWindow>& sink) { mb_emit_command_pieces(B, c, m, bit, sink); });
}

__global__ __launch_bounds__(256) void k_emit_literals(MbBuffers B) {
  __shared__ unsigned long long windows[4 * kEmitLiteralWindow];
  mb_emit_wave<kEmitLiteralWindow>(
      B, B.n_lits, windows, [&](uint32_t i, uint64_t* bit) { return mb_literal_base(B, i, bit); },
      [&](uint32_t i, uint64_t bit, const MbWindowSink<kEmitLiteralWindow>& sink) {
        const SymbolCode sc = mb_literal_code(B, i);
        sink.put(bit, sc.nbits, sc.bits);
      });
}

void mb_emit(const MbBuffers& B) {
  if (B.n_cmds) hipLaunchKernelGGL(k_emit_commands, dim3((B.n_cmds + 255) / 256), dim3(256), 0, BR_STREAM, B);
  if (B.n_lits) hipLaunchKernelGGL(k_emit_literals, dim3((B.n_lits + 255) / 256), dim3(256), 0, BR_STREAM, B);
  HIP_CHECK(hipGetLastError());
}

// every piece by itself (MbAtomicSink), into `out_words` instead of B.out_words: what mb_emit is checked against
void mb_emit_piecewise(const MbBuffers& B, uint64_t* out_words) {
  MbBuffers b = B;
  b.out_words = out_words;
  for_each(b.n_cmds, [b] __device__(uint32_t c) { mb_item_emit_command(b, c); });
  for_each(b.n_lits, [b] __device__(uint32_t i) { mb_item_emit_literal(b, i); });
  HIP_CHECK(hipGetLastError());
}

// ---- quality >= 10: one lane per sequential job (metablock_hq.h says why), all lanes for the per-symbol passes
__global__ __launch_bounds__(256) void k_hq_utf8_census(MbBuffers B) {
  __shared__ HqCensusScratch S;
  if (!B.descs[blockIdx.x].uncompressed) hq_item_utf8_census(B, blockIdx.x, S);
}
void mb_hq_utf8_census(const MbBuffers& B) {
  if (B.n_mb == 0) return;
  hipLaunchKernelGGL(k_hq_utf8_census, dim3(B.n_mb), dim3(256), 0, BR_STREAM, B);
  HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(64) void k_hq_distance_params(MbBuffers B) {
  __shared__ HqWaveScratch S;
  hq_item_distance_params(B, blockIdx.x, S);
}
void mb_hq_distance_params(const MbBuffers& B) {
  if (B.n_mb == 0) return;
  hipLaunchKernelGGL(k_hq_distance_params, dim3(B.n_mb), dim3(64), 0, BR_STREAM, B);
  HIP_CHECK(hipGetLastError());
}
void mb_hq_gather_symbols(const MbBuffers& B) {
  const MbBuffers b = B;
  for_each(b.n_lits, [b] __device__(uint32_t i) { hq_item_literal_symbol(b, i); });
  for_each(b.n_cmds, [b] __device__(uint32_t c) { hq_item_command_symbols(b, c); });
  HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(64) void k_hq_find_blocks(EntropyTables et, HqSplitJob* jobs) {
  __shared__ HqWaveScratch S;
  hq_item_find_blocks(et, jobs[blockIdx.x], S);
}
void mb_hq_find_blocks(const MbBuffers& B, HqSplitJob* jobs_dev, uint32_t n_jobs) {
  if (n_jobs == 0) return;
  hipLaunchKernelGGL(k_hq_find_blocks, dim3(n_jobs), dim3(64), 0, BR_STREAM, B.et, jobs_dev);
  HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(64) void k_hq_blocks_prep(const HqSplitJob* jobs) { hq_item_blocks_prep(jobs[blockIdx.x]); }
__global__ __launch_bounds__(64) void k_hq_cluster_blocks_batch(EntropyTables et, const HqSplitJob* jobs, const HqBatchRef* batches) {
  __shared__ HqWaveScratch S;
  __shared__ HqBatchPairs P;
  const HqBatchRef ref = batches[blockIdx.x];
  hq_item_cluster_blocks_batch(et, jobs[ref.job], ref.batch, S, P.pairs);
}
__global__ __launch_bounds__(64) void k_hq_cluster_blocks(MbBuffers B, const HqSplitJob* jobs) {
  __shared__ HqWaveScratch S;
  hq_item_cluster_blocks(B, jobs[blockIdx.x], S);
}
void mb_hq_cluster_blocks(const MbBuffers& B, const HqSplitJob* jobs_dev, uint32_t n_jobs, const HqBatchRef* batches_dev, uint32_t n_batches) {
  if (n_jobs == 0) return;
  hipLaunchKernelGGL(k_hq_blocks_prep, dim3(n_jobs), dim3(64), 0, BR_STREAM, jobs_dev);
  if (n_batches) hipLaunchKernelGGL(k_hq_cluster_blocks_batch, dim3(n_batches), dim3(64), 0, BR_STREAM, B.et, jobs_dev, batches_dev);
  hipLaunchKernelGGL(k_hq_cluster_blocks, dim3(n_jobs), dim3(64), 0, BR_STREAM, B, jobs_dev);
  HIP_CHECK(hipGetLastError());
}
void mb_hq_context_histograms(const MbBuffers& B) {
  const MbBuffers b = B;
  for_each(b.n_lits, [b] __device__(uint32_t i) { hq_item_literal_context_count(b, i); });
  for_each(b.n_cmds, [b] __device__(uint32_t c) { hq_item_command_context_count(b, c); });
  HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(64) void k_hq_cluster_histograms_batch(EntropyTables et, const HqClusterJob* jobs, const HqBatchRef* batches) {
  __shared__ HqWaveScratch S;
  __shared__ HqBatchPairs P;
  const HqBatchRef ref = batches[blockIdx.x];
  hq_item_cluster_histograms_batch(et, jobs[ref.job], ref.batch, S, P.pairs);
}
__global__ __launch_bounds__(64) void k_hq_cluster_histograms(MbBuffers B, const HqClusterJob* jobs) {
  __shared__ HqWaveScratch S;
  hq_item_cluster_histograms(B, jobs[blockIdx.x], S);
}
void mb_hq_cluster_histograms(const MbBuffers& B, const HqClusterJob* jobs_dev, uint32_t n_jobs, const HqBatchRef* batches_dev,
                              uint32_t n_batches) {
  if (n_jobs == 0) return;
  if (n_batches) hipLaunchKernelGGL(k_hq_cluster_histograms_batch, dim3(n_batches), dim3(64), 0, BR_STREAM, B.et, jobs_dev, batches_dev);
  hipLaunchKernelGGL(k_hq_cluster_histograms, dim3(n_jobs), dim3(64), 0, BR_STREAM, B, jobs_dev);
  HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_copy_bits_batch(unsigned long long* __restrict__ out, const uint64_t* __restrict__ src_words,
                                                          const MbBitCopy* __restrict__ items) {
  const MbBitCopy it = items[blockIdx.y];
  const uint64_t* src = src_words + it.src_word;
  const uint64_t chunks = (it.nbits + 63) >> 6;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t v = src[c];
    const uint64_t left = it.nbits - (c << 6);
    if (left < 64) v &= (1ull << left) - 1ull;
    if (v == 0) continue;
    const uint64_t d = it.dst_bit + (c << 6);
    const uint32_t dh = (uint32_t)(d & 63u);
    atomicOr(out + (d >> 6), (unsigned long long)(v << dh));
    if (dh != 0 && (v >> (64u - dh)) != 0) atomicOr(out + (d >> 6) + 1, (unsigned long long)(v >> (64u - dh)));
  }
}
void mb_copy_bits_batch(uint64_t* out, const uint64_t* src_words, const MbBitCopy* items_dev, uint32_t n) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_copy_bits_batch, dim3(8, n), dim3(256), 0, BR_STREAM, (unsigned long long*)out, src_words, items_dev);
  HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(256) void k_place_pieces(unsigned long long* __restrict__ out, const MbBitPiece* __restrict__ pieces, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MbBitPiece pc = pieces[i];
  uint64_t v = pc.bits;
  if (pc.nbits < 64) v &= (1ull << pc.nbits) - 1ull;
  if (v == 0) return;
  const uint32_t dh = (uint32_t)(pc.pos & 63u);
  atomicOr(out + (pc.pos >> 6), (unsigned long long)(v << dh));
  if (dh != 0 && (v >> (64u - dh)) != 0) atomicOr(out + (pc.pos >> 6) + 1, (unsigned long long)(v >> (64u - dh)));
}
void mb_place_pieces(uint64_t* out, const MbBitPiece* pieces_dev, uint32_t n) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_place_pieces, dim3((n + 255) / 256), dim3(256), 0, BR_STREAM, (unsigned long long*)out, pieces_dev, n);
  HIP_CHECK(hipGetLastError());
}
// (byte-aligned destinations: a stored meta-block starts behind a jump to the byte boundary; 16 bytes per thread where both sides
// allow it, single bytes at the ragged ends)
__global__ __launch_bounds__(256) void k_raw_copies(uint8_t* __restrict__ out, const uint8_t* __restrict__ text, const MbRawCopy* __restrict__ items) {
  const MbRawCopy it = items[blockIdx.y];
  uint8_t* dst = out + it.dst_byte;
  const uint8_t* src = text + it.src_pos;
  // head up to the first 16-byte boundary of the destination
  uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
  if (head > it.bytes) head = it.bytes;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  for (uint32_t i = t; i < head; i += nt) dst[i] = src[i];
  const uint32_t body = (it.bytes - head) / 16u;
  typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
  typedef uint32_t u32x4_a __attribute__((ext_vector_type(4)));
  for (uint32_t i = t; i < body; i += nt) *(u32x4_a*)(dst + head + 16u * i) = *(const u32x4_u*)(src + head + 16u * i);
  for (uint32_t i = head + 16u * body + t; i < it.bytes; i += nt) dst[i] = src[i];
}
void mb_raw_copies(uint8_t* out_bytes, const uint8_t* text, const MbRawCopy* items_dev, uint32_t n) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_raw_copies, dim3(64, n), dim3(256), 0, BR_STREAM, out_bytes, text, items_dev);
  HIP_CHECK(hipGetLastError());
}

void mb_copy_bits(uint64_t* out, uint64_t dst_bit, const uint64_t* src, uint64_t nbits) {
  const uint32_t words = (uint32_t)((nbits + 63) / 64);
  for_each(words, [=] __device__(uint32_t w) { mb_item_copy_bits_word(out, dst_bit, src, nbits, w); });
  HIP_CHECK(hipGetLastError());
}

}  // namespace brotli_mi355x
