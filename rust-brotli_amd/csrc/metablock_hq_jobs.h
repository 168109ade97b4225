// metablock_hq_jobs.h -- host side of metablock_hq.h: the job tables of BrotliSplitBlock and BrotliClusterHistograms and the device
// scratch every job needs, for the two callers that launch them: BuildHqMetaBlocks (encoder.cpp) and the introspection entries
// (hq_entry.inc).  `mm` is a DevMem.
#ifndef BROTLI_MI355X_METABLOCK_HQ_JOBS_H_
#define BROTLI_MI355X_METABLOCK_HQ_JOBS_H_

#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_api.h"
#include "metablock_api.h"
#include "metablock_device.h"
#include "metablock_hq.h"

namespace brotli_mi355x {

// BrotliSplitBlock, block_splitter.rs:840-929: the constants of the three kinds (literals, commands, distance prefixes)
static const uint32_t kHqSymbolsPerHistogram[3] = {544, 530, 544}, kHqMaxHistograms[3] = {100, 50, 50}, kHqStride[3] = {70, 40, 40};
static const float kHqSwitchCost[3] = {28.1f, 13.5f, 14.6f};

// the job of (m, kind) over `length` symbols: its parameters and, from 128 symbols on, the scratch of phase 1 (FindBlocks)
inline HqSplitJob HqMakeSplitJob(DevMem& mm, uint32_t m, uint32_t kind, uint32_t length, int quality, const uint16_t* data, uint8_t* block_ids) {
  HqSplitJob j;
  memset(&j, 0, sizeof(j));
  j.m = m;
  j.kind = kind;
  j.length = length;
  j.alphabet = kRowLen[kind];
  j.num_histograms = std::min(j.length / kHqSymbolsPerHistogram[kind] + 1, kHqMaxHistograms[kind]);
  j.stride = kHqStride[kind];
  j.iters = quality <= 11 ? 3 : 10;  // block_splitter.rs:794
  j.block_switch_cost = kHqSwitchCost[kind];
  j.data = data;
  j.block_ids = block_ids;
  if (j.length >= 128) {
    const size_t nh = j.num_histograms, bitmaplen = (nh + 7) >> 3;
    j.histo_data = mm.alloc<uint32_t>((nh + 1) * j.alphabet);
    j.histo_total = mm.alloc<uint32_t>(nh + 1);
    j.insert_cost = mm.alloc<float>((size_t)j.alphabet * nh + nh + 8);
    j.cost = mm.alloc<float>(bitmaplen * 8 + 8);
    j.switch_signal = mm.alloc<uint8_t>((size_t)j.length * bitmaplen + 8);
    j.new_id = mm.alloc<uint16_t>(nh + 8);
  }
  return j;
}

// ClusterBlocks keeps one histogram per block FindBlocks found, twice (the batches' rows and the gathered clusters);
// a pathological input (a switch every few symbols over a 16 MiB meta-block) would ask for more than the device
// has.  Refuse with a message instead of dying in an allocation half-way through.
inline void HqCheckClusterRoom(const std::vector<HqSplitJob>& jobs) {
  uint64_t need = 0;
  for (const HqSplitJob& j : jobs)
    if (j.length >= 128) need += (uint64_t)(j.num_blocks + 2) * (2ull * j.alphabet * 4 + 64ull * sizeof(HqPair) + 64);
  if (need > (96ull << 30))
    throw std::runtime_error("brotli_mi355x: quality 9.5: clustering " + std::to_string(need >> 30) +
                             " GiB of block histograms is more than this build sets aside; feed the stream in smaller pieces");
}

// the scratch of phase 2 (ClusterBlocks), sized by the j.num_blocks that FindBlocks left
inline void HqAllocClusterBlocks(DevMem& mm, HqSplitJob& j) {
  if (j.length < 128) return;
  const size_t n = j.num_blocks;
  uint64_t max_pairs = std::min<uint64_t>(64ull * n, (uint64_t)(n / 2) * n);
  max_pairs = std::max<uint64_t>(max_pairs, kHqBatchPairs);
  j.histogram_symbols = mm.alloc<uint32_t>(n + 8);
  j.block_lengths = mm.alloc<uint32_t>(n + 8);
  j.block_pos = mm.alloc<uint32_t>(n + 8);
  j.batch_data = mm.alloc<uint32_t>((n + 2) * j.alphabet);
  j.batch_total = mm.alloc<uint32_t>(n + 8);
  j.batch_cost = mm.alloc<float>(n + 8);
  j.batch_sizes = mm.alloc<uint32_t>(n + 8);
  j.batch_clusters = mm.alloc<uint32_t>(n + 8);
  j.batch_symbols = mm.alloc<uint32_t>(n + 8);
  j.batch_count = mm.alloc<uint32_t>(n / kHqBatch + 8);
  j.all_data = mm.alloc<uint32_t>((n + 2) * j.alphabet);
  j.all_total = mm.alloc<uint32_t>(n + 2);
  j.all_cost = mm.alloc<float>(n + 2);
  j.cluster_size = mm.alloc<uint32_t>(n + 8);
  j.clusters = mm.alloc<uint32_t>(n + 2 * kHqBatch + 8);  // (also the per-batch sizes / cluster lists)
  j.new_index = mm.alloc<uint32_t>(n + 2 * kHqBatch + 8);
  j.pairs = mm.alloc<HqPair>(max_pairs + 2);
}

// the batches of 64 blocks of every job that is searched at all
inline std::vector<HqBatchRef> HqSplitBatches(const std::vector<HqSplitJob>& jobs) {
  std::vector<HqBatchRef> refs;
  for (uint32_t ji = 0; ji < jobs.size(); ++ji)
    if (jobs[ji].length >= 128)
      for (uint32_t b = 0; b * kHqBatch < jobs[ji].num_blocks; ++b) refs.push_back({ji, b});
  return refs;
}

// one context-map clustering job over `in_size` rows at in_data, with its scratch (cluster.rs:353-465)
inline HqClusterJob HqMakeClusterJob(DevMem& mm, uint32_t m, uint32_t kind, uint32_t in_size, uint32_t expand64, const uint32_t* in_data) {
  HqClusterJob j;
  memset(&j, 0, sizeof(j));
  j.m = m;
  j.kind = kind;
  j.in_size = in_size;
  j.len = kRowLen[kind];
  j.expand64 = expand64;
  j.in_data = in_data;
  const size_t n = j.in_size, re = std::min<size_t>(n, 256);
  j.in_total = mm.alloc<uint32_t>(n + 8);
  j.out_data = mm.alloc<uint32_t>((n + 2) * j.len);
  j.out_total = mm.alloc<uint32_t>(n + 2);
  j.out_cost = mm.alloc<float>(n + 2);
  j.cluster_size = mm.alloc<uint32_t>(n + 8);
  j.clusters = mm.alloc<uint32_t>(n + 8);
  j.symbols = mm.alloc<uint32_t>(n + 8);
  j.new_index = mm.alloc<uint32_t>(n + 8);
  j.batch_count = mm.alloc<uint32_t>(n / kHqBatch + 8);
  j.reindex_data = mm.alloc<uint32_t>(re * j.len + 8);
  j.reindex_total = mm.alloc<uint32_t>(re + 8);
  j.reindex_cost = mm.alloc<float>(re + 8);
  j.pairs = mm.alloc<HqPair>(std::max<size_t>(kHqBatchPairs, 64 * n) + 2);
  return j;
}

inline std::vector<HqBatchRef> HqClusterBatches(const std::vector<HqClusterJob>& jobs) {
  std::vector<HqBatchRef> refs;
  for (uint32_t ji = 0; ji < jobs.size(); ++ji)
    for (uint32_t b = 0; b * kHqBatch < jobs[ji].in_size; ++b) refs.push_back({ji, b});
  return refs;
}

}  // namespace brotli_mi355x
#endif
