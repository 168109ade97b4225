// hq_entry.inc -- introspection entry points of the quality >= 10 meta-block builder (metablock_hq.h): symbol vectors straight to
// FindBlocks + ClusterBlocks, histogram rows straight to BrotliClusterHistograms (k_hq_* in the product library, the scalar twins
// in the emulation build).  Whole streams cannot steer these stages -- LZ77 decides which symbols exist, and the sizes at which the
// device form changes shape (65 entropy codes, 65 / 129 / 257 clusters, a full pair queue) are not ones natural inputs are known
// to reach -- so the parity tests of the builder (tests/test_hq_builder.py) come in here.  Every job is a meta-block of its own
// (one MbDesc / MbResult row), so hundreds run side by side in one launch, with the job tables and the scratch BuildHqMetaBlocks
// uses (metablock_hq_jobs.h).  Not part of the public header.
#include <string.h>

#include <exception>
#include <vector>

#include "device_api.h"
#include "metablock_api.h"
#include "metablock_device.h"
#include "metablock_hq.h"
#include "metablock_hq_jobs.h"
#include "metablock_items.h"

using namespace brotli_mi355x;

namespace {
constexpr uint32_t kHqEntryMaxJobs = 4096;
MbBuffers HqEntryBuffers(DevMem& mm, uint32_t n_jobs) {
  MbBuffers B{};
  const DeviceTables& dt = dev_tables();
  B.et.logs_16 = dt.logs_16;
  B.et.logs_8 = dt.logs_8;
  B.n_mb = n_jobs;
  B.descs = mm.alloc<MbDesc>(n_jobs);
  B.results = mm.alloc<MbResult>(n_jobs);
  return B;
}
}  // namespace

extern "C" {

// BrotliSplitBlock's SplitByteVector of n_jobs symbol vectors of one kind (0 literals, 1 commands, 2 distance prefixes), at the
// quality 10 / 11 setting (three FindBlocks iterations).  lengths: n_jobs; symbols: the vectors one behind the other.  Out, per job:
// phase1_blocks and, at the job's symbol offset, phase1_ids -- what mb_hq_find_blocks left (0 blocks: no symbols; under 128 symbols
// one block of id 0 and no search); num_types, num_blocks and, at the job's symbol offset, types / block_lengths (num_blocks entries
// each) -- the split behind mb_hq_cluster_blocks.  Returns 0, -1 for arguments it refuses (nothing is launched), -2 when the device
// layer threw.
int brotli_mi355x_debug_hq_split(uint32_t kind, uint32_t n_jobs, const uint32_t* lengths, const uint16_t* symbols, uint32_t* phase1_blocks,
                                 uint8_t* phase1_ids, uint32_t* num_types, uint32_t* num_blocks, uint8_t* types, uint32_t* block_lengths) {
  constexpr uint32_t kMaxLength = 1u << 20;
  constexpr uint64_t kMaxTotal = 1ull << 24;
  if (kind >= 3 || n_jobs == 0 || n_jobs > kHqEntryMaxJobs) return -1;
  if (!lengths || !phase1_blocks || !num_types || !num_blocks) return -1;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (lengths[i] > kMaxLength) return -1;
    total += lengths[i];
  }
  if (total > kMaxTotal) return -1;
  if (total != 0 && (!symbols || !phase1_ids || !types || !block_lengths)) return -1;
  for (uint64_t i = 0; i < total; ++i)
    if (symbols[i] >= kRowLen[kind]) return -1;
  try {
    DevMem mm;
    MbBuffers B = HqEntryBuffers(mm, n_jobs);
    uint16_t* sym_dev = mm.alloc<uint16_t>(total + 8);
    uint8_t* ids_dev = mm.alloc<uint8_t>(total + 8);
    if (total) dev_h2d(sym_dev, symbols, total * sizeof(uint16_t));
    std::vector<HqSplitJob> jobs;
    std::vector<uint64_t> offset(n_jobs);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
      offset[i] = at;
      jobs.push_back(HqMakeSplitJob(mm, i, kind, lengths[i], 11, sym_dev + at, ids_dev + at));
      at += lengths[i];
    }
    HqSplitJob* jobs_dev = mm.alloc<HqSplitJob>(n_jobs + 1);
    dev_h2d(jobs_dev, jobs.data(), n_jobs * sizeof(HqSplitJob));
    mb_hq_find_blocks(B, jobs_dev, n_jobs);
    dev_d2h(jobs.data(), jobs_dev, n_jobs * sizeof(HqSplitJob));
    if (total) dev_d2h(phase1_ids, ids_dev, total);
    for (uint32_t i = 0; i < n_jobs; ++i) phase1_blocks[i] = jobs[i].num_blocks;
    HqCheckClusterRoom(jobs);
    std::vector<MbDesc> descs(n_jobs);
    memset(descs.data(), 0, n_jobs * sizeof(MbDesc));
    uint32_t block_total = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
      descs[i].block_base[kind] = block_total;
      descs[i].max_blocks[kind] = jobs[i].num_blocks + 1;
      block_total += jobs[i].num_blocks + 2;
      HqAllocClusterBlocks(mm, jobs[i]);
    }
    B.block_types[kind] = mm.alloc<uint8_t>(block_total + 8);
    B.block_lengths[kind] = mm.alloc<uint32_t>(block_total + 8);
    B.block_start[kind] = mm.alloc<uint32_t>(block_total + 8);
    dev_h2d(B.descs, descs.data(), n_jobs * sizeof(MbDesc));
    dev_h2d(jobs_dev, jobs.data(), n_jobs * sizeof(HqSplitJob));
    const std::vector<HqBatchRef> refs = HqSplitBatches(jobs);
    HqBatchRef* refs_dev = mm.alloc<HqBatchRef>(refs.size() + 1);
    dev_h2d(refs_dev, refs.data(), refs.size() * sizeof(HqBatchRef));
    mb_hq_cluster_blocks(B, jobs_dev, n_jobs, refs_dev, (uint32_t)refs.size());
    std::vector<MbResult> results(n_jobs);
    std::vector<uint8_t> all_types(block_total + 8);
    std::vector<uint32_t> all_lengths(block_total + 8);
    dev_d2h(results.data(), B.results, n_jobs * sizeof(MbResult));
    dev_d2h(all_types.data(), B.block_types[kind], block_total);
    dev_d2h(all_lengths.data(), B.block_lengths[kind], block_total * sizeof(uint32_t));
    for (uint32_t i = 0; i < n_jobs; ++i) {
      num_types[i] = results[i].num_types[kind];
      num_blocks[i] = results[i].num_blocks[kind];
      if (num_blocks[i] > jobs[i].num_blocks) return -2;  // (more blocks than phase 1 left: no room was set aside for them)
      for (uint32_t b = 0; b < num_blocks[i]; ++b) {
        types[offset[i] + b] = all_types[descs[i].block_base[kind] + b];
        block_lengths[offset[i] + b] = all_lengths[descs[i].block_base[kind] + b];
      }
    }
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}

// BrotliClusterHistograms (max_histograms 256, as BrotliBuildMetaBlock calls it) of n_jobs sets of histogram rows: kind 0 (literal
// contexts, rows of 256) or 2 (distance contexts, rows of 544).  in_sizes: n_jobs, each 1..16384; rows: the sets one behind the
// other; expand64: per job, the map is spread over 64 contexts per input (literal jobs only).  Out, per job: out_count; at the job's
// row offset out_rows / out_total / out_cost (out_count entries: the clustered histograms, their totals and the bit patterns of their
// cached costs) and slot_cost (in_size entries: the bit pattern of the cached cost of every slot of the working set behind
// BrotliHistogramRemap -- HistogramClear's 3.402e+38 where a cluster survived, elsewhere what the slot cost when it was merged
// away, so the BrotliPopulationCost of an input that never led a cluster); map: the context maps one behind the other (in_size
// entries, or 64 x in_size with expand64).  Return values as above.
int brotli_mi355x_debug_hq_cluster(uint32_t kind, uint32_t n_jobs, const uint32_t* in_sizes, const uint32_t* rows, const uint32_t* expand64,
                                   uint32_t* out_count, uint32_t* out_rows, uint32_t* out_total, uint32_t* out_cost, uint32_t* slot_cost,
                                   uint32_t* map) {
  constexpr uint32_t kMaxInSize = 16384;
  constexpr uint64_t kMaxTotalRows = 1ull << 16;
  if ((kind != kSplitLiteral && kind != kSplitDistance) || n_jobs == 0 || n_jobs > kHqEntryMaxJobs) return -1;
  if (!in_sizes || !rows || !expand64 || !out_count || !out_rows || !out_total || !out_cost || !slot_cost || !map) return -1;
  uint64_t total_rows = 0;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    if (in_sizes[i] == 0 || in_sizes[i] > kMaxInSize || expand64[i] > 1 || (expand64[i] && kind != kSplitLiteral)) return -1;
    total_rows += in_sizes[i];
  }
  if (total_rows > kMaxTotalRows) return -1;
  try {
    const uint32_t len = kRowLen[kind], which = kind == kSplitLiteral ? 0u : 1u;
    DevMem mm;
    MbBuffers B = HqEntryBuffers(mm, n_jobs);
    uint32_t* rows_dev = mm.alloc<uint32_t>(total_rows * len + 8);
    dev_h2d(rows_dev, rows, total_rows * len * sizeof(uint32_t));
    std::vector<MbDesc> descs(n_jobs);
    memset(descs.data(), 0, n_jobs * sizeof(MbDesc));
    std::vector<HqClusterJob> jobs;
    std::vector<uint64_t> row_base(n_jobs), map_base(n_jobs);
    uint64_t row_at = 0, map_at = 0, histo_at = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
      row_base[i] = row_at;
      map_base[i] = map_at;
      descs[i].histo_base[kind] = (uint32_t)histo_at;
      descs[i].max_histos[kind] = 256;
      descs[i].hq_ctx_map_base[which] = (uint32_t)map_at;
      jobs.push_back(HqMakeClusterJob(mm, i, kind, in_sizes[i], expand64[i], rows_dev + row_at * len));
      row_at += in_sizes[i];
      map_at += (uint64_t)in_sizes[i] * (expand64[i] ? 64 : 1);
      histo_at += in_sizes[i] < 256 ? in_sizes[i] : 256;
    }
    B.histo[kind] = mm.alloc<uint32_t>(histo_at * len + 8);
    B.hq_ctx_map[which] = mm.alloc<uint32_t>(map_at + 8);
    dev_h2d(B.descs, descs.data(), n_jobs * sizeof(MbDesc));
    HqClusterJob* jobs_dev = mm.alloc<HqClusterJob>(n_jobs + 1);
    dev_h2d(jobs_dev, jobs.data(), n_jobs * sizeof(HqClusterJob));
    const std::vector<HqBatchRef> refs = HqClusterBatches(jobs);
    HqBatchRef* refs_dev = mm.alloc<HqBatchRef>(refs.size() + 1);
    dev_h2d(refs_dev, refs.data(), refs.size() * sizeof(HqBatchRef));
    mb_hq_cluster_histograms(B, jobs_dev, n_jobs, refs_dev, (uint32_t)refs.size());
    std::vector<MbResult> results(n_jobs);
    dev_d2h(results.data(), B.results, n_jobs * sizeof(MbResult));
    dev_d2h(map, B.hq_ctx_map[which], map_at * sizeof(uint32_t));
    for (uint32_t i = 0; i < n_jobs; ++i) {
      const uint32_t n = results[i].num_histos[kind];
      out_count[i] = n;
      if (n > in_sizes[i] || n > 256) return -2;  // (more histograms than there is room for)
      dev_d2h(out_rows + row_base[i] * len, B.histo[kind] + (size_t)descs[i].histo_base[kind] * len, (size_t)n * len * sizeof(uint32_t));
      dev_d2h(out_total + row_base[i], jobs[i].reindex_total, n * sizeof(uint32_t));
      dev_d2h(out_cost + row_base[i], jobs[i].reindex_cost, n * sizeof(float));
      dev_d2h(slot_cost + row_base[i], jobs[i].out_cost, in_sizes[i] * sizeof(float));
    }
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}
}
