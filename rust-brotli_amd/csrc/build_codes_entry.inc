// build_codes_entry.inc -- introspection entry point: hands histogram rows straight to the prefix-code builder (mb_build_codes:
// k_build_codes in the product library, the scalar loop in the emulation build) and returns what it made of them.  Whole streams
// cannot steer this stage -- LZ77 and the block splitter shape every histogram first -- so the parity tests of the builder
// (tests/test_build_codes.py) come in here.  Not part of the public header.
#include <string.h>

#include <exception>
#include <vector>

#include "device_api.h"
#include "metablock_api.h"
#include "metablock_device.h"
#include "metablock_items.h"

using namespace brotli_mi355x;

extern "C" {

// histograms: n_rows rows of kRowLen[kind] (256 / 704 / 544) counts, in and out (kCodeOptimized rewrites them); depth / bits: rows of
// the same length; tree_words: n_rows x kTreeBitsWords; tree_nbits: n_rows.  Returns 0, -1 for arguments it refuses (nothing is
// launched), -2 when the device layer threw.
int brotli_mi355x_debug_build_codes(uint32_t kind, uint32_t num_distance_symbols, uint32_t mode, uint32_t n_rows, uint32_t* histograms,
                                    uint8_t* depth, uint16_t* bits, uint64_t* tree_words, uint32_t* tree_nbits) {
  constexpr uint32_t kMaxRows = 1u << 16;
  constexpr uint32_t kMaxDistanceSymbols = 16 + 120 + (62u << 4);  // the large-window alphabet at NPOSTFIX 3, NDIRECT 120
  if (kind >= 3 || (mode != kCodeOptimized && mode != kCodePlain)) return -1;
  if (num_distance_symbols < 16 || num_distance_symbols > kMaxDistanceSymbols) return -1;
  if (n_rows == 0 || n_rows > kMaxRows) return -1;
  if (!histograms || !depth || !bits || !tree_words || !tree_nbits) return -1;
  try {
    const size_t row = kRowLen[kind];
    const size_t cells = (size_t)n_rows * row;
    DevBlocks tmp;
    MbBuffers B{};
    B.histo[kind] = tmp.zeroed<uint32_t>(cells * sizeof(uint32_t));
    B.depth[kind] = tmp.zeroed<uint8_t>(cells);
    B.bits[kind] = tmp.zeroed<uint16_t>(cells * sizeof(uint16_t));
    B.tree_bits[kind] = tmp.zeroed<uint64_t>(((size_t)n_rows * kTreeBitsWords + 8) * sizeof(uint64_t));
    B.tree_nbits[kind] = tmp.zeroed<uint32_t>(((size_t)n_rows + 8) * sizeof(uint32_t));
    B.huff_scratch = tmp.zeroed<HuffmanScratch>(sizeof(HuffmanScratch));
    CodeJob* jobs_dev = tmp.zeroed<CodeJob>((size_t)n_rows * sizeof(CodeJob));
    std::vector<CodeJob> jobs(n_rows);
    for (uint32_t i = 0; i < n_rows; ++i) jobs[i] = CodeJob{kind, i, num_distance_symbols, mode};
    dev_h2d(jobs_dev, jobs.data(), (size_t)n_rows * sizeof(CodeJob));
    dev_h2d(B.histo[kind], histograms, cells * sizeof(uint32_t));
    mb_build_codes(B, jobs_dev, n_rows);
    dev_d2h(histograms, B.histo[kind], cells * sizeof(uint32_t));
    dev_d2h(depth, B.depth[kind], cells);
    dev_d2h(bits, B.bits[kind], cells * sizeof(uint16_t));
    dev_d2h(tree_words, B.tree_bits[kind], (size_t)n_rows * kTreeBitsWords * sizeof(uint64_t));
    dev_d2h(tree_nbits, B.tree_nbits[kind], (size_t)n_rows * sizeof(uint32_t));
    tmp.clear();
    return 0;
  } catch (const std::exception&) {
    return -2;
  }
}
}
