// zopfli_parts_check.cpp -- a stand-alone host program over the emulation build (device memory is host memory there) for what the
// Python tests of the introspection entries of zopfli_entry.inc cannot see: that the entries, and the functions of zopfli_device.h
// behind them, read nothing beyond what they were given.
//
//   zopfli_parts_check FILE        FILE: the constructed queries of tests/test_zopfli_parts.py (family A), written by
//                                  `python tests/test_zopfli_parts.py FILE`.
//     * the text and the query arrays go through brotli_mi355x_debug_dictionary_matches from heap blocks of exactly their sizes;
//     * the same queries go straight to the seam (zopfli_debug_dictionary_matches) with the text in a heap block of exactly
//       n_text + 64 bytes -- the text and the padding the entry adds, as the product's text buffer has it: the search itself reads
//       nothing behind that -- and must give the same answers; the last byte of the text, asked on its own, with exactly the three
//       bytes behind it that the four-byte load at the place takes;
//     * blocks of 1, 495, 2000 and 4001 bytes, of two kinds (mostly UTF-8 and not), go through brotli_mi355x_debug_literal_costs from
//       exactly sized blocks, and straight to the seam (zopfli_debug_literal_costs) with NO padding behind the data, 3 * 256 words
//       of histogram, `len` costs and `len + 2` prefix sums;
//     * three histogram rows and a few values go through the other two entries the same way.
//   Under a sanitizer any read or write outside those blocks is an error.
//
// Against the emulation library:   g++ -std=c++17 -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc tests/zopfli_parts_check.cpp
//                                      tests/emu/libbrotli_emu.so -Wl,-rpath,$PWD/tests/emu -o zopfli_parts_check
// Under a sanitizer the emulation sources are compiled into the program itself (the list is OBJS_SRC of tests/emu/Makefile):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -DBROTLI_HOST_EMU=1
//       -I rust-brotli_amd/csrc tests/zopfli_parts_check.cpp <OBJS_SRC> -o zopfli_parts_check_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zopfli_entry_api.h"

using namespace brotli_mi355x;

extern "C" {
int brotli_mi355x_debug_dictionary_matches(const uint8_t* text, uint32_t n_text, uint32_t n_queries, const uint32_t* at, const uint32_t* min_length,
                                           const uint32_t* max_length, uint32_t* out_matches, uint32_t* out_any);
int brotli_mi355x_debug_fast_log2(uint32_t mode, uint32_t n, const uint64_t* values, uint32_t* out_bits);
int brotli_mi355x_debug_literal_costs(uint32_t n_jobs, const uint32_t* lengths, const uint8_t* data, uint32_t* out_cost_bits, uint32_t* out_prefix_bits);
int brotli_mi355x_debug_cost_from_histogram(uint32_t n_jobs, const uint32_t* sizes, const uint32_t* literal, const uint32_t* histograms,
                                            uint32_t* out_cost_bits);
}

namespace {

// a heap block of exactly `count` entries (never a vector: its capacity may exceed its size)
template <typename T>
T* Exact(size_t count) {
  T* p = (T*)malloc(count * sizeof(T));
  if (!p) abort();
  return p;
}

int Fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

int Dictionary(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return Fail("cannot open the query file");
  uint32_t head[2];
  if (fread(head, 4, 2, f) != 2) return Fail("short query file");
  const uint32_t n_text = head[0], n = head[1];
  uint8_t* text = Exact<uint8_t>(n_text);
  uint32_t* at = Exact<uint32_t>(n);
  uint32_t* lo = Exact<uint32_t>(n);
  uint32_t* hi = Exact<uint32_t>(n);
  if (fread(text, 1, n_text, f) != n_text || fread(at, 4, n, f) != n || fread(lo, 4, n, f) != n || fread(hi, 4, n, f) != n) return Fail("short query file");
  fclose(f);
  uint32_t* matches = Exact<uint32_t>((size_t)n * 38);
  uint32_t* any = Exact<uint32_t>(n);
  if (brotli_mi355x_debug_dictionary_matches(text, n_text, n, at, lo, hi, matches, any) != 0) return Fail("the dictionary entry refused the queries");
  // the search itself, on the text and exactly the padding the entry adds
  uint8_t* padded = Exact<uint8_t>((size_t)n_text + 64);
  memcpy(padded, text, n_text);
  memset(padded + n_text, 0, 64);
  uint32_t* matches2 = Exact<uint32_t>((size_t)n * 38);
  uint32_t* any2 = Exact<uint32_t>(n);
  zopfli_debug_dictionary_matches(padded, n, at, lo, hi, matches2, any2);
  if (memcmp(matches, matches2, (size_t)n * 38 * 4) != 0 || memcmp(any, any2, (size_t)n * 4) != 0) return Fail("entry and seam disagree");
  // the last byte of the text asked on its own: four bytes are loaded at the place, three of them padding
  uint32_t last_at = n_text - 1, last_lo = 4, last_hi = 1, last_any = 7;
  uint32_t* last = Exact<uint32_t>(38);
  if (brotli_mi355x_debug_dictionary_matches(text, n_text, 1, &last_at, &last_lo, &last_hi, last, &last_any) != 0 || last_any != 0) return Fail("last byte");
  // ... and straight at the seam with exactly those three bytes behind the text
  uint8_t* tight = Exact<uint8_t>((size_t)n_text + 3);
  memcpy(tight, text, n_text);
  memset(tight + n_text, 0, 3);
  zopfli_debug_dictionary_matches(tight, 1, &last_at, &last_lo, &last_hi, last, &last_any);
  if (last_any != 0) return Fail("last byte, seam");
  free(tight);
  uint64_t with_match = 0, sum = 0;
  for (uint32_t q = 0; q < n; ++q) with_match += any[q];
  for (size_t i = 0; i < (size_t)n * 38; ++i) sum = sum * 1099511628211ull + matches[i];
  printf("dictionary: %u bytes of text, %u queries, %llu with a match, checksum %016llx\n", n_text, n, (unsigned long long)with_match, (unsigned long long)sum);
  free(text), free(at), free(lo), free(hi), free(matches), free(any), free(padded), free(matches2), free(any2), free(last);
  return 0;
}

int LiteralCosts() {
  const uint32_t lens[4] = {1, 495, 2000, 4001};
  for (int kind = 0; kind < 2; ++kind) {
    uint32_t* lengths = Exact<uint32_t>(4);
    size_t total = 0;
    for (int j = 0; j < 4; ++j) total += lengths[j] = lens[j];
    uint8_t* data = Exact<uint8_t>(total);
    // kind 0: words with a two-byte UTF-8 letter now and then (mostly UTF-8); kind 1: bytes of which most are lone continuation bytes
    for (size_t i = 0; i < total; ++i) data[i] = kind == 0 ? (uint8_t)"the quick brown fox \xc3\xa9t\xc3\xa9 "[i % 26] : (uint8_t)(0x80 | ((i * 37) & 0x3f));
    if (kind == 1)
      for (size_t i = 0; i < total; i += 7) data[i] = 'a' + (uint8_t)(i % 23);
    uint32_t* cost = Exact<uint32_t>(total);
    uint32_t* prefix = Exact<uint32_t>(total + 4);
    if (brotli_mi355x_debug_literal_costs(4, lengths, data, cost, prefix) != 0) return Fail("the literal-cost entry refused the blocks");
    size_t off = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      // the cost model itself, one block with nothing behind it
      const uint32_t len = lens[j];
      uint8_t* d = Exact<uint8_t>(len);
      memcpy(d, data + off, len);
      uint32_t* histo = Exact<uint32_t>(768);
      float* c = Exact<float>(len);
      float* p = Exact<float>((size_t)len + 2);
      const uint32_t one_len = len;
      const unsigned long long zero = 0;
      zopfli_debug_literal_costs(1, &one_len, &zero, d, histo, c, p);
      if (memcmp(c, cost + off, (size_t)len * 4) != 0 || memcmp(p, prefix + off + j, ((size_t)len + 1) * 4) != 0) return Fail("literal costs: entry and seam disagree");
      free(d), free(histo), free(c), free(p);
      off += len;
    }
    uint64_t sum = 0;
    for (size_t i = 0; i < total; ++i) sum = sum * 1099511628211ull + cost[i];
    for (size_t i = 0; i < total + 4; ++i) sum = sum * 1099511628211ull + prefix[i];
    printf("literal costs, kind %d: blocks of 1, 495, 2000, 4001 bytes, checksum %016llx\n", kind, (unsigned long long)sum);
    free(lengths), free(data), free(cost), free(prefix);
  }
  return 0;
}

int HistogramsAndLogs() {
  uint32_t* sizes = Exact<uint32_t>(3);
  uint32_t* literal = Exact<uint32_t>(3);
  sizes[0] = 1, sizes[1] = 64, sizes[2] = 1200;
  literal[0] = 0, literal[1] = 1, literal[2] = 0;
  uint32_t* rows = Exact<uint32_t>(1265);
  for (uint32_t i = 0; i < 1265; ++i) rows[i] = (i % 3 == 0) ? 0u : i * 2654435761u >> (i % 29);
  uint32_t* cost = Exact<uint32_t>(1265);
  if (brotli_mi355x_debug_cost_from_histogram(3, sizes, literal, rows, cost) != 0) return Fail("the histogram entry refused the rows");
  uint64_t* values = Exact<uint64_t>(5);
  values[0] = 0, values[1] = 255, values[2] = 256, values[3] = 65535, values[4] = ~0ull;
  uint32_t* bits = Exact<uint32_t>(5);
  for (uint32_t mode = 0; mode < 3; ++mode)
    if (brotli_mi355x_debug_fast_log2(mode, 5, values, bits) != 0) return Fail("the log2 entry refused the values");
  printf("histogram rows of 1, 64, 1200 counts and five logarithms: done\n");
  free(sizes), free(literal), free(rows), free(cost), free(values), free(bits);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    printf("usage: zopfli_parts_check FILE   (FILE written by `python tests/test_zopfli_parts.py FILE`)\n");
    return 2;
  }
  if (Dictionary(argv[1]) || LiteralCosts() || HistogramsAndLogs()) return 1;
  printf("OK\n");
  return 0;
}
