// batch_device_check.cpp -- a stand-alone host program over the emulation build (device memory is host memory there) for what the
// Python tests of BrotliMi355xCompressBatchDevice cannot see.
//
//   batch_device_check layouts     the layouts of tests/test_batch_device.py (items of 1 .. 300 bytes, and five of two input blocks)
//                                  with every item and every output in a heap block of exactly its size: under a sanitizer any read
//                                  behind an item or write outside [0, capacity) is an error.
//   batch_device_check stored N    the stored-stream fallback, which no small input reaches through the encoder (a seeded search of
//                                  10 000 items of at most 4 KiB at qualities 0 .. 11 found none): the delivery rule is called directly
//                                  for streams that exceed BrotliEncoderMaxCompressedSize, and the stored stream of N seeded bytes is
//                                  produced in a heap block of exactly its size and printed in hex.
//
// Against the emulation library:   g++ -std=c++17 -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc tests/batch_device_check.cpp
//                                      tests/emu/libbrotli_emu.so -Wl,-rpath,$PWD/tests/emu -o batch_device_check
// Under a sanitizer the emulation sources are compiled into the program itself (the list is OBJS_SRC of tests/emu/Makefile):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc tests/batch_device_check.cpp
//       <OBJS_SRC> -o batch_device_check_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/brotli_mi355x.h"
#include "batch_greedy.h"

using namespace brotli_mi355x;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t Next() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}

std::vector<uint8_t> Item(size_t n, int kind) {
  static const char* words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "lazy ", "dog. ", "Alice ", "was ", "beginning ", "to "};
  std::vector<uint8_t> v;
  while (v.size() < n) {
    if (kind == 0) {
      const char* w = words[Next() % 12];
      v.insert(v.end(), w, w + strlen(w));
    } else {
      v.push_back(kind == 1 ? (uint8_t)Next() : 0);
    }
  }
  v.resize(n);
  return v;
}

int Fail(const char* what, size_t i) {
  printf("FAILED: %s (item %zu)\n", what, i);
  return 1;
}

// every item and every output a heap block of exactly its size
int Layout(const std::vector<std::vector<uint8_t>>& items, int quality, uint32_t routes) {
  const size_t n = items.size();
  std::vector<std::vector<uint8_t>> want(n);
  std::vector<uint8_t*> in(n), out(n);
  std::vector<size_t> in_sizes(n), out_sizes(n);
  for (size_t i = 0; i < n; ++i) {
    want[i].resize(BrotliEncoderMaxCompressedSize(items[i].size()) + 16);
    size_t size = want[i].size();
    if (!BrotliEncoderCompress(quality, 22, BROTLI_MODE_GENERIC, items[i].size(), items[i].data(), &size, want[i].data())) return Fail("one-shot", i);
    want[i].resize(size);
    in[i] = (uint8_t*)malloc(items[i].size());
    memcpy(in[i], items[i].data(), items[i].size());
    in_sizes[i] = items[i].size();
    out[i] = (uint8_t*)malloc(size);
    out_sizes[i] = size;
  }
  std::vector<int32_t> results(n);
  const int32_t ok = BrotliMi355xCompressBatchDevice(quality, 22, BROTLI_MODE_GENERIC, routes, n, in.data(), in_sizes.data(), out.data(), out_sizes.data(),
                                                     results.data());
  uint64_t info[8];
  BrotliMi355xLastBatchInfo(info);
  int bad = 0;
  if (!ok) bad = Fail("the call", 0);
  if (info[1] != n) bad = Fail("not every item went side by side", (size_t)info[1]);
  for (size_t i = 0; i < n && !bad; ++i)
    if (!results[i] || out_sizes[i] != want[i].size() || memcmp(out[i], want[i].data(), want[i].size()) != 0) bad = Fail("stream differs from the one-shot call's", i);
  for (size_t i = 0; i < n; ++i) {
    free(in[i]);
    free(out[i]);
  }
  return bad;
}

int Layouts() {
  std::vector<std::vector<uint8_t>> small, longer;
  for (int i = 0; i < 200; ++i) small.push_back(Item(1 + Next() % 300, (int)(Next() % 3)));
  for (size_t bytes : {65537, 66001, 67890, 69999, 70001}) longer.push_back(Item(bytes, 0));
  if (Layout(small, 5, 0) || Layout(small, 2, BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS) || Layout(longer, 5, BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS)) return 1;
  printf("layouts ok\n");
  return 0;
}

int Stored(size_t n) {
  const size_t max_size = BrotliEncoderMaxCompressedSize(n);
  // a stream above BrotliEncoderMaxCompressedSize never goes out; the stored stream does where the buffer holds that many bytes
  if (DeliveryRule(max_size + 1, n, max_size + 100) != Delivery::kStored) return Fail("rule: roomy buffer", 0);
  if (DeliveryRule(max_size + 1, n, max_size) != Delivery::kStored) return Fail("rule: exact buffer", 0);
  if (DeliveryRule(max_size + 1, n, max_size - 1) != Delivery::kFails) return Fail("rule: one byte short", 0);
  if (DeliveryRule(max_size, n, max_size) != Delivery::kStream) return Fail("rule: the stream fits", 0);
  if (DeliveryRule(max_size, n, max_size - 1) != Delivery::kFails) return Fail("rule: the stream does not fit, nor would the stored one", 0);
  if (DeliveryRule(10, n, 9) != (max_size <= 9 ? Delivery::kStored : Delivery::kFails)) return Fail("rule: small buffer", 0);
  std::vector<uint8_t> item = Item(n, 1);
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  memcpy(in, item.data(), n);
  // (the size first, into a roomy block; then again into a block of exactly that size)
  std::vector<uint8_t> roomy(max_size + 64);
  const size_t size = StoredStreamToDevice(in, n, roomy.data());
  if (size > max_size) return Fail("the stored stream exceeds BrotliEncoderMaxCompressedSize", 0);
  uint8_t* out = (uint8_t*)malloc(size);
  if (StoredStreamToDevice(in, n, out) != size || memcmp(out, roomy.data(), size) != 0) return Fail("stored stream", 0);
  printf("stored %zu ", size);
  for (size_t i = 0; i < size; ++i) printf("%02x", out[i]);
  printf("\n");
  free(in);
  free(out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "layouts")) return Layouts();
  if (argc >= 3 && !strcmp(argv[1], "stored")) return Stored((size_t)strtoull(argv[2], nullptr, 10));
  printf("usage: batch_device_check layouts | stored N\n");
  return 2;
}
