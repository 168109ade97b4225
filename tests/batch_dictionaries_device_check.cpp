// batch_dictionaries_device_check.cpp -- a stand-alone host program over the emulation build (device memory is host memory there)
// for what the Python tests of BrotliMi355xCompressBatchWithDictionariesDevice cannot see: every dictionary, every item and every
// output lies in a heap block of exactly its size, so under a sanitizer any read in front of or behind a dictionary or an item and
// any write outside [0, capacity) is an error.  A truncated dictionary is given as the address its first byte WOULD have: only its
// last (1 << lgwin) - 16 bytes are allocated, and the library must not touch the front.  All four side-by-side routes, one item
// that runs one by one, and the rule of the call's delivery.  Prints "layouts ok".
//
// Against the emulation library:   g++ -std=c++17 -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc tests/batch_dictionaries_device_check.cpp
//                                      tests/emu/libbrotli_emu.so -Wl,-rpath,$PWD/tests/emu -o batch_dictionaries_device_check
// Under a sanitizer the emulation sources are compiled into the program itself (the list is OBJS_SRC of tests/emu/Makefile):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc
//       tests/batch_dictionaries_device_check.cpp <OBJS_SRC> -o batch_dictionaries_device_check_asan
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

std::vector<uint8_t> Text(size_t n) {
  static const char* words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "lazy ", "dog. ", "Alice ", "was ", "beginning ", "to "};
  std::vector<uint8_t> v;
  while (v.size() < n) {
    const char* w = words[Next() % 12];
    v.insert(v.end(), w, w + strlen(w));
  }
  v.resize(n);
  return v;
}

int Fail(const char* what, size_t i) {
  printf("FAILED: %s (item %zu)\n", what, i);
  return 1;
}

// a heap block of exactly the bytes given (one byte for none: never read)
uint8_t* Block(const uint8_t* bytes, size_t n) {
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, bytes, n);
  return p;
}

// Item i behind dictionary named[i], every buffer a heap block of exactly its size; the host call on the same bytes is the
// reference.  A dictionary longer than the window's (1 << lgwin) - 16 is allocated from its first byte in use on.
// side: the items expected side by side.
int Layout(const std::vector<std::vector<uint8_t>>& dictionaries, const std::vector<std::vector<uint8_t>>& items, const std::vector<size_t>& named, int quality,
           int lgwin, uint32_t routes, size_t side) {
  const size_t n = items.size(), nd = dictionaries.size();
  std::vector<const uint8_t*> host_dicts(nd), host_in(n);
  std::vector<size_t> dict_sizes(nd), in_sizes(n), want_sizes(n);
  std::vector<std::vector<uint8_t>> want(n);
  std::vector<uint8_t*> want_out(n);
  for (size_t k = 0; k < nd; ++k) {
    host_dicts[k] = dictionaries[k].data();
    dict_sizes[k] = dictionaries[k].size();
  }
  for (size_t i = 0; i < n; ++i) {
    host_in[i] = items[i].data();
    in_sizes[i] = items[i].size();
    want[i].resize(BrotliEncoderMaxCompressedSize(items[i].size()) + 1024);
    want_out[i] = want[i].data();
    want_sizes[i] = want[i].size();
  }
  if (!BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, BROTLI_MODE_GENERIC, routes, nd, host_dicts.data(), dict_sizes.data(), n, named.data(),
                                                 host_in.data(), in_sizes.data(), want_out.data(), want_sizes.data(), nullptr))
    return Fail("the host call", 0);
  uint64_t host_info[8], info[8];
  BrotliMi355xLastBatchInfo(host_info);

  const size_t window = ((size_t)1 << lgwin) - 16;
  std::vector<uint8_t*> dict_blocks(nd), in(n), out(n);
  std::vector<const uint8_t*> dicts(nd);
  std::vector<size_t> out_sizes(n);
  for (size_t k = 0; k < nd; ++k) {
    const size_t use = dict_sizes[k] > window ? window : dict_sizes[k];
    dict_blocks[k] = Block(dictionaries[k].data() + (dict_sizes[k] - use), use);
    dicts[k] = (const uint8_t*)((uintptr_t)dict_blocks[k] - (dict_sizes[k] - use));  // (the unused front is not there)
  }
  for (size_t i = 0; i < n; ++i) {
    in[i] = Block(items[i].data(), items[i].size());
    out[i] = (uint8_t*)malloc(want_sizes[i] ? want_sizes[i] : 1);
    out_sizes[i] = want_sizes[i];
  }
  std::vector<int32_t> results(n);
  const int32_t ok = BrotliMi355xCompressBatchWithDictionariesDevice(quality, lgwin, BROTLI_MODE_GENERIC, routes, nd, dicts.data(), dict_sizes.data(), n,
                                                                     named.data(), in.data(), in_sizes.data(), out.data(), out_sizes.data(), results.data());
  BrotliMi355xLastBatchInfo(info);
  int bad = 0;
  if (!ok) bad = Fail(BrotliMi355xLastError(), 0);
  if (memcmp(info, host_info, sizeof(info)) != 0) bad = Fail("info differs from the host call's", 0);
  if (info[1] != side) bad = Fail("items side by side", (size_t)info[1]);
  for (size_t i = 0; i < n && !bad; ++i)
    if (!results[i] || out_sizes[i] != want_sizes[i] || memcmp(out[i], want[i].data(), want_sizes[i]) != 0) bad = Fail("stream differs from the host call's", i);
  for (size_t k = 0; k < nd; ++k) free(dict_blocks[k]);
  for (size_t i = 0; i < n; ++i) {
    free(in[i]);
    free(out[i]);
  }
  return bad;
}

int Layouts() {
  // the stream rule beside BrotliEncoderCompress's: no stored stream to fall back to, no BrotliEncoderMaxCompressedSize to hold against
  const size_t max_size = BrotliEncoderMaxCompressedSize(2000);
  if (DeliveryRule(max_size + 1, 2000, max_size) != Delivery::kStored || StreamDeliveryRule(max_size + 1, 2000, max_size) != Delivery::kFails)
    return Fail("rule: one byte short, room for the stored stream", 0);
  if (StreamDeliveryRule(max_size + 1, 2000, max_size + 1) != Delivery::kStream) return Fail("rule: a stream above the one-shot bound that fits", 0);
  if (StreamDeliveryRule(0, 0, 0) != Delivery::kStream || StreamDeliveryRule(1, 0, 0) != Delivery::kFails) return Fail("rule: no room", 0);

  static const size_t dictionary_sizes[] = {2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 4097, 65536};
  static const size_t item_sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4097};
  std::vector<std::vector<uint8_t>> dictionaries, items;
  std::vector<size_t> each, one;
  for (size_t bytes : dictionary_sizes) dictionaries.push_back(Text(bytes));
  for (size_t bytes : item_sizes) {
    each.push_back(items.size() % dictionaries.size());
    one.push_back(16);  // the 4097-byte dictionary, cut at lgwin 10
    items.push_back(Text(bytes));
  }
  const size_t n = items.size();
  // a dictionary per item: qualities 5 .. 8, and 2 .. 4 with the bit (at lgwin 10 the dictionaries of 4097 and 65 536 bytes are cut)
  if (Layout(dictionaries, items, each, 5, 22, 0, n) || Layout(dictionaries, items, each, 8, 17, 0, n)) return 1;
  if (Layout(dictionaries, items, each, 2, 22, BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, n)) return 1;
  if (Layout(dictionaries, items, each, 4, 10, BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, n)) return 1;
  // one index named by every item: the shared image of either kind
  if (Layout(dictionaries, items, one, 5, 22, 0, n) || Layout(dictionaries, items, one, 4, 10, BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, n)) return 1;
  // one by one beside side-by-side items: the empty item, an item of two input blocks, and a dictionary of one byte
  std::vector<std::vector<uint8_t>> mixed = {Text(3000), {}, Text(70000), Text(500)};
  std::vector<std::vector<uint8_t>> mixed_dictionaries = {Text(1000), Text(1)};
  if (Layout(mixed_dictionaries, mixed, {0, 0, 0, 1}, 5, 22, 0, 1)) return 1;
  // ... and at a window that cuts the dictionary of an item that runs one by one (quality 2 without the bit)
  if (Layout(dictionaries, {Text(300), Text(40)}, {17, 16}, 2, 10, 0, 0)) return 1;
  printf("layouts ok\n");
  return 0;
}

}  // namespace

int main() { return Layouts(); }
