// batch_dictionaries_zopfli_check.cpp -- a stand-alone host program over the emulation build (device memory is host memory there)
// for what the Python tests of BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS cannot see: every dictionary, every item and every
// output lies in a heap block of exactly its size, so under a sanitizer any read in front of or behind a dictionary or an item --
// the prepend's 128-byte comparisons, the stitch, the hash loads of the last positions -- and any write outside [0, capacity) is an
// error.  A truncated dictionary is given as the address its first byte WOULD have: only its last (1 << lgwin) - 16 bytes are
// allocated, and the library must not touch the front.  Both qualities of the route through the host entry and the device entry,
// against the same call without the route (every item through the stream path), and one item that runs one by one.  Prints
// "layouts ok".
//
// Against the emulation library:   g++ -std=c++17 -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc tests/batch_dictionaries_zopfli_check.cpp
//                                      tests/emu/libbrotli_emu.so -Wl,-rpath,$PWD/tests/emu -o batch_dictionaries_zopfli_check
// Under a sanitizer the emulation sources are compiled into the program itself (the list is OBJS_SRC of tests/emu/Makefile):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DBROTLI_HOST_EMU=1 -I rust-brotli_amd/csrc
//       tests/batch_dictionaries_zopfli_check.cpp <OBJS_SRC> -o batch_dictionaries_zopfli_check_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/brotli_mi355x.h"

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

// Item i behind dictionary named[i].  The reference is the call without the route on the vectors: every item through the stream
// path.  Then, with the route, the host entry and the device entry on heap blocks of exactly each buffer's size; a dictionary
// longer than the window's (1 << lgwin) - 16 is allocated from its first byte in use on.  side: the items expected side by side.
int Layout(const std::vector<std::vector<uint8_t>>& dictionaries, const std::vector<std::vector<uint8_t>>& items, const std::vector<size_t>& named, int quality,
           int lgwin, size_t side) {
  const uint32_t routes = BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS;
  const size_t n = items.size(), nd = dictionaries.size();
  std::vector<const uint8_t*> plain_dicts(nd), plain_in(n);
  std::vector<size_t> dict_sizes(nd), in_sizes(n), want_sizes(n);
  std::vector<std::vector<uint8_t>> want(n);
  std::vector<uint8_t*> want_out(n);
  for (size_t k = 0; k < nd; ++k) {
    plain_dicts[k] = dictionaries[k].data();
    dict_sizes[k] = dictionaries[k].size();
  }
  for (size_t i = 0; i < n; ++i) {
    plain_in[i] = items[i].data();
    in_sizes[i] = items[i].size();
    want[i].resize(BrotliEncoderMaxCompressedSize(items[i].size()) + 1024);
    want_out[i] = want[i].data();
    want_sizes[i] = want[i].size();
  }
  if (!BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, BROTLI_MODE_GENERIC, 0, nd, plain_dicts.data(), dict_sizes.data(), n, named.data(),
                                                 plain_in.data(), in_sizes.data(), want_out.data(), want_sizes.data(), nullptr))
    return Fail("the call without the route", 0);
  uint64_t info[8];
  BrotliMi355xLastBatchInfo(info);
  if (info[1] != 0 || info[2] != n) return Fail("the call without the route took items side by side", (size_t)info[1]);

  const size_t window = ((size_t)1 << lgwin) - 16;
  int bad = 0;
  for (int device = 0; device < 2 && !bad; ++device) {
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
      out[i] = (uint8_t*)malloc(want_sizes[i] ? want_sizes[i] : 1);  // (exactly the stream: one byte more written is an error)
      out_sizes[i] = want_sizes[i];
    }
    std::vector<int32_t> results(n);
    const int32_t ok =
        device ? BrotliMi355xCompressBatchWithDictionariesDevice(quality, lgwin, BROTLI_MODE_GENERIC, routes, nd, dicts.data(), dict_sizes.data(), n, named.data(),
                                                                 in.data(), in_sizes.data(), out.data(), out_sizes.data(), results.data())
               : BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, BROTLI_MODE_GENERIC, routes, nd, dicts.data(), dict_sizes.data(), n, named.data(),
                                                           in.data(), in_sizes.data(), out.data(), out_sizes.data(), results.data());
    BrotliMi355xLastBatchInfo(info);
    if (!ok) bad = Fail(BrotliMi355xLastError(), 0);
    if (info[0] != n || info[1] != side || info[2] != n - side || info[6] != 0 || info[7] != 0) bad = Fail("items side by side", (size_t)info[1]);
    for (size_t i = 0; i < n && !bad; ++i)
      if (!results[i] || out_sizes[i] != want_sizes[i] || memcmp(out[i], want[i].data(), want_sizes[i]) != 0)
        bad = Fail(device ? "device entry: stream differs from the stream path's" : "host entry: stream differs from the stream path's", i);
    for (size_t k = 0; k < nd; ++k) free(dict_blocks[k]);
    for (size_t i = 0; i < n; ++i) {
      free(in[i]);
      free(out[i]);
    }
  }
  return bad;
}

int Layouts() {
  // (127 / 128 / 129: the first dictionary position the prepend stores and the stitch's threshold; 4097 and 20000 are cut at lgwin 10)
  static const size_t dictionary_sizes[] = {2, 3, 126, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1008, 4097, 20000};
  static const size_t item_sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 2049};
  std::vector<std::vector<uint8_t>> dictionaries, items;
  std::vector<size_t> each, one;
  for (size_t bytes : dictionary_sizes) dictionaries.push_back(Text(bytes));
  for (size_t bytes : item_sizes) {
    each.push_back((items.size() * 7) % dictionaries.size());
    one.push_back(13);  // the 4097-byte dictionary
    items.push_back(Text(bytes));
  }
  const size_t n = items.size();
  if (Layout(dictionaries, items, each, 11, 22, n) || Layout(dictionaries, items, each, 10, 22, n)) return 1;
  if (Layout(dictionaries, items, each, 11, 10, n) || Layout(dictionaries, items, each, 10, 16, n)) return 1;
  // one index named by every item: no image, the route all the same
  if (Layout(dictionaries, items, one, 11, 22, n) || Layout(dictionaries, items, one, 10, 10, n)) return 1;
  // one by one beside side-by-side items: the empty item, an item of 65 537 bytes, and a dictionary of one byte
  std::vector<std::vector<uint8_t>> mixed = {Text(3000), {}, Text(65537), Text(500)};
  std::vector<std::vector<uint8_t>> mixed_dictionaries = {Text(1000), Text(1)};
  if (Layout(mixed_dictionaries, mixed, {0, 0, 0, 1}, 11, 22, 1) || Layout(mixed_dictionaries, mixed, {0, 0, 0, 1}, 10, 18, 1)) return 1;
  printf("layouts ok\n");
  return 0;
}

}  // namespace

int main() { return Layouts(); }
