// batch_greedy.inc -- see batch_greedy.h: the plan of a group, its upload, the parse launch, the command gather and the
// hand-over to the meta-block stage.  The product library compiles it as batch_greedy.cpp; the emulation library, whose list of
// sources is fixed, gets it through cabi.cpp (the caller), together with the host emulation of the seam.
#include "batch_greedy.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <stdexcept>
#include <utility>

#include "batch_device.h"
#include "batch_q9.h"
#include "batch_quick.h"
#include "batch_zopfli.h"
#include "device_api.h"
#if defined(BROTLI_HOST_EMU)
#include "batch_device_emu.inc"  // the host emulation of batch_stage_device / batch_deliver / batch_gather_context
#include "batch_greedy_emu.inc"  // the host emulation of lz77_batch_parse / lz77_batch_gather
#include "batch_quick_emu.inc"   // ... and of lz77_quick_batch_parse
#include "batch_zopfli_emu.inc"  // ... and of lz77_zopfli_batch_parse
#endif

namespace brotli_mi355x {

namespace {

size_t EnvSize(const char* name, size_t otherwise) {
  const char* s = getenv(name);
  return s ? (size_t)strtoull(s, nullptr, 10) : otherwise;
}

// the parameters every eligible item of a call shares: FinalizeParams + ChooseHasher as EncodeStream runs them for a one-shot
// call whose size hint is the item's size (<= 1 << lgblock, so the hint reaches nothing the items differ in)
EncoderParams ItemParams(const EncoderParams& user, size_t input_size) {
  EncoderParams p = user;
  FinalizeParams(&p);
  p.size_hint = input_size;
  ChooseHasher(&p);
  return p;
}

// ... and behind BrotliEncoderSetCustomDictionary: no static dictionary, the hasher chosen inside that call with the size hint
// of then (none), the hint itself filled in by the FINISH call with the item's size (encode.rs:1196-1270, 1604-1620)
EncoderParams DictionaryItemParams(const EncoderParams& user, size_t input_size) {
  EncoderParams p = user;
  p.use_dictionary = false;
  FinalizeParams(&p);
  p.size_hint = 0;
  ChooseHasher(&p);
  p.size_hint = input_size;
  return p;
}

uint32_t Padded(uint32_t bytes) { return ((bytes + 63u) & ~63u) + 64u; }  // at least 64 zero bytes behind every item

// what every side-by-side route asks of the caller's parameters, whatever its qualities and sizes
bool PlainStreamParams(const EncoderParams& user) {
  return !user.large_window && !(user.catable || user.appendable || user.bare_stream || user.byte_align || user.magic_number);
}

}  // namespace

// The default of BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS (DESIGN.md section 10 has the sweep behind it).
static constexpr size_t kBatchDictImageMinItems = 16;
size_t BatchDictImageMinItems() {
  static const size_t min_items =
      EnvSize("BROTLI_MI355X_BATCH_DICT_SELF_FILE", 0) != 0 ? 0 : EnvSize("BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS", kBatchDictImageMinItems);
  return min_items;
}

BatchImageCounts& BatchImageTally() {
  static thread_local BatchImageCounts counts{0, 0, 0};
  return counts;
}

bool BatchGreedyEligible(const EncoderParams& user, size_t input_size) {
  if (input_size == 0) return false;  // (answered without an encoder)
  if (user.quality < 5 || user.quality > 8 || user.lgwin < 17 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  if (input_size > ((size_t)1 << 24)) return false;
  const EncoderParams p = ItemParams(user, input_size);
  return p.hasher.type == 5 && input_size <= ((size_t)1 << p.lgblock);
}

bool BatchDictionaryEligible(const EncoderParams& user, size_t dict_size, size_t input_size) {
  if (input_size == 0 || input_size > 65536 || dict_size < 2 || dict_size > 65536) return false;
  if (user.quality < 5 || user.quality > 8 || user.lgwin < 17 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  // (dictionary + item stay below the ring-buffer size, 1 << (lgwin + 1): no masked entry differs from its position)
  const EncoderParams p = DictionaryItemParams(user, input_size);
  return p.hasher.type == 5 && p.hasher.block_bits <= 7 && input_size <= ((size_t)1 << p.lgblock) && dict_size <= ((size_t)1 << p.lgwin) - 16;
}

bool BatchLongEligible(const EncoderParams& user, size_t input_size) {
  if (input_size > kBatchLongBytes) return false;
  if (user.quality < 5 || user.quality > 8 || user.lgwin < 17 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  // (kBatchLongBytes is the ring-buffer size at lgwin 17 and below the size hint that selects another hasher)
  const EncoderParams p = ItemParams(user, input_size);
  return p.hasher.type == 5 && p.hasher.block_bits <= 7 && input_size > ((size_t)1 << p.lgblock) &&
         input_size <= (size_t)kBatchLongBlocks << p.lgblock;
}

namespace {

// the search parameters of a chain whose stream starts at 0 and ends inside the first ring-buffer revolution
Lz77Params ChainParams(const EncoderParams& p) {
  Lz77Params P;
  memset(&P, 0, sizeof(P));
  P.ring_mask = (1u << ComputeRbBits(p)) - 1u;
  P.max_backward_limit = (1u << p.lgwin) - 16u;
  P.hasher_kind = p.hasher.type == 9 ? 9 : 5;  // as Lz77Stage::Setup: H9 (qualities 9 and 10) hashes like H5, onto 15 bits
  P.bucket_bits = (uint32_t)p.hasher.bucket_bits;
  P.block_bits = (uint32_t)p.hasher.block_bits;
  P.hash_len = (uint32_t)p.hasher.hash_len;
  P.ndist = (uint32_t)p.hasher.num_last_distances_to_check;
  P.htl = 4;
  P.literal_byte_score = (uint32_t)(p.hasher.literal_byte_score ? p.hasher.literal_byte_score : 540);
  P.score_per_byte = P.literal_byte_score >> 2;
  P.use_dictionary = p.use_dictionary ? 1 : 0;
  P.spree_window = p.hasher.type == 9 ? 512 : 64;  // (Lz77Stage::Setup: 512 from quality 9 on; the Zopfli walk has no use for it)
  P.dist_max_distance = (uint32_t)p.dist.max_distance;
  P.quality = (uint32_t)p.quality;
  P.num_segments = 1;
  P.dist_postfix_bits = p.dist.distance_postfix_bits;
  P.num_direct_distance_codes = p.dist.num_direct_distance_codes;
  P.masked_from = kNeverMasked;  // (an item ends inside the first ring-buffer revolution of its stream)
  P.block_bytes = 1u << p.lgblock;
  P.max_metablock_bytes = (uint32_t)MaxMetablockSize(p);
  return P;
}

// ---- the steps of a group: every route (CompressGroups, Batch*Compress) composes them in the same order.
// the limits of a group, read once per process, like BROTLI_MI355X_FRAGMENT_BATCH
struct BatchLimits {
  size_t group_items, group_bytes;
  size_t tables;  // 0: TablesMax works it out
};
const BatchLimits& Limits() {
  static const BatchLimits limits{std::max<size_t>(1, EnvSize("BROTLI_MI355X_BATCH_GROUP_ITEMS", 4096)),
                                  std::max<size_t>(1, EnvSize("BROTLI_MI355X_BATCH_GROUP_BYTES", (size_t)64 << 20)),
                                  EnvSize("BROTLI_MI355X_BATCH_TABLES", 0)};
  return limits;
}
// a table is 1 MiB at quality 5 and 16 MiB at quality 8, 256 KiB (H2, H3) or 512 KiB (H4) at qualities 2 .. 4, 32 MiB + 64 KiB
// at qualities 9 and 10 (255 of them): as many as the parse kernel keeps resident (256 CUs x 4 SIMDs x 4 wavefronts) within 8 GiB
size_t TablesMax(size_t table_bytes) {
  return Limits().tables ? Limits().tables : std::max<size_t>(1, std::min<size_t>(4096, ((size_t)8 << 30) / table_bytes));
}

// Qualities 2 .. 4: the hasher and the search parameters of the chains, in a job that has no group yet (QuickGroupJob)
QuickBatchJob QuickChains(const EncoderParams& p) {
  QuickBatchJob J{};
  QuickJob& Q = J.Q;  // as Lz77Stage::Setup fills it in
  Q.kind = (uint32_t)p.hasher.type;
  Q.bucket_bits = Q.kind == 4 ? 17 : 16;
  Q.sweep = Q.kind == 2 ? 1 : (Q.kind == 3 ? 2 : 4);
  Q.hash_len = 5;
  Q.use_dictionary = (p.use_dictionary && (Q.kind == 2 || Q.kind == 4)) ? 1 : 0;
  J.P = ChainParams(p);  // (ring_mask: the items' own ring buffer, which an item of three blocks outruns at lgwin <= 14)
  J.P.hasher_kind = 6;  // (what Lz77Stage::Setup gives every hasher but H5 and H9; br_quick_block does not look at it)
  J.P.htl = 8;  // HashTypeLength of every BasicHasher
  J.P.use_dictionary = Q.use_dictionary;
  J.P.dict_break = 0;
  return J;
}
size_t QuickTableBytes(const QuickBatchJob& J) { return (size_t)quick_table_words(J.Q) * 4; }

// the page-locked arrays of a call: they live across its groups and grow through resize_discard only
struct CallArrays {
  PinnedArray<uint8_t> staging;
  PinnedArray<BatchItem> items;
  PinnedArray<uint32_t> order, offsets, starts;
  PinnedArray<uint32_t> dict_bytes, dict_off;  // a dictionary per item: its bytes, and where it starts in `dict_pool`
  PinnedArray<uint8_t> dict_pool;
  PinnedArray<BatchRecord> records;
  PinnedArray<BatchLongRecord> long_records;
  PinnedArray<const uint8_t*> sources;  // items in device memory: their addresses
};
// one group, staged and uploaded: the caller's items [first, last)
struct Group {
  CallArrays* A;
  DevBlocks mem;  // everything the group has on the device: freed with the group, also when a step throws
  size_t first, last;
  uint32_t n;
  size_t padded;     // bytes of the padded text
  size_t packed_at;  // where the packed text starts in `uploaded`
  size_t cmd_slots;
  uint32_t tables;
  uint8_t* uploaded;  // on the device, like the two below
  bool on_device;     // the caller's items lie in device memory: `uploaded` was filled there (batch_stage_device)
  BatchItem* items_dev;
  uint32_t* order_dev;
  // on_device behind dictionaries: the padded text, dictionary | item per item, laid out by the same launch that filled `uploaded`
  // (batch_stage_dicts_device), and A->dict_bytes on the device; nullptr for every other group
  uint8_t* dict_text = nullptr;
  uint32_t* dict_bytes_dev = nullptr;
};
// The dictionary bytes that go in front of every item of a call in the padded text: one size for all of them (the calls with a
// shared dictionary; 0: none) or a size per item, of which "all equal" is the former.
// Where the items lie in device memory the dictionaries do too: their device addresses stand beside the sizes, first byte in use.
struct DictSizes {
  uint32_t all;
  const size_t* each;  // [count], nullptr: `all`
  const uint8_t* all_dev = nullptr;          // the device mode: the one dictionary ...
  const uint8_t* const* each_dev = nullptr;  // ... or [count], that of every item
  DictSizes(uint32_t all_items, const uint8_t* all_items_dev = nullptr) : all(all_items), each(nullptr), all_dev(all_items_dev) {}
  explicit DictSizes(const size_t* per_item, const uint8_t* const* per_item_dev = nullptr) : all(0), each(per_item), each_dev(per_item_dev) {}
  bool any() const { return each != nullptr || all != 0; }
  uint32_t of(size_t i) const { return each ? (uint32_t)each[i] : all; }
  const uint8_t* dev(size_t i) const { return each_dev ? each_dev[i] : all_dev; }
};
uint32_t DictRoom(uint32_t D) { return (D + 63u) & ~63u; }
// dict: the dictionary bytes of every item of the call; with a size per item g->A->dict_bytes holds those of the group's items
// max_items: a bound of the route's own on the items of a group, below BROTLI_MI355X_BATCH_GROUP_ITEMS (0: none)
// on_device: inputs[i] is a device address.  The same buffer with the same layout is allocated zeroed on the device and filled
// there by one launch from an array of the group's source addresses: no staging buffer, no memcpy, no bulk upload.  Behind
// dictionaries (dict.dev(i): their device addresses) the same launch lays out the padded text as well (g->dict_text), every
// dictionary read where it lies: no pool, no upload, and no lz77_batch_dict_text / lz77_batch_dicts_text for the route to run.
void StageGroup(size_t first, size_t count, const uint8_t* const* inputs, const size_t* sizes, const DictSizes& dict, size_t tables_max,
                CallArrays* arrays, Group* g, size_t max_items = 0, bool on_device = false) {
  CallArrays& A = *arrays;
  // (the limit counts the dictionary copies of the padded text: scratch -- keys and flags -- grows with them)
  size_t last = first, padded = 0, packed = 0, dict_copies = 0;
  const size_t group_items = max_items ? std::min(max_items, Limits().group_items) : Limits().group_items;
  while (last < count && last - first < group_items &&
         (last == first || packed + dict_copies + dict.of(last) + sizes[last] <= Limits().group_bytes)) {
    padded += DictRoom(dict.of(last)) + Padded((uint32_t)sizes[last]);
    packed += sizes[last];
    dict_copies += dict.of(last);
    ++last;
  }
  const uint32_t n = (uint32_t)(last - first);
  // one page-locked buffer, one upload: [padded text | 64 | packed text | 64]; with a dictionary the packed text alone -- the
  // padded text, dictionary | item per item, is laid out on the device
  const size_t packed_at = dict.any() ? 0 : padded + 64;
  const size_t text_bytes = packed_at + packed + 64;
  if (!on_device) {
    A.staging.resize_discard(text_bytes);
    memset(A.staging.data(), 0, text_bytes);
  }
  const bool dicts_on_device = on_device && dict.any();
  A.sources.resize_discard(on_device ? (dicts_on_device ? 2 * (size_t)n : n) : 0);  // (the items' addresses, then the dictionaries')
  A.items.resize_discard(n);
  A.order.resize_discard(n);
  A.starts.resize_discard(n);
  A.dict_bytes.resize_discard(n);
  uint32_t off = 0, start = 0, cmd_base = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t bytes = (uint32_t)sizes[first + i];
    const uint32_t cmd_cap = bytes / 2 + 8;
    A.dict_bytes[i] = dict.of(first + i);
    off += DictRoom(A.dict_bytes[i]);
    if (on_device) {
      A.sources[i] = inputs[first + i];
      if (dicts_on_device) A.sources[n + i] = dict.dev(first + i);
    } else {
      if (!dict.any()) memcpy(A.staging.data() + off, inputs[first + i], bytes);
      memcpy(A.staging.data() + packed_at + start, inputs[first + i], bytes);
    }
    A.items[i] = BatchItem{off, bytes, cmd_base, cmd_cap};
    A.starts[i] = start;
    off += Padded(bytes);
    start += bytes;
    cmd_base += cmd_cap;
    A.order[i] = i;
  }
  // largest first: the large items of a group run as long as a lone wavefront takes, the small ones fill in behind them.  The
  // length of a chain's work is dictionary + item where the chain files its dictionary itself; behind a shared dictionary the
  // sum orders the items as their sizes do.
  std::stable_sort(A.order.data(), A.order.data() + n,
                   [&](uint32_t a, uint32_t b) { return A.dict_bytes[a] + A.items[a].bytes > A.dict_bytes[b] + A.items[b].bytes; });

  g->A = arrays;
  g->first = first;
  g->last = last;
  g->n = n;
  g->padded = padded;
  g->packed_at = packed_at;
  g->cmd_slots = (size_t)A.items[n - 1].cmd_base + A.items[n - 1].cmd_cap;
  g->tables = (uint32_t)std::min<size_t>(tables_max, n);
  g->on_device = on_device;
  if (on_device) {
    g->uploaded = g->mem.zeroed<uint8_t>(text_bytes);
  } else {
    g->uploaded = g->mem.uninit<uint8_t>(text_bytes);
    dev_h2d_bulk(g->uploaded, A.staging.data(), text_bytes);
  }
  g->items_dev = g->mem.uninit<BatchItem>((size_t)n * sizeof(BatchItem));
  dev_h2d(g->items_dev, A.items.data(), (size_t)n * sizeof(BatchItem));
  g->order_dev = g->mem.uninit<uint32_t>((size_t)n * 4);
  dev_h2d(g->order_dev, A.order.data(), (size_t)n * 4);
  if (on_device) {
    const uint8_t** sources_dev = g->mem.uninit<const uint8_t*>(A.sources.size() * sizeof(const uint8_t*));
    dev_h2d(sources_dev, A.sources.data(), A.sources.size() * sizeof(const uint8_t*));
    uint32_t* starts_dev = g->mem.uninit<uint32_t>((size_t)n * 4);
    dev_h2d(starts_dev, A.starts.data(), (size_t)n * 4);
    if (dicts_on_device) {
      g->dict_bytes_dev = g->mem.uninit<uint32_t>((size_t)n * 4);
      dev_h2d(g->dict_bytes_dev, A.dict_bytes.data(), (size_t)n * 4);
      g->dict_text = g->mem.zeroed<uint8_t>(padded + 64);
      batch_stage_dicts_device(sources_dev, sources_dev + n, g->dict_bytes_dev, g->items_dev, starts_dev, n, g->dict_text, g->uploaded + packed_at);
    } else {
      batch_stage_device(sources_dev, g->items_dev, starts_dev, n, g->uploaded, g->uploaded + packed_at);
    }
  }
}

// The device sink of a group: the streams that go out leave the group's output (out_dev, still on the device) for the caller's
// device buffers by one launch, the others get their answer by the sink's rule.  An item that takes the stored fallback is copied from
// the group's packed text.  item: the group's; out_byte / out_bytes: where its stream lies in out_dev.
struct Outgoing {
  uint32_t item;
  uint64_t out_byte, out_bytes;
};
void DeliverGroup(Group& g, const uint8_t* out_dev, const std::vector<Outgoing>& outgoing, const BatchDeviceSink& sink) {
  CallArrays& A = *g.A;
  std::vector<BatchDeliverOp> ops;
  for (const Outgoing& o : outgoing) {
    const size_t k = g.first + o.item;
    const uint32_t bytes = A.items[o.item].bytes;
    switch (sink.rule((size_t)o.out_bytes, bytes, sink.capacities[k])) {
      case Delivery::kStream:
        ops.push_back({(uint64_t)(uintptr_t)sink.outputs[k], o.out_byte, o.out_bytes});
        sink.sizes[k] = (size_t)o.out_bytes;
        sink.results[k] = 1;
        break;
      case Delivery::kStored:
        sink.sizes[k] = StoredStreamToDevice(g.uploaded + g.packed_at + A.starts[o.item], bytes, sink.outputs[k]);
        sink.results[k] = 1;
        break;
      case Delivery::kFails:
        sink.sizes[k] = 0;
        sink.results[k] = 0;
        break;
    }
  }
  if (ops.empty()) return;
  BatchDeliverOp* ops_dev = g.mem.uninit<BatchDeliverOp>(ops.size() * sizeof(BatchDeliverOp));
  dev_h2d(ops_dev, ops.data(), ops.size() * sizeof(BatchDeliverOp));
  batch_deliver(out_dev, ops_dev, (uint32_t)ops.size());
}

// the key pass over the group's padded text and the job of an H5 parse launch; `records` and `dict` are the caller's to set
BatchParseJob GreedyJob(const EncoderParams& p, const Lz77Params& P, Group& g, uint8_t* text) {
  const size_t keys_per_table = (size_t)1 << p.hasher.bucket_bits;
  Lz77Buffers B{};
  B.text = text;
  B.keys = g.mem.uninit<uint16_t>(g.padded * 2 + 256);
  B.changed_count = g.mem.zeroed<uint32_t>(64);
  Lz77Params PK = P;
  PK.total_bytes = (uint32_t)g.padded;  // (the last item's padding gives every position four bytes to hash)
  lz77_compute_keys(PK, B);

  BatchParseJob J{};
  J.P = P;
  J.text = text;
  J.keys = B.keys;
  J.flags = g.mem.uninit<uint8_t>(g.padded + 64);
  J.slabs = g.mem.uninit<Command>(g.cmd_slots * sizeof(Command) + 64);
  J.items = g.items_dev;
  J.order = g.order_dev;
  J.n_items = g.n;
  J.tables = g.tables;
  J.num = g.mem.uninit<uint16_t>((size_t)g.tables * keys_per_table * 2 + 64);
  J.buckets = g.mem.uninit<uint32_t>(((size_t)g.tables * keys_per_table << p.hasher.block_bits) * 4 + 64);
  J.counter = g.mem.zeroed<uint32_t>(64);
  return J;
}

// the job of a BasicHasher parse launch: no key pass and no flags -- a BasicHasher hashes from the text -- and a table of
// quick_table_words per wavefront; `records` is the caller's to set
QuickBatchJob QuickGroupJob(const QuickBatchJob& chains, Group& g) {
  QuickBatchJob J = chains;
  J.Q.table = g.mem.uninit<uint32_t>((size_t)g.tables * QuickTableBytes(J) + 64);  // (every chain fills its whole table in front of every item: zeros, or the dictionary's image)
  J.text = g.uploaded;
  J.slabs = g.mem.uninit<Command>(g.cmd_slots * sizeof(Command) + 64);
  J.items = g.items_dev;
  J.order = g.order_dev;
  J.n_items = g.n;
  J.tables = g.tables;
  J.counter = g.mem.zeroed<uint32_t>(64);
  return J;
}
// ... and what the gathers want of it: br_raw_command / br_finish_command are those of qualities 5 .. 8, and they read the
// slabs, the items, the records and the distance parameters
BatchParseJob GatherJobOf(const QuickBatchJob& J) {
  BatchParseJob G{};
  G.P = J.P;
  G.slabs = J.slabs;
  G.items = J.items;
  G.n_items = J.n_items;
  G.records = J.records;
  return G;
}

// (cannot happen: a copy is at least two bytes long)
void CheckSlab(uint32_t overflow) {
  if (overflow) throw std::runtime_error("brotli_mi355x: a batch chain ran out of its command slab");
}

// One-block items, from the records on: the gather offsets and one meta-block entry per item (one small round trip), the command
// gather, one meta-block per item, and the streams of the items the reference does not fail on.  J: the parse job, or what
// GatherJobOf leaves of it.
// sink != nullptr: the device mode (BatchDeviceSink).
void FinishOneBlockItems(const EncoderParams& p, const BatchParseJob& J, Group& g, std::vector<std::vector<uint8_t>>* streams,
                         std::vector<uint8_t>* reference_fails, const BatchDeviceSink* sink = nullptr) {
  CallArrays& A = *g.A;
  A.records.resize_discard(g.n);
  dev_d2h(A.records.data(), J.records, (size_t)g.n * sizeof(BatchRecord));
  A.offsets.resize_discard(g.n);
  std::vector<BatchStreamItem> mbs(g.n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < g.n; ++i) {
    const BatchRecord& r = A.records[i];
    CheckSlab(r.overflow);
    A.offsets[i] = (uint32_t)total;
    mbs[i].start = A.starts[i];
    mbs[i].bytes = A.items[i].bytes;
    mbs[i].cmd_offset = (uint32_t)total;
    mbs[i].n_cmds = r.n_cmds;
    mbs[i].n_lits = r.n_lits;
    mbs[i].uncompressed = r.uncompressed;
    // (the Zopfli chains behind a dictionary per item leave their dictionary's last two bytes in pad[0], every other chain 0: what
    // the quality >= 10 UTF-8 census reads in front of the stream, EncodeBatchMetaBlocks)
    mbs[i].prev_byte2 = (uint8_t)(r.pad[0] & 0xffu);
    mbs[i].prev_byte = (uint8_t)((r.pad[0] >> 8) & 0xffu);
    total += r.n_cmds;
    if (r.bad_commands != 0 && reference_fails) (*reference_fails)[g.first + i] = 1;
  }
  uint32_t* offsets_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
  dev_h2d(offsets_dev, A.offsets.data(), (size_t)g.n * 4);
  Command* cmds = g.mem.uninit<Command>((size_t)(total + 16) * sizeof(Command));
  lz77_batch_gather(J, offsets_dev, cmds);
  std::vector<uint8_t> out;
  if (sink) {
    BatchOutputOnDevice keep{&g.mem, nullptr};
    EncodeBatchMetaBlocks(p, g.uploaded + g.packed_at, cmds, (uint32_t)total, &mbs, &out, &keep);
    std::vector<Outgoing> outgoing;
    for (uint32_t i = 0; i < g.n; ++i)
      if (A.records[i].bad_commands == 0) outgoing.push_back({i, mbs[i].out_byte, mbs[i].out_bytes});
    DeliverGroup(g, keep.bytes, outgoing, *sink);
    return;
  }
  EncodeBatchMetaBlocks(p, g.uploaded + g.packed_at, cmds, (uint32_t)total, &mbs, &out);
  for (uint32_t i = 0; i < g.n; ++i)
    if (A.records[i].bad_commands == 0) (*streams)[g.first + i].assign(out.begin() + (ptrdiff_t)mbs[i].out_byte, out.begin() + (ptrdiff_t)(mbs[i].out_byte + mbs[i].out_bytes));
}

// Items of several blocks, from the records on: the same with a gather offset and an entry per meta-block.  A record is taken as
// far as its meta-blocks follow each other inside the item: one that would pass the item's end stops the walk.  (For the H5 kernel
// that test changes no outcome: behind such a meta-block `at` cannot come back to the item's size, and the same error is thrown.)
// An item's first entry says where its stream lies, or that a meta-block of it took the size fallback (`demoted`: no stream).
// sink != nullptr: the device mode (BatchDeviceSink) -- `inputs` are device addresses and are not read here: the context bytes of
// the follow-on meta-blocks come from the group's packed text, one small gather and one download per group.
void FinishLongItems(const EncoderParams& p, const BatchParseJob& J, const BatchLongRecord* records_dev, const uint8_t* const* inputs, Group& g,
                     std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* demoted, const BatchDeviceSink* sink = nullptr) {
  CallArrays& A = *g.A;
  A.long_records.resize_discard(g.n);
  dev_d2h(A.long_records.data(), records_dev, (size_t)g.n * sizeof(BatchLongRecord));
  A.offsets.resize_discard((size_t)g.n * kBatchLongBlocks);
  std::vector<BatchStreamItem> mbs;
  std::vector<uint32_t> first_mb(g.n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < g.n; ++i) {
    const BatchLongRecord& r = A.long_records[i];
    const BatchItem& item = A.items[i];
    CheckSlab(r.overflow);
    uint32_t at = 0, cmd_at = 0;
    first_mb[i] = (uint32_t)mbs.size();
    for (uint32_t m = 0; m < kBatchLongBlocks; ++m) A.offsets[(size_t)i * kBatchLongBlocks + m] = 0;
    for (uint32_t m = 0; m < r.n_mb && m < kBatchLongBlocks; ++m) {
      const BatchLongMetaBlock& mb = r.mb[m];
      if (mb.start != at || mb.bytes == 0 || mb.bytes > item.bytes - at || mb.first_cmd != cmd_at) break;
      A.offsets[(size_t)i * kBatchLongBlocks + m] = (uint32_t)total;
      BatchStreamItem e{};
      e.start = A.starts[i] + mb.start;
      e.bytes = mb.bytes;
      e.cmd_offset = (uint32_t)total;
      e.n_cmds = mb.n_cmds + (mb.trailing != 0 ? 1u : 0u);
      e.n_lits = mb.n_lits;
      e.uncompressed = mb.uncompressed;
      e.follows = m != 0;
      e.more = m + 1 != r.n_mb;
      e.item_bytes = item.bytes;
      if (m != 0 && !g.on_device) {
        e.prev_byte = inputs[g.first + i][mb.start - 1];
        e.prev_byte2 = inputs[g.first + i][mb.start - 2];
      }
      mbs.push_back(e);
      total += e.n_cmds;
      at += mb.bytes;
      cmd_at += mb.n_cmds;
    }
    if (at != item.bytes || cmd_at > item.cmd_cap) throw std::runtime_error("brotli_mi355x: a batch chain left meta-block records that do not cover its item");
  }
  uint32_t* offsets_dev = g.mem.uninit<uint32_t>((size_t)g.n * kBatchLongBlocks * 4);
  dev_h2d(offsets_dev, A.offsets.data(), (size_t)g.n * kBatchLongBlocks * 4);
  Command* cmds = g.mem.uninit<Command>((size_t)(total + 16) * sizeof(Command));
  lz77_batch_gather_long(J, records_dev, offsets_dev, cmds);
  if (g.on_device) {
    std::vector<uint32_t> at;
    for (const BatchStreamItem& e : mbs)
      if (e.follows) at.push_back(e.start);  // (mb.start is a whole number of input blocks: at least 2)
    if (!at.empty()) {
      uint32_t* at_dev = g.mem.uninit<uint32_t>(at.size() * 4);
      dev_h2d(at_dev, at.data(), at.size() * 4);
      uint8_t* context_dev = g.mem.zeroed<uint8_t>(at.size() * 2);
      batch_gather_context(g.uploaded + g.packed_at, at_dev, (uint32_t)at.size(), context_dev);
      std::vector<uint8_t> context(at.size() * 2);
      dev_d2h(context.data(), context_dev, context.size());
      size_t k = 0;
      for (BatchStreamItem& e : mbs)
        if (e.follows) {
          e.prev_byte = context[2 * k];
          e.prev_byte2 = context[2 * k + 1];
          ++k;
        }
    }
  }
  std::vector<uint8_t> out;
  if (sink) {
    BatchOutputOnDevice keep{&g.mem, nullptr};
    EncodeBatchMetaBlocks(p, g.uploaded + g.packed_at, cmds, (uint32_t)total, &mbs, &out, &keep);
    std::vector<Outgoing> outgoing;
    for (uint32_t i = 0; i < g.n; ++i) {
      const BatchStreamItem& e = mbs[first_mb[i]];
      if (e.demoted) (*demoted)[g.first + i] = 1; else outgoing.push_back({i, e.out_byte, e.out_bytes});
    }
    DeliverGroup(g, keep.bytes, outgoing, *sink);
    return;
  }
  EncodeBatchMetaBlocks(p, g.uploaded + g.packed_at, cmds, (uint32_t)total, &mbs, &out);
  for (uint32_t i = 0; i < g.n; ++i) {
    const BatchStreamItem& e = mbs[first_mb[i]];
    if (e.demoted) {
      (*demoted)[g.first + i] = 1;
      continue;
    }
    (*streams)[g.first + i].assign(out.begin() + (ptrdiff_t)e.out_byte, out.begin() + (ptrdiff_t)(e.out_byte + e.out_bytes));
  }
}

// Qualities 5 .. 8, items of one block, and qualities 9 / 10 on the H9 hasher (BatchQ9Compress: p.hasher.type == 9, no dictionary;
// BatchQ9CompressWithDictionary: quality 9 behind the shared dictionary, whose image is 64 KiB of counters and at most D entries --
// the scratch table lz77_batch_dict_image files it on is a whole H9 table, 32 MiB allocated and D slots of it touched).
// p: the parameters the items share, finalized.  dict == nullptr: the plain call.
void CompressGroups(const EncoderParams& p, const uint8_t* dict, uint32_t D, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                    std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails, uint32_t* groups,
                    const BatchDeviceSink* sink = nullptr) {
  streams->assign(count, std::vector<uint8_t>());
  if (reference_fails) reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const size_t keys_per_table = (size_t)1 << p.hasher.bucket_bits;
  const size_t tables_max = TablesMax(keys_per_table * 2 + (keys_per_table << p.hasher.block_bits) * 4);
  const Lz77Params P = ChainParams(p);

  // ---- the dictionary, once per call: its bytes on the device, and what the prepend leaves in a table (BatchDictImage)
  DevBlocks call_mem;
  uint8_t *dict_shifted = nullptr, *dict_dev = nullptr;
  BatchDictImage image{};
  // measurement only (DESIGN.md section 10): no image, every chain files the dictionary itself with br_live_store
  static const bool self_file = EnvSize("BROTLI_MI355X_BATCH_DICT_SELF_FILE", 0) != 0;
  if (D != 0) {
    // (shifted so that it ends on a 16-byte boundary, like its copies in the padded text: k_batch_dict_text moves whole words)
    dict_shifted = call_mem.zeroed<uint8_t>((size_t)D + 16 + 64);
    dict_dev = dict_shifted + ((0u - D) & 15u);
    if (sink) batch_copy_device(dict_dev, dict, D); else dev_h2d_bulk(dict_dev, dict, D);  // (the device mode: `dict` is a device address)
    image.bytes = D;
  }
  if (D != 0 && !self_file) {
    Lz77Buffers B{};
    B.text = dict_dev;
    B.keys = call_mem.uninit<uint16_t>((size_t)D * 2 + 256);
    B.changed_count = call_mem.zeroed<uint32_t>(64);
    B.dict_items = nullptr;
    B.run_end = nullptr;
    Lz77Params PK = P;
    PK.total_bytes = D;  // (every filed position hashes dictionary bytes only)
    lz77_compute_keys(PK, B);
    uint16_t* num = call_mem.uninit<uint16_t>(keys_per_table * 2 + 64);
    uint32_t* scratch_buckets = call_mem.uninit<uint32_t>((keys_per_table << p.hasher.block_bits) * 4 + 64);
    uint32_t* entries = call_mem.uninit<uint32_t>((size_t)D * 8 + 64);
    uint32_t* n_entries = call_mem.zeroed<uint32_t>(64);
    lz77_batch_dict_image(P, B.keys, D, num, scratch_buckets, entries, n_entries);
    image.bytes = D;
    image.num = num;
    image.entries = entries;
    image.n_entries = n_entries;
    ++BatchImageTally().images;
  }

  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(D, dict_dev), tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    uint8_t* text = g.uploaded;
    if (D != 0) (image.entries != nullptr ? BatchImageTally().replayed : BatchImageTally().filed) += g.n;
    if (g.dict_text) {
      text = g.dict_text;  // (the device mode: laid out with the staging, from the call's own copy of the dictionary)
    } else if (D != 0) {
      text = g.mem.zeroed<uint8_t>(g.padded + 64);
      uint32_t* starts_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
      dev_h2d(starts_dev, A.starts.data(), (size_t)g.n * 4);
      lz77_batch_dict_text(dict_shifted, D, g.uploaded, starts_dev, g.items_dev, g.n, text);
    }
    BatchParseJob J = GreedyJob(p, P, g, text);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    J.dict = image;
    if (P.hasher_kind == 9) lz77_batch_parse_h9(J); else lz77_batch_parse(J);
    FinishOneBlockItems(p, J, g, streams, reference_fails, sink);
    first = g.last;
  }
}

// A dictionary per item, one step for the routes of qualities 5 .. 8 and 2 .. 4: a group uploads, once each, the dictionaries its
// items name -- a pool in which every dictionary ends on a 16-byte boundary behind zero bytes of its own (the dict_shifted
// convention of lz77_batch_dict_text), with the place and the size of item i's dictionary beside it -- and lays out the padded
// text, dictionary | item per item, on the device.  (The group's byte limit counts a dictionary per item, so the pool stays
// below it.)  dicts[i] / dict_sizes[i]: the dictionary of the call's item i as in use; two items share one where pointer and
// size agree.  In the device mode every item reads its dictionary where it lies, and the step hands on what StageGroup left.
struct DictsText {
  uint8_t* text;             // the group's padded text
  uint32_t* dict_bytes_dev;  // [g.n]: A.dict_bytes on the device
};
DictsText StageDictsText(Group& g, const uint8_t* const* dicts, const size_t* dict_sizes) {
  if (g.dict_text) return DictsText{g.dict_text, g.dict_bytes_dev};  // the device mode: StageGroup has laid the text out
  CallArrays& A = *g.A;
  const size_t first = g.first;
  std::map<std::pair<const uint8_t*, size_t>, uint32_t> placed;
  A.dict_off.resize_discard(g.n);
  size_t pool_bytes = 0;
  for (uint32_t i = 0; i < g.n; ++i)
    if (placed.emplace(std::make_pair(dicts[first + i], dict_sizes[first + i]), 0u).second) pool_bytes += (dict_sizes[first + i] + 15) & ~(size_t)15;
  A.dict_pool.resize_discard(pool_bytes + 64);
  placed.clear();
  uint32_t at = 0;
  for (uint32_t i = 0; i < g.n; ++i) {
    const uint32_t D = A.dict_bytes[i], lead = (0u - D) & 15u;
    const auto slot = placed.emplace(std::make_pair(dicts[first + i], dict_sizes[first + i]), at + lead);
    if (slot.second) {
      memset(A.dict_pool.data() + at, 0, lead);
      memcpy(A.dict_pool.data() + at + lead, dicts[first + i], D);
      at += lead + D;
    }
    A.dict_off[i] = slot.first->second;
  }
  memset(A.dict_pool.data() + at, 0, 64);
  uint8_t* pool_dev = g.mem.uninit<uint8_t>(pool_bytes + 64);
  dev_h2d_bulk(pool_dev, A.dict_pool.data(), pool_bytes + 64);
  uint32_t* dict_off_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
  dev_h2d(dict_off_dev, A.dict_off.data(), (size_t)g.n * 4);
  DictsText out;
  out.dict_bytes_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
  dev_h2d(out.dict_bytes_dev, A.dict_bytes.data(), (size_t)g.n * 4);
  uint32_t* starts_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
  dev_h2d(starts_dev, A.starts.data(), (size_t)g.n * 4);
  out.text = g.mem.zeroed<uint8_t>(g.padded + 64);
  lz77_batch_dicts_text(pool_dev, dict_off_dev, out.dict_bytes_dev, g.uploaded, starts_dev, g.items_dev, g.n, out.text);
  return out;
}

// The dictionaries of a group that get an image: those that at least BatchDictImageMinItems() of its items name, and never one
// that a single item names -- build plus replay cannot beat one filing.  At most kBatchGroupImages, the most named first, ties to
// the dictionary that appears first in the group.  Dictionaries are told apart as StageDictsText does it: by pointer and size in use.
struct GroupImages {
  std::vector<uint32_t> item_image;  // [g.n]: the image of item i's dictionary, or kBatchNoImage
  std::vector<uint32_t> first_item;  // [images]: the first item of the group that names the image's dictionary
  uint32_t replayed = 0;             // items with an image
};
GroupImages PickGroupImages(const Group& g, const uint8_t* const* dicts, const size_t* dict_sizes) {
  GroupImages out;
  out.item_image.assign(g.n, kBatchNoImage);
  const size_t min_items = BatchDictImageMinItems();
  if (min_items == 0) return out;
  struct Named {
    uint32_t first, items;
  };
  std::map<std::pair<const uint8_t*, size_t>, uint32_t> place;  // -> index into `named`
  std::vector<Named> named;
  std::vector<uint32_t> of_item(g.n);
  for (uint32_t i = 0; i < g.n; ++i) {
    const auto slot = place.emplace(std::make_pair(dicts[g.first + i], dict_sizes[g.first + i]), (uint32_t)named.size());
    if (slot.second) named.push_back(Named{i, 0});
    of_item[i] = slot.first->second;
    ++named[of_item[i]].items;
  }
  std::vector<uint32_t> chosen;
  for (uint32_t k = 0; k < named.size(); ++k)
    if (named[k].items >= std::max<size_t>(min_items, 2)) chosen.push_back(k);
  // (`named` is in the order of first appearance, and the sort keeps it among equals)
  std::stable_sort(chosen.begin(), chosen.end(), [&](uint32_t a, uint32_t b) { return named[a].items > named[b].items; });
  if (chosen.size() > kBatchGroupImages) chosen.resize(kBatchGroupImages);
  std::vector<uint32_t> image_of(named.size(), kBatchNoImage);
  for (uint32_t j = 0; j < chosen.size(); ++j) {
    image_of[chosen[j]] = j;
    out.first_item.push_back(named[chosen[j]].first);
  }
  for (uint32_t i = 0; i < g.n; ++i) {
    out.item_image[i] = image_of[of_item[i]];
    if (out.item_image[i] != kBatchNoImage) ++out.replayed;
  }
  return out;
}
// ... counted for BrotliMi355xLastBatchImageInfo, and the image numbers of the items on the device (nullptr: the group has no image)
const uint32_t* CountGroupImages(Group& g, const GroupImages& gi) {
  BatchImageCounts& tally = BatchImageTally();
  tally.images += gi.first_item.size();
  tally.replayed += gi.replayed;
  tally.filed += g.n - gi.replayed;
  if (gi.first_item.empty()) return nullptr;
  uint32_t* item_image_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
  dev_h2d(item_image_dev, gi.item_image.data(), (size_t)g.n * 4);
  return item_image_dev;
}

// The images of an H5 / H9 group, built into group-scoped memory from the copy of each dictionary that the text layout has put in
// front of the first item that names it, with the keys of the group's key pass (so the device form needs no copy of its own) and the
// group's own tables as the scratch: the parse launch empties or overwrites every counter in front of every item anyway, which
// saves 16 / 32 MiB of scratch per image at quality 8 / 9.  An image is its counters (32 / 64 KiB) and at most D entries of 8 bytes.
void BuildGroupImages(Group& g, const GroupImages& gi, BatchParseJob* J) {
  J->item_image = CountGroupImages(g, gi);
  if (J->item_image == nullptr) return;
  CallArrays& A = *g.A;
  const uint32_t n_images = (uint32_t)gi.first_item.size();
  const size_t keys_per_table = (size_t)1 << J->P.bucket_bits;
  std::vector<BatchImagePlan> plan(n_images);
  uint32_t entries_at = 0;
  for (uint32_t j = 0; j < n_images; ++j) {
    const uint32_t i = gi.first_item[j], D = A.dict_bytes[i];
    plan[j] = BatchImagePlan{A.items[i].text_off - D, D, entries_at, 0};
    entries_at += D;
  }
  BatchImagePlan* plan_dev = g.mem.uninit<BatchImagePlan>((size_t)n_images * sizeof(BatchImagePlan));
  dev_h2d(plan_dev, plan.data(), (size_t)n_images * sizeof(BatchImagePlan));
  uint16_t* num = g.mem.uninit<uint16_t>((size_t)n_images * keys_per_table * 2 + 64);
  uint32_t* entries = g.mem.uninit<uint32_t>((size_t)entries_at * 8 + 64);
  uint32_t* n_entries = g.mem.zeroed<uint32_t>((size_t)n_images * 4 + 64);
  lz77_batch_dict_images(*J, n_images, plan_dev, num, entries, n_entries);
  std::vector<BatchDictImage> images(n_images);
  for (uint32_t j = 0; j < n_images; ++j)
    images[j] = BatchDictImage{plan[j].bytes, num + (size_t)j * keys_per_table, entries + 2 * (size_t)plan[j].entries_at, n_entries + j};
  BatchDictImage* images_dev = g.mem.uninit<BatchDictImage>((size_t)n_images * sizeof(BatchDictImage));
  dev_h2d(images_dev, images.data(), (size_t)n_images * sizeof(BatchDictImage));
  J->images = images_dev;
}

// Qualities 5 .. 8 behind a dictionary per item: the steps of CompressGroups' dictionary path in the text StageDictsText lays out,
// with an image per frequently named dictionary of the group (PickGroupImages, BuildGroupImages) where CompressGroups has the one of
// its call: the chain of an item that names such a dictionary replays the image, every other chain files its own dictionary
// (br_batch_item<kRows, true, true>).
// Quality 9 (BatchQ9CompressWithDictionaries: p.hasher.type == 9) takes the same steps onto H9 tables and br_batch_item_h9_dict<true>.
// dicts[i] / dict_sizes[i]: the dictionary of item i as in use.
void CompressGroupsWithDictionaries(const EncoderParams& p, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                    const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                    std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const size_t keys_per_table = (size_t)1 << p.hasher.bucket_bits;
  const size_t tables_max = TablesMax(keys_per_table * 2 + (keys_per_table << p.hasher.block_bits) * 4);
  const Lz77Params P = ChainParams(p);

  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(dict_sizes, sink ? dicts : nullptr), tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    const DictsText staged = StageDictsText(g, dicts, dict_sizes);

    BatchParseJob J = GreedyJob(p, P, g, staged.text);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    J.item_dict_bytes = staged.dict_bytes_dev;
    BuildGroupImages(g, PickGroupImages(g, dicts, dict_sizes), &J);
    if (P.hasher_kind == 9) lz77_batch_parse_h9(J); else lz77_batch_parse_dicts(J);
    FinishOneBlockItems(p, J, g, streams, reference_fails, sink);
    first = g.last;
  }
}

}  // namespace

void BatchGreedyCompressWithDictionaries(const EncoderParams& user, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                         const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                         std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  CompressGroupsWithDictionaries(DictionaryItemParams(user, count ? sizes[0] : 0), count, dicts, dict_sizes, inputs, sizes, streams, reference_fails,
                                 groups, sink);
}

void BatchGreedyCompress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                         std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink) {
  CompressGroups(ItemParams(user, count ? sizes[0] : 0), nullptr, 0, count, inputs, sizes, streams, nullptr, groups, sink);
}

void BatchGreedyCompressWithDictionary(const EncoderParams& user, const uint8_t* dict, size_t dict_size, size_t count,
                                       const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                       std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  CompressGroups(DictionaryItemParams(user, count ? sizes[0] : 0), dict, (uint32_t)dict_size, count, inputs, sizes, streams, reference_fails, groups, sink);
}

namespace {
// BrotliEncoderCompress runs quality 10 at quality 9 (encode.rs:1468-1481; CompressOneShot, cabi.cpp): the parameters of an item
// of either quality are those of quality 9
EncoderParams Q9ItemParams(const EncoderParams& user, size_t input_size) {
  EncoderParams u = user;
  if (u.quality == 10) u.quality = 9;
  return ItemParams(u, input_size);
}
}  // namespace

bool BatchQ9Eligible(const EncoderParams& user, size_t input_size) {
  if (input_size == 0) return false;  // (answered without an encoder)
  // (lgwin <= 16 is hasher 42 in the reference: one by one)
  if ((user.quality != 9 && user.quality != 10) || user.lgwin < 17 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  if (input_size > ((size_t)1 << 18)) return false;  // (lgblock is 18 at most at this quality)
  // one block of a stream that starts at 0: the item ends inside the first half of its ring buffer, 1 << (1 + max(lgwin, lgblock)),
  // so no filed position differs from its ring-buffer index and H9's ring-end case (SearchResult::stored) does not come up
  const EncoderParams p = Q9ItemParams(user, input_size);
  return p.hasher.type == 9 && p.hasher.bucket_bits == 15 && p.hasher.block_bits == 8 && input_size <= ((size_t)1 << p.lgblock);
}

// Qualities 9 and 10, items of one block: the steps of BatchGreedyCompress on H9 tables, parsed by k_parse_batch_h9.
void BatchQ9Compress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                     std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink) {
  // (nothing in the parameters differs between items of at most one block)
  CompressGroups(Q9ItemParams(user, count ? sizes[0] : 0), nullptr, 0, count, inputs, sizes, streams, nullptr, groups, sink);
}

// Quality 9 behind a custom dictionary (batch_q9.h).  D: the dictionary bytes in use, set_custom_dictionary's truncation applied.
// What bounds it: D <= 65536 and input_size <= 65536 give D + input_size <= 131072, the first half of the smallest ring buffer in
// range (1 << (1 + max(lgwin, lgblock)) >= 1 << 18 at lgwin 17).  So no filed position -- the dictionary's, the stitch's, the
// chain's -- differs from its ring-buffer index, nothing is filed masked, and H9's ring-end case (SearchResult::stored,
// lz77_chain.h: br_fold_probe, br_search) stays unreachable: it needs (cur & ring_mask) + best_len > ring_mask, and
// cur + best_len <= D + input_size <= 131072 < ring_mask.  batch_q9_device.h carries the argument on the chain's side.
// (lgwin <= 16 is hasher 42 in the reference, and quality 10 is Zopfli through the stream API: one by one, or the Zopfli route.)
bool BatchQ9DictionaryEligible(const EncoderParams& user, size_t dict_size, size_t input_size) {
  if (input_size == 0 || input_size > 65536 || dict_size < 2) return false;
  if (user.quality != 9 || user.lgwin < 17 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  const size_t D = std::min(dict_size, ((size_t)1 << user.lgwin) - 16);
  if (D > 65536) return false;
  const EncoderParams p = DictionaryItemParams(user, input_size);
  return p.hasher.type == 9 && p.hasher.bucket_bits == 15 && p.hasher.block_bits == 8 && input_size <= ((size_t)1 << p.lgblock) &&
         ComputeRbBits(p) >= 18;
}

// One dictionary that every item names: the steps of BatchGreedyCompressWithDictionary on H9 tables, parsed by k_parse_batch_h9_dict.
void BatchQ9CompressWithDictionary(const EncoderParams& user, const uint8_t* dict, size_t dict_size, size_t count, const uint8_t* const* inputs,
                                   const size_t* sizes, std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails,
                                   uint32_t* groups, const BatchDeviceSink* sink) {
  // (nothing in the parameters differs between items of at most 65536 bytes)
  CompressGroups(DictionaryItemParams(user, count ? sizes[0] : 0), dict, (uint32_t)dict_size, count, inputs, sizes, streams, reference_fails, groups, sink);
}

// A dictionary per item: the steps of BatchGreedyCompressWithDictionaries on H9 tables, parsed by k_parse_batch_h9_dicts.
void BatchQ9CompressWithDictionaries(const EncoderParams& user, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                     const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                     std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  CompressGroupsWithDictionaries(DictionaryItemParams(user, count ? sizes[0] : 0), count, dicts, dict_sizes, inputs, sizes, streams, reference_fails,
                                 groups, sink);
}

// Qualities 5 .. 8, items of two to kBatchLongBlocks blocks: one chain and up to kBatchLongBlocks meta-blocks per item.
void BatchLongCompress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                       std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* demoted, uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  demoted->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = ItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most kBatchLongBytes)
  const size_t keys_per_table = (size_t)1 << p.hasher.bucket_bits;
  const size_t tables_max = TablesMax(keys_per_table * 2 + (keys_per_table << p.hasher.block_bits) * 4);
  const Lz77Params P = ChainParams(p);
  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, 0, tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    const BatchParseJob J = GreedyJob(p, P, g, g.uploaded);  // (J.records is not used, J.dict.bytes is 0)
    BatchLongRecord* records_dev = g.mem.uninit<BatchLongRecord>((size_t)g.n * sizeof(BatchLongRecord));
    lz77_batch_parse_long(J, records_dev);
    FinishLongItems(p, J, records_dev, inputs, g, streams, demoted, sink);
    first = g.last;
  }
}

bool BatchQuickEligible(const EncoderParams& user, size_t input_size) {
  if (input_size == 0) return false;  // (answered without an encoder)
  if (user.quality < 2 || user.quality > 4 || user.lgwin < 10 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  if (input_size > ((size_t)1 << 16)) return false;
  // (the item's size is its stream's size hint: below the 1 MiB that selects H54)
  const EncoderParams p = ItemParams(user, input_size);
  return (p.hasher.type == 2 || p.hasher.type == 3 || p.hasher.type == 4) && input_size <= ((size_t)1 << p.lgblock);
}

// Qualities 2 .. 4 (batch_quick.h), items of one block.  (The plain quick kernel leaves bad_commands at 0: no stream is dropped.)
void BatchQuickCompress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                        std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = ItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  const QuickBatchJob chains = QuickChains(p);
  const size_t tables_max = TablesMax(QuickTableBytes(chains));
  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, 0, tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    QuickBatchJob J = QuickGroupJob(chains, g);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    lz77_quick_batch_parse(J);
    FinishOneBlockItems(p, GatherJobOf(J), g, streams, nullptr, sink);
    first = g.last;
  }
}

bool BatchQuickDictionaryEligible(const EncoderParams& user, size_t dict_size, size_t input_size) {
  if (input_size == 0 || input_size > ((size_t)1 << 16) || dict_size < 2) return false;
  if (user.quality < 2 || user.quality > 4 || user.lgwin < 10 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  // (the reference cuts the dictionary to its last (1 << lgwin) - 16 bytes: dictionary + item stay inside the first lap of the
  // ring buffer, 1 << (1 + max(lgwin, lgblock)), so no filed position differs from its ring-buffer index)
  const EncoderParams p = DictionaryItemParams(user, input_size);
  return (p.hasher.type == 2 || p.hasher.type == 3 || p.hasher.type == 4) && input_size <= ((size_t)1 << p.lgblock) &&
         std::min(dict_size, ((size_t)1 << p.lgwin) - 16) <= ((size_t)1 << 16);
}

// Qualities 2 .. 4 behind a shared custom dictionary (batch_quick.h), items of one block: the steps of BatchQuickCompress with the
// dictionary steps of CompressGroups.  Once per call the dictionary goes up and the table HasherPrependCustomDictionary leaves is
// built on a scratch table (the image: each slot the largest position filed under it, the books 0; a dictionary of 2 .. 7 bytes
// files nothing, but positions still count from its first byte); every chain copies it over its own table.
void BatchQuickCompressWithDictionary(const EncoderParams& user, const uint8_t* dict, size_t dict_use, size_t count,
                                      const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                      std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  if (dict_use < 2 || dict_use > ((size_t)1 << 16)) throw std::runtime_error("brotli_mi355x: a dictionary the quick batch chains do not take");
  const EncoderParams p = DictionaryItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  QuickBatchJob chains = QuickChains(p);  // (no static dictionary behind a custom one: Q.use_dictionary is 0)
  const uint32_t D = (uint32_t)dict_use;
  chains.dict_bytes = D;
  const size_t tables_max = TablesMax(QuickTableBytes(chains));

  DevBlocks call_mem;
  // (shifted so that it ends on a 16-byte boundary, like its copies in the padded text: k_batch_dict_text moves whole words)
  uint8_t* dict_shifted = call_mem.zeroed<uint8_t>((size_t)D + 16 + 64);
  uint8_t* dict_dev = dict_shifted + ((0u - D) & 15u);
  if (sink) batch_copy_device(dict_dev, dict, D); else dev_h2d_bulk(dict_dev, dict, D);  // (the device mode: `dict` is a device address)
  {
    QuickJob image = chains.Q;
    image.table = call_mem.uninit<uint32_t>(QuickTableBytes(chains) + 64);
    lz77_quick_init(image);
    Lz77Buffers B{};
    B.text = dict_dev;  // (every filed position hashes dictionary bytes only)
    lz77_quick_prepend(chains.P, B, image, D);
    chains.image = image.table;
    ++BatchImageTally().images;
  }

  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(D, dict_dev), tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    BatchImageTally().replayed += g.n;
    uint8_t* text = g.dict_text;  // (the device mode: laid out with the staging, from the call's own copy of the dictionary)
    if (!text) {
      text = g.mem.zeroed<uint8_t>(g.padded + 64);
      uint32_t* starts_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
      dev_h2d(starts_dev, A.starts.data(), (size_t)g.n * 4);
      lz77_batch_dict_text(dict_shifted, D, g.uploaded, starts_dev, g.items_dev, g.n, text);
    }
    QuickBatchJob J = QuickGroupJob(chains, g);
    J.text = text;
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    lz77_quick_batch_parse_dict(J);
    // (the gather reads raw commands, whose distance codes the chain took from positions that count the dictionary: it needs no D)
    FinishOneBlockItems(p, GatherJobOf(J), g, streams, reference_fails, sink);
    first = g.last;
  }
}

// Qualities 2 .. 4 behind a dictionary per item (batch_quick.h), items of one block: the steps of BatchQuickCompressWithDictionary
// with the pool step of CompressGroupsWithDictionaries (StageDictsText) in place of the one dictionary, and a table image per
// frequently named dictionary of the group in place of the call's one image -- the chain of an item that names such a dictionary
// copies the image over its table (br_quick_batch_prime), every other chain zeroes its table and files its item's dictionary itself
// (br_quick_batch_file).
void BatchQuickCompressWithDictionaries(const EncoderParams& user, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                        const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                        std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  for (size_t i = 0; i < count; ++i)
    if (dict_sizes[i] < 2 || dict_sizes[i] > ((size_t)1 << 16)) throw std::runtime_error("brotli_mi355x: a dictionary the quick batch chains do not take");
  const EncoderParams p = DictionaryItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  const QuickBatchJob chains = QuickChains(p);  // (no static dictionary behind a custom one: Q.use_dictionary is 0)
  const size_t tables_max = TablesMax(QuickTableBytes(chains));

  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(dict_sizes, sink ? dicts : nullptr), tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    const DictsText staged = StageDictsText(g, dicts, dict_sizes);
    QuickBatchJob J = QuickGroupJob(chains, g);
    J.text = staged.text;
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    J.item_dict_bytes = staged.dict_bytes_dev;
    // an image per frequently named dictionary of the group (PickGroupImages): the table lz77_quick_init + lz77_quick_prepend leave
    // for the dictionary's copy in front of the first item that names it, 256 / 512 KiB each, all built by one launch
    const GroupImages gi = PickGroupImages(g, dicts, dict_sizes);
    J.item_image = CountGroupImages(g, gi);
    if (J.item_image != nullptr) {
      const uint32_t n_images = (uint32_t)gi.first_item.size();
      std::vector<uint32_t> at(2 * (size_t)n_images);  // where each dictionary's copy starts in the text, then its bytes
      for (uint32_t j = 0; j < n_images; ++j) {
        const uint32_t i = gi.first_item[j];
        at[j] = A.items[i].text_off - A.dict_bytes[i];
        at[n_images + j] = A.dict_bytes[i];
      }
      uint32_t* at_dev = g.mem.uninit<uint32_t>(at.size() * 4);
      dev_h2d(at_dev, at.data(), at.size() * 4);
      uint32_t* images = g.mem.zeroed<uint32_t>((size_t)n_images * QuickTableBytes(J) + 64);
      lz77_quick_dict_images(J.Q, staged.text, n_images, at_dev, at_dev + n_images, images);
      J.images = images;
    }
    lz77_quick_batch_parse_dicts(J);
    // (the gather reads raw commands, whose distance codes the chain took from positions that count the dictionary: it needs no D)
    FinishOneBlockItems(p, GatherJobOf(J), g, streams, reference_fails, sink);
    first = g.last;
  }
}

bool BatchQuickLongEligible(const EncoderParams& user, size_t input_size) {
  if (user.quality < 2 || user.quality > 4 || user.lgwin < 10 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  if (input_size > kBatchLongBytes) return false;
  // (four blocks are 64 KiB at quality 2 / 3 and 256 KiB at quality 4: the size hint stays below the 1 MiB that selects H54)
  const EncoderParams p = ItemParams(user, input_size);
  return (p.hasher.type == 2 || p.hasher.type == 3 || p.hasher.type == 4) && input_size > ((size_t)1 << p.lgblock) &&
         input_size <= (size_t)kBatchLongBlocks << p.lgblock;
}

// Qualities 2 .. 4, items of two to kBatchLongBlocks input blocks (batch_quick.h).
void BatchQuickLongCompress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                            std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* demoted, uint32_t* groups,
                            const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  demoted->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = ItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most four blocks)
  const QuickBatchJob chains = QuickChains(p);
  const size_t tables_max = TablesMax(QuickTableBytes(chains));
  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, 0, tables_max, &A, &g, 0, sink != nullptr);
    ++*groups;
    const QuickBatchJob J = QuickGroupJob(chains, g);  // (J.records is not used)
    BatchLongRecord* records_dev = g.mem.uninit<BatchLongRecord>((size_t)g.n * sizeof(BatchLongRecord));
    lz77_quick_batch_parse_long(J, records_dev);
    FinishLongItems(p, GatherJobOf(J), records_dev, inputs, g, streams, demoted, sink);
    first = g.last;
  }
}

bool BatchZopfliEligible(const EncoderParams& user, size_t input_size) {
  if (input_size == 0) return false;  // (answered without an encoder)
  // Quality 11 alone.  An item is what BrotliEncoderCompress gives, and that entry runs quality 10 at quality 9
  // (encode.rs:1468-1481): the stream of plain quality 9 -- bytes a Zopfli walk does not give.  Such items stay one by one.
  if (user.quality != 11 || user.lgwin < 10 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  if (input_size > ((size_t)1 << 16)) return false;  // (at most one input block: lgblock is at least 16 at this quality)
  const EncoderParams p = ItemParams(user, input_size);
  return p.quality == 11 && p.hasher.type == 10 && input_size <= ((size_t)1 << p.lgblock);
}

// Quality 11 (batch_zopfli.h), items of one block: StageGroup, the parse launch on tables sized by the group's largest
// item, FinishOneBlockItems with the quality >= 10 meta-block builder.  A group holds at most kBatchHqGroupItems items (what that
// builder sets aside per meta-block); the tables are as many as stay resident (kZopfliBatchResident) within 8 GiB.
void BatchZopfliCompress(const EncoderParams& user, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                         std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails, uint32_t* groups,
                         const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = ItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  ZopfliBatchJob chains{};
  chains.P = ChainParams(p);
  chains.P.hasher_kind = 6;  // (what Lz77Stage::Setup gives every hasher but H5 and H9; the Zopfli walk does not look at it)
  chains.quality = (uint32_t)p.quality;
  chains.lgwin = (uint32_t)p.lgwin;
  chains.use_dictionary = p.use_dictionary ? 1 : 0;
  chains.dist_alphabet_size = p.dist.alphabet_size;
  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    // (the tables hang on the group's largest item, which the staging finds: staged for the most tables a group can have, then cut)
    StageGroup(first, count, inputs, sizes, 0, kZopfliBatchResident, &A, &g, kBatchHqGroupItems, sink != nullptr);
    ++*groups;
    ZopfliBatchJob J = chains;
    zopfli_batch_layout(&J, A.items[A.order[0]].bytes);
    // (TablesMax: 8 GiB, or BROTLI_MI355X_BATCH_TABLES; more tables than stay resident would only wait for a CU, whoever asks)
    g.tables = (uint32_t)std::min<size_t>(std::min<size_t>(kZopfliBatchResident, TablesMax(J.table_bytes)), g.n);
    J.table_mem = g.mem.uninit<uint8_t>((size_t)g.tables * J.table_bytes + 256);  // (a chain empties its hasher itself; everything else it writes before it reads)
    J.text = g.uploaded;
    J.slabs = g.mem.uninit<Command>(g.cmd_slots * sizeof(Command) + 64);
    J.items = g.items_dev;
    J.order = g.order_dev;
    J.n_items = g.n;
    J.tables = g.tables;
    J.counter = g.mem.zeroed<uint32_t>(64);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    lz77_zopfli_batch_parse(J);
    BatchParseJob G{};  // what the gather wants (GatherJobOf)
    G.P = J.P;
    G.slabs = J.slabs;
    G.items = J.items;
    G.n_items = J.n_items;
    G.records = J.records;
    FinishOneBlockItems(p, G, g, streams, reference_fails, sink);
    first = g.last;
  }
}

bool BatchZopfliDictionaryEligible(const EncoderParams& user, size_t dict_size, size_t input_size) {
  if (input_size == 0 || input_size > ((size_t)1 << 16) || dict_size < 2) return false;
  // (both qualities: through the stream API, which defines these items, quality 10 is a Zopfli walk as well)
  if ((user.quality != 10 && user.quality != 11) || user.lgwin < 10 || user.lgwin > 24 || !PlainStreamParams(user)) return false;
  // (dictionary in use + item stay inside the first lap of the ring buffer, 1 << (1 + max(lgwin, lgblock)), lgblock >= 16)
  const EncoderParams p = DictionaryItemParams(user, input_size);
  return p.hasher.type == 10 && input_size <= ((size_t)1 << p.lgblock) && std::min(dict_size, ((size_t)1 << p.lgwin) - 16) <= ((size_t)1 << 16);
}

// Qualities 10 and 11 behind a dictionary per item (batch_zopfli.h), items of one block: the steps of BatchZopfliCompress with the
// pool step of CompressGroupsWithDictionaries (StageDictsText).  No tree image per dictionary: every chain empties its hasher and
// files its item's dictionary itself (br_zopfli_batch_prepend).  (A call in which every item names ONE dictionary has an image:
// BatchZopfliCompressWithDictionary below.)
void BatchZopfliCompressWithDictionaries(const EncoderParams& user, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                         const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                         std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = DictionaryItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  for (size_t i = 0; i < count; ++i)
    if (dict_sizes[i] < 2 || dict_sizes[i] > ((size_t)1 << 16) || dict_sizes[i] > ((size_t)1 << p.lgwin) - 16)
      throw std::runtime_error("brotli_mi355x: a dictionary the Zopfli batch chains do not take");
  // the measured alternative of the wave-wide prepend (profiles/r27_batch_dictionaries_zopfli.json), read once per process
  static const bool prepend_lane0 = EnvSize("BROTLI_MI355X_ZOPFLI_PREPEND_LANE0", 0) != 0;
  ZopfliBatchJob chains{};
  chains.P = ChainParams(p);
  chains.P.hasher_kind = 6;  // (as BatchZopfliCompress)
  chains.quality = (uint32_t)p.quality;
  chains.lgwin = (uint32_t)p.lgwin;
  chains.use_dictionary = 0;  // (no static dictionary behind a custom one)
  chains.dist_alphabet_size = p.dist.alphabet_size;
  chains.prepend_lane0 = prepend_lane0 ? 1 : 0;
  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(dict_sizes, sink ? dicts : nullptr), kZopfliBatchResident, &A, &g, kBatchHqGroupItems, sink != nullptr);
    ++*groups;
    const DictsText staged = StageDictsText(g, dicts, dict_sizes);
    BatchImageTally().filed += g.n;  // (no image per dictionary on this route: its image is a tree forest with its own builder)
    // (the order is by dictionary + item, which sizes the forest; everything else hangs on the largest item)
    uint32_t largest_item = 0;
    for (uint32_t i = 0; i < g.n; ++i) largest_item = std::max(largest_item, A.items[i].bytes);
    ZopfliBatchJob J = chains;
    zopfli_batch_layout(&J, largest_item, A.dict_bytes[A.order[0]] + A.items[A.order[0]].bytes);
    g.tables = (uint32_t)std::min<size_t>(std::min<size_t>(kZopfliBatchResident, TablesMax(J.table_bytes)), g.n);
    J.table_mem = g.mem.uninit<uint8_t>((size_t)g.tables * J.table_bytes + 256);
    J.text = staged.text;
    J.item_dict_bytes = staged.dict_bytes_dev;
    J.slabs = g.mem.uninit<Command>(g.cmd_slots * sizeof(Command) + 64);
    J.items = g.items_dev;
    J.order = g.order_dev;
    J.n_items = g.n;
    J.tables = g.tables;
    J.counter = g.mem.zeroed<uint32_t>(64);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    lz77_zopfli_batch_parse_dicts(J);
    BatchParseJob G{};  // what the gather wants (GatherJobOf); the raw commands carry distances, so it needs no D
    G.P = J.P;
    G.slabs = J.slabs;
    G.items = J.items;
    G.n_items = J.n_items;
    G.records = J.records;
    FinishOneBlockItems(p, G, g, streams, reference_fails, sink);
    first = g.last;
  }
}

// Qualities 10 and 11 behind ONE dictionary that every item names (batch_zopfli.h), items of one block: the steps above with the
// dictionary steps of CompressGroups.  Once per call the dictionary goes up (the device mode: one device copy) and its tree image
// is built in call-scoped memory (lz77_zopfli_dict_image: the buckets and at most 8 << 16 bytes of forest, 1 MiB in all); a group
// stages dictionary | item per item as the shared routes of the other qualities do, and every chain replays the image
// (k_zopfli_batch_dict).  Groups, tables and the forest's size are those of BatchZopfliCompressWithDictionaries.
void BatchZopfliCompressWithDictionary(const EncoderParams& user, const uint8_t* dict, size_t dict_use, size_t count, const uint8_t* const* inputs,
                                       const size_t* sizes, std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails,
                                       uint32_t* groups, const BatchDeviceSink* sink) {
  streams->assign(count, std::vector<uint8_t>());
  reference_fails->assign(count, 0);
  *groups = 0;
  if (count == 0) return;
  const EncoderParams p = DictionaryItemParams(user, sizes[0]);  // (nothing in the parameters differs between items of at most one block)
  if (dict_use < 2 || dict_use > ((size_t)1 << 16) || dict_use > ((size_t)1 << p.lgwin) - 16)
    throw std::runtime_error("brotli_mi355x: a dictionary the Zopfli batch chains do not take");
  const uint32_t D = (uint32_t)dict_use;
  // measurement only (DESIGN.md section 10): no image, every chain files the dictionary itself (k_zopfli_batch_dicts)
  static const bool self_file = EnvSize("BROTLI_MI355X_BATCH_DICT_SELF_FILE", 0) != 0;
  static const bool prepend_lane0 = EnvSize("BROTLI_MI355X_ZOPFLI_PREPEND_LANE0", 0) != 0;
  ZopfliBatchJob chains{};
  chains.P = ChainParams(p);
  chains.P.hasher_kind = 6;  // (as BatchZopfliCompress)
  chains.quality = (uint32_t)p.quality;
  chains.lgwin = (uint32_t)p.lgwin;
  chains.use_dictionary = 0;  // (no static dictionary behind a custom one)
  chains.dist_alphabet_size = p.dist.alphabet_size;
  chains.prepend_lane0 = prepend_lane0 ? 1 : 0;
  chains.dict_bytes = D;

  DevBlocks call_mem;
  // (shifted so that it ends on a 16-byte boundary, like its copies in the padded text: k_batch_dict_text moves whole words)
  uint8_t* dict_shifted = call_mem.zeroed<uint8_t>((size_t)D + 16 + 64);
  uint8_t* dict_dev = dict_shifted + ((0u - D) & 15u);
  if (sink) batch_copy_device(dict_dev, dict, D); else dev_h2d_bulk(dict_dev, dict, D);  // (the device mode: `dict` is a device address)
  if (!self_file) {
    uint16_t* classes = call_mem.uninit<uint16_t>((size_t)zopfli_dict_image_class_entries(D) * 2 + 64);
    uint32_t* image_buckets = call_mem.uninit<uint32_t>(((size_t)4 << 17) + 64);
    uint32_t* image_forest = call_mem.uninit<uint32_t>((size_t)8 * zopfli_dict_image_slots(D, chains.lgwin) + 64);
    lz77_zopfli_dict_image(dict_dev, D, chains.lgwin, classes, image_buckets, image_forest);
    chains.image_buckets = image_buckets;
    chains.image_forest = image_forest;
    ++BatchImageTally().images;
  }

  CallArrays A;
  size_t first = 0;
  while (first < count) {
    Group g;
    StageGroup(first, count, inputs, sizes, DictSizes(D, dict_dev), kZopfliBatchResident, &A, &g, kBatchHqGroupItems, sink != nullptr);
    ++*groups;
    (self_file ? BatchImageTally().filed : BatchImageTally().replayed) += g.n;
    uint8_t* text = g.dict_text;  // (the device mode: laid out with the staging, from the call's own copy of the dictionary)
    if (!text) {
      text = g.mem.zeroed<uint8_t>(g.padded + 64);
      uint32_t* starts_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
      dev_h2d(starts_dev, A.starts.data(), (size_t)g.n * 4);
      lz77_batch_dict_text(dict_shifted, D, g.uploaded, starts_dev, g.items_dev, g.n, text);
    }
    ZopfliBatchJob J = chains;
    const uint32_t largest_item = A.items[A.order[0]].bytes;  // (behind one dictionary the order by dictionary + item is the order by item)
    zopfli_batch_layout(&J, largest_item, D + largest_item);
    g.tables = (uint32_t)std::min<size_t>(std::min<size_t>(kZopfliBatchResident, TablesMax(J.table_bytes)), g.n);
    J.table_mem = g.mem.uninit<uint8_t>((size_t)g.tables * J.table_bytes + 256);
    J.text = text;
    J.slabs = g.mem.uninit<Command>(g.cmd_slots * sizeof(Command) + 64);
    J.items = g.items_dev;
    J.order = g.order_dev;
    J.n_items = g.n;
    J.tables = g.tables;
    J.counter = g.mem.zeroed<uint32_t>(64);
    J.records = g.mem.uninit<BatchRecord>((size_t)g.n * sizeof(BatchRecord));
    if (self_file) {
      uint32_t* dict_bytes_dev = g.dict_bytes_dev;  // (the device mode: StageGroup has sent A.dict_bytes up)
      if (!dict_bytes_dev) {
        dict_bytes_dev = g.mem.uninit<uint32_t>((size_t)g.n * 4);
        dev_h2d(dict_bytes_dev, A.dict_bytes.data(), (size_t)g.n * 4);
      }
      J.item_dict_bytes = dict_bytes_dev;
      lz77_zopfli_batch_parse_dicts(J);
    } else {
      lz77_zopfli_batch_parse_dict(J);
    }
    BatchParseJob G{};  // what the gather wants (GatherJobOf); the raw commands carry distances, so it needs no D
    G.P = J.P;
    G.slabs = J.slabs;
    G.items = J.items;
    G.n_items = J.n_items;
    G.records = J.records;
    FinishOneBlockItems(p, G, g, streams, reference_fails, sink);
    first = g.last;
  }
}

size_t StoredStreamToDevice(const uint8_t* input_dev, size_t input_size, uint8_t* output_dev) {
  size_t size = input_size, result = 0, offset = 0;
  if (input_size == 0) {
    const uint8_t empty = 6;
    dev_h2d(output_dev, &empty, 1);
    return 1;
  }
  const uint8_t window[2] = {0x21, 0x03};
  dev_h2d(output_dev, window, 2);
  result = 2;
  while (size > 0) {
    uint32_t nibbles = 0;
    const uint32_t chunk_size = size > (1u << 24) ? (1u << 24) : (uint32_t)size;
    if (chunk_size > (1u << 16)) nibbles = chunk_size > (1u << 20) ? 2 : 1;
    const uint32_t bits = (nibbles << 1) | ((chunk_size - 1) << 3) | (1u << (19 + 4 * nibbles));
    const uint8_t header[4] = {(uint8_t)bits, (uint8_t)(bits >> 8), (uint8_t)(bits >> 16), (uint8_t)(bits >> 24)};
    const size_t header_bytes = nibbles == 2 ? 4 : 3;
    dev_h2d(output_dev + result, header, header_bytes);
    result += header_bytes;
    dev_d2d(output_dev + result, input_dev + offset, chunk_size);
    result += chunk_size;
    offset += chunk_size;
    size -= chunk_size;
  }
  const uint8_t last = 3;
  dev_h2d(output_dev + result, &last, 1);
  return result + 1;
}

}  // namespace brotli_mi355x
