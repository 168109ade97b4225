// batch_zopfli.h -- the small items of a batch at quality 11, side by side on the device (BrotliMi355xCompressBatchEx with
// BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS).
//
// (Quality 11 alone: BrotliEncoderCompress, which defines an item's bytes, runs quality 10 at quality 9 -- encode.rs:1468-1481:
// the stream is byte for byte that of plain quality 9 -- and a Zopfli walk does not give those bytes.  Items of quality 10 are not this route's: they go
// one by one, or side by side as quality 9 under BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS, batch_greedy.h.)
// An item of at most 65 536 bytes -- at most one input block, lgblock is at least 16 at this quality -- is ONE sequential walk of
// br_zopfli_parse (zopfli_device.h, precomputed = false: matching, tree updates and the dynamic programme position by position, the
// reference's way) on H10 trees of its own, and ONE meta-block.  The sequential form handles the positions skipped behind a match
// beyond the Zopfli length exactly, so nothing is speculated, backed up or repeated.  A group shares the
// plan of the other routes (batch_greedy.h): one padded text buffer, one parse launch (k_zopfli_batch: one wavefront per table, each
// emptying its hasher in front of every item), the per-item records, the command gather (lz77_batch_gather: the raw commands are
// those of qualities 5 .. 8) and one pass of the meta-block stage with the quality >= 10 builder.  No key pass, no dictionary.
//
// Memory of a table, sized by the group's largest item rounded up to 64 bytes (cap), every part on a 256-byte boundary:
//   buckets        4 << 17                         (512 KiB)
//   forest         8 * min(cap, 1 << lgwin)        only the slots 2 * (pos & window mask) of the item's positions are touched
//                  (behind a dictionary per item: 8 * min(largest dictionary + item rounded up to 64, 1 << lgwin))
//   nodes          20 * (cap + 2)
//   literal costs  4 * (cap + 4)
//   cost tables    4 * (dist alphabet + 64) + 4 * 704, histograms 4 * 2048
//   matches        8 * (128 * cap + 256) (the reference's bound of 128 per position, and room for the static-dictionary matches the
//                  last position adds behind 128 tree matches)
//   match counts   4 * cap,  first-pass commands 16 * (cap / 2 + 8),  control words 64 + 256
// which is 4.7 MiB for items of 4 KiB and 66 MiB for items of 64 KiB.  The
// number of tables is min(items of the group, 8 GiB / table bytes, kZopfliBatchResident); BROTLI_MI355X_BATCH_TABLES stands in for
// the 8 GiB term (TablesMax).
#ifndef BROTLI_MI355X_BATCH_ZOPFLI_H_
#define BROTLI_MI355X_BATCH_ZOPFLI_H_

#include <stddef.h>
#include <stdint.h>

#include "batch_greedy.h"
#include "metablock_types.h"

namespace brotli_mi355x {

// The parse kernel keeps a node window of 104 KiB in workgroup memory: one workgroup per CU, 256 CUs.  More tables than that
// would only wait for a CU.
static constexpr uint32_t kZopfliBatchResident = 256;

// (A group of the route holds at most kBatchHqGroupItems items, metablock_types.h: the bound of the quality >= 10 meta-block builder.)

// ---- device seam (batch_zopfli_kernels.hip; the emulation build: batch_zopfli_emu.inc)
struct ZopfliBatchJob {
  Lz77Params P;  // of a stream that starts at 0 and stays inside the first ring-buffer revolution (ChainParams)
  uint32_t quality;  // 11
  uint32_t lgwin;
  uint32_t use_dictionary;
  uint32_t dist_alphabet_size;
  const uint8_t* text;  // the group's padded text: every item at a 64-byte boundary, at least 64 zero bytes behind it
  Command* slabs;
  const BatchItem* items;
  const uint32_t* order;  // largest item first
  uint32_t n_items;
  uint32_t tables;
  uint32_t* counter;  // [1], zero: the next place of `order` to hand out
  BatchRecord* records;
  uint8_t* table_mem;  // [tables][table_bytes], 256-byte aligned
  // a dictionary per item (k_zopfli_batch_dicts): `text` is the staged text, dictionary | item per item, and item i's dictionary
  // is the item_dict_bytes[i] bytes that end where the item starts.  nullptr: no dictionaries (k_zopfli_batch)
  const uint32_t* item_dict_bytes;  // [n_items], device
  uint32_t prepend_lane0;           // the dictionary goes into the trees on lane 0 alone (the measured alternative), not wave-wide
  // one dictionary that every item names (k_zopfli_batch_dict): `text` is staged the same way, every item behind the dict_bytes
  // bytes of the call's dictionary, and a chain replays the call's tree image (lz77_zopfli_dict_image) instead of filing them
  const uint32_t* image_buckets;  // [1 << 17]
  const uint32_t* image_forest;   // [2 * zopfli_dict_image_slots(dict_bytes, lgwin)], 16-byte aligned
  uint32_t dict_bytes;
  // the layout of a table (zopfli_batch_layout): byte offsets, multiples of 256
  uint32_t cap;   // the group's largest item rounded up to 64
  uint32_t span;  // the positions the forest has slots for: the group's largest dictionary + item rounded up to 64, at most 1 << lgwin
  size_t table_bytes;
  size_t off_forest, off_nodes, off_literal_costs, off_cost_dist, off_cost_cmd, off_histo, off_matches, off_num_matches, off_tmp_cmds,
      off_ctl, off_exit;
};
// fills in cap, span, the offsets and table_bytes from lgwin, dist_alphabet_size and the largest item of the group.  largest_text:
// the group's largest dictionary + item where the items lie behind dictionaries of their own -- the forest alone grows with it,
// everything else is indexed by the position inside the item; 0: no dictionaries, the largest item.
inline void zopfli_batch_layout(ZopfliBatchJob* J, uint32_t largest_item, uint32_t largest_text = 0) {
  const size_t cap = ((size_t)largest_item + 63) & ~(size_t)63;
  const size_t window = (size_t)1 << J->lgwin;
  const size_t text = largest_text ? ((size_t)largest_text + 63) & ~(size_t)63 : cap;
  const size_t span = text < window ? text : window;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) & ~(size_t)255;
    return here;
  };
  J->cap = (uint32_t)cap;
  J->span = (uint32_t)span;
  take((size_t)4 << 17);  // buckets, at 0
  J->off_forest = take(8 * span);
  J->off_nodes = take(20 * (cap + 2));
  J->off_literal_costs = take(4 * (cap + 4));
  J->off_cost_dist = take(4 * ((size_t)J->dist_alphabet_size + 64));
  J->off_cost_cmd = take(4 * 704);
  J->off_histo = take(4 * 2048);
  J->off_matches = take(8 * (128 * cap + 256));
  J->off_num_matches = take(4 * cap);
  J->off_tmp_cmds = take(16 * (cap / 2 + 8));
  J->off_ctl = take(64);
  J->off_exit = take(256);
  J->table_bytes = at;
}
// one wavefront per table; a wavefront takes items from `counter` until none is left.  BatchRecord::bad_commands flags the items
// the reference encoder panics on (kZopfliReferencePanics).  The gather is lz77_batch_gather.
void lz77_zopfli_batch_parse(const ZopfliBatchJob& J);
// ... behind a dictionary per item (J.item_dict_bytes): every chain empties its hasher, files its item's dictionary wave-wide
// (br_zopfli_batch_prepend), stitches and walks the item from position D
void lz77_zopfli_batch_parse_dicts(const ZopfliBatchJob& J);
// ... behind the one dictionary of the call (J.dict_bytes, J.image_buckets, J.image_forest): every chain copies the image over
// its buckets and the dictionary's part of its forest (br_zopfli_batch_replay), stitches and walks the item from position D
void lz77_zopfli_batch_parse_dict(const ZopfliBatchJob& J);

// The tree image of a dictionary of D bytes in use at `lgwin`: what br_zopfli_batch_reset(B, lgwin, D) and the prepend of the D
// bytes leave in the buckets and in the forest slots of the positions below D rounded up to 64 (at most 1 << lgwin).  It hangs on
// the dictionary alone -- a Store of position i, i + 127 < D, compares at most 128 bytes, all of them the dictionary's -- so one
// image serves every item of a call.
constexpr uint32_t zopfli_dict_image_slots(uint32_t D, uint32_t lgwin) {
  const uint32_t rounded = (D + 63u) & ~63u;
  return rounded < (1u << lgwin) ? rounded : (1u << lgwin);
}
// the positions the prepend stores: [0, D - 127)
constexpr uint32_t zopfli_dict_image_stored(uint32_t D) { return D >= 128u ? D - 127u : 0u; }
// entries of the class array the build writes in front of its stores (zopfli_dict_image_stored rounded up to 16)
constexpr uint32_t zopfli_dict_image_class_entries(uint32_t D) { return (zopfli_dict_image_stored(D) + 15u) & ~15u; }
// dict: the D bytes, the 4-byte loads of the stored positions end inside them; classes: [zopfli_dict_image_class_entries(D)],
// scratch; buckets: [1 << 17]; forest: [2 * zopfli_dict_image_slots(D, lgwin)], 16-byte aligned.  All device memory, all written
// here: a fill launch (every bucket the invalid position, the forest 0), the class of every stored position, and the store launch
// in which lanes that own disjoint classes of hash keys file their positions in ascending order.  D <= (1 << lgwin) - 16.
void lz77_zopfli_dict_image(const uint8_t* dict, uint32_t D, uint32_t lgwin, uint16_t* classes, uint32_t* buckets, uint32_t* forest);

// ---- host
// Does this item go side by side under the Zopfli route?  `params`: the caller's parameters as set, not finalized.
bool BatchZopfliEligible(const EncoderParams& params, size_t input_size);
// The streams of `count` eligible items.  Throws std::runtime_error on a device error.  *groups: device groups run.
// (*reference_fails)[i] != 0: the reference itself fails on item i; its stream stays empty.
void BatchZopfliCompress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                         std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails, uint32_t* groups,
                         const BatchDeviceSink* sink = nullptr);

// BrotliMi355xCompressBatchWithDictionaries under BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS: qualities 10 AND 11 -- an
// item is the stream of BrotliEncoderSetCustomDictionary + one FINISH, and the stream API runs both as Zopfli.  Does this item go
// side by side?  dict_size: the dictionary as handed in (the reference cuts it to its last (1 << lgwin) - 16 bytes).
bool BatchZopfliDictionaryEligible(const EncoderParams& params, size_t dict_size, size_t input_size);
// The streams of `count` eligible items; dicts[i] / dict_sizes[i]: the dictionary of item i as in use.  A table's forest is sized
// by the group's largest dictionary + item (8 bytes per position, at most 8 << lgwin), everything else as above.
void BatchZopfliCompressWithDictionaries(const EncoderParams& params, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                         const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                         std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// ... behind ONE dictionary that every item names (dict / dict_size: as in use): the dictionary goes up once and its tree image is
// built once per call; every chain replays it.  BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 (measurement): no image, every chain files
// the dictionary itself, as behind a dictionary per item.
void BatchZopfliCompressWithDictionary(const EncoderParams& params, const uint8_t* dict, size_t dict_size, size_t count, const uint8_t* const* inputs,
                                       const size_t* sizes, std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* reference_fails,
                                       uint32_t* groups, const BatchDeviceSink* sink = nullptr);

}  // namespace brotli_mi355x
#endif
