// batch_greedy.h -- the small items of a batch at qualities 5 .. 8, side by side on the device (BrotliMi355xCompressBatch).
//
// An item of at most one input block (1 << lgblock bytes) under an H5 hasher is ONE live chain (lz77_live.h) and ONE meta-block:
// it starts on empty bucket rings, so the chain is exact on its own stores and nothing is speculated, verified or repeated.
// A group of such items shares one text buffer (every item at a 64-byte boundary, at least 64 zero bytes behind it), one key
// pass, one parse launch (k_parse_batch: one wavefront per item, each on a private table that it zeroes itself), one command
// gather and one pass of the meta-block stage with one meta-block per item.  The streams come out of the same kernels as those
// of the one-shot call, item by item the bytes BrotliEncoderCompress gives.
//
// With a shared custom dictionary (BrotliMi355xCompressBatchWithDictionary) an item is the stream of an encoder whose hasher
// HasherPrependCustomDictionary (encode.rs:1163-1194) has primed: its text is `dictionary | item`, laid out on the device with the
// dictionary's end abutting the item's first byte, and its chain starts on a table that already holds the dictionary.  What the
// prepend leaves in the rings hangs on the dictionary and the hasher parameters alone, so it is built once per call (BatchDictImage:
// the ring counters, and the list of (slot, position) the counters still cover) and replayed by every chain with independent stores.
#ifndef BROTLI_MI355X_BATCH_GREEDY_H_
#define BROTLI_MI355X_BATCH_GREEDY_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "encoder_params.h"
#include "lz77_types.h"

namespace brotli_mi355x {

// ---- device seam (lz77_kernels.hip; the emulation build: batch_greedy_emu.inc)
struct BatchItem {
  uint32_t text_off;  // where the item starts in the group's padded text (a multiple of 64)
  uint32_t bytes;     // 1 .. 1 << lgblock
  uint32_t cmd_base;  // its command slab
  uint32_t cmd_cap;
};
// What the chain leaves per item: Lz77Stage::Resolve for a stream of one block.
struct BatchRecord {
  uint32_t n_cmds;        // commands of the meta-block, the trailing insert-only one included
  uint32_t n_lits;        // literals, the trailing ones included
  uint32_t trailing;      // literals of the trailing insert-only command (0: there is none)
  uint32_t uncompressed;  // should_compress (encode.rs:1325-1354) said no
  uint32_t overflow;      // the slab was too small (cannot happen: a copy is at least two bytes long)
  uint32_t bad_commands;  // SegExit::bad_commands (a match cut to one byte at the dictionary end): the reference fails on this item;
                          // the record then describes the item as one insert-only command, stored, so that the gather and the
                          // meta-block stage never see the copy (its stream is dropped by the host)
  uint32_t pad[2];
};
// What HasherPrependCustomDictionary leaves in an H5 table, in a form a chain can replay without a dependent chain of stores.
struct BatchDictImage {
  uint32_t bytes;           // D: dictionary bytes in use (0: no dictionary); an item parses [D, D + its bytes) of its own text
  const uint16_t* num;      // [1 << bucket_bits]: the ring counters behind the prepend
  const uint32_t* entries;  // [2 * *n_entries]: (slot in `buckets`, position) of every entry the counters still cover;
                            // nullptr: no image, every chain files the dictionary itself (measurement only)
  const uint32_t* n_entries;  // [1], on the device: at most D
};
struct BatchParseJob {
  Lz77Params P;  // of a stream that starts at 0; total_bytes is the item's and set per item
  const uint8_t* text;
  const uint16_t* keys;
  uint8_t* flags;
  Command* slabs;
  const BatchItem* items;
  const uint32_t* order;  // largest item first
  uint32_t n_items;
  uint32_t tables;
  uint16_t* num;      // [tables][1 << bucket_bits]
  uint32_t* buckets;  // [tables][(1 << bucket_bits) << block_bits]
  uint32_t* counter;  // [1], zero: the next place of `order` to hand out
  BatchRecord* records;
  BatchDictImage dict;  // bytes == 0: the plain call
  // a dictionary per item (BrotliMi355xCompressBatchWithDictionaries, lz77_batch_parse_dicts): [n_items], the dictionary bytes in
  // front of item i, 2 .. 65536; nullptr: every other caller.
  const uint32_t* item_dict_bytes;
  // ... and the images of the group's frequently named dictionaries (lz77_batch_dict_images): item i's chain replays
  // images[item_image[i]], or files its dictionary itself where item_image[i] is kBatchNoImage.  item_image == nullptr: no images,
  // every chain files.  Read by the instances of a dictionary per item alone.
  const BatchDictImage* images;  // [n_images], device
  const uint32_t* item_image;    // [n_items], device
};
static constexpr uint32_t kBatchNoImage = 0xffffffffu;
static constexpr uint32_t kBatchGroupImages = 64;  // images per group at most
// one wavefront per table; a wavefront takes items from `counter` until none is left
void lz77_batch_parse(const BatchParseJob& J);
// The same launch shape for the H9 hasher of qualities 9 and 10 (batch_q9_kernels.hip: k_parse_batch_h9).  J.P is that of an H9
// chain (hasher_kind 9, bucket_bits 15, block_bits 8, ndist 16), J.keys the H9 keys, J.dict.bytes is 0.
void lz77_batch_parse_h9(const BatchParseJob& J);
// Items of several blocks.  A meta-block of an item: a whole number of input blocks (the item's last one may be short).
static constexpr uint32_t kBatchLongBlocks = 4;  // input blocks per item at most, hence meta-blocks
static constexpr uint32_t kBatchLongBytes = 262144;
struct BatchLongMetaBlock {
  uint32_t start, bytes;  // item-local text range
  uint32_t first_cmd;     // in the item's slab, from cmd_base: its raw commands lie contiguous, in text order
  uint32_t n_cmds;        // raw commands (the trailing insert-only command is not in the slab)
  uint32_t n_lits;        // literals, the trailing ones included
  uint32_t trailing;      // literals of the trailing insert-only command (0: there is none)
  uint32_t uncompressed;  // should_compress said no
  uint32_t pad;
};
struct BatchLongRecord {
  uint32_t n_mb;          // 1 .. kBatchLongBlocks
  uint32_t overflow;      // the slab was too small (cannot happen: a copy is at least two bytes long); the chain stopped there
  uint32_t bad_commands;  // always 0 (no dictionary end to cut a match at)
  uint32_t pad;
  BatchLongMetaBlock mb[kBatchLongBlocks];
};
// the same launch shape as lz77_batch_parse; J.records is not used, J.dict.bytes is 0, every item has kBatchLongBytes at most
void lz77_batch_parse_long(const BatchParseJob& J, BatchLongRecord* records);
// out[offsets[kBatchLongBlocks * i + m] ..) = the finished commands of meta-block m of item i and its trailing insert-only command
void lz77_batch_gather_long(const BatchParseJob& J, const BatchLongRecord* records, const uint32_t* offsets_dev, Command* out);
// The dictionary path.  lz77_batch_dict_text: text[items[i].text_off - dict_bytes ..) = dictionary | item i (packed + starts[i]) for
// every item; `text` is zero where nothing is written, text_off is a multiple of 64 and at least dict_bytes rounded up to 16.
// dict_shifted_dev: 16-byte aligned, (-dict_bytes & 15) zero bytes and then the dictionary, so that it ends on a 16-byte boundary.
void lz77_batch_dict_text(const uint8_t* dict_shifted_dev, uint32_t dict_bytes, const uint8_t* packed_dev, const uint32_t* starts_dev,
                          const BatchItem* items_dev, uint32_t n_items, uint8_t* text);
// A dictionary per item.  lz77_batch_dicts_text: text[items[i].text_off - dict_bytes[i] ..) = dictionary i | item i for every item,
// the dictionary's dict_bytes[i] bytes read from pool_dev + dict_off[i]; `text` is zero where nothing is written, text_off is a multiple
// of 64 and at least dict_bytes[i] rounded up to 16.  pool_dev: 16-byte aligned, every dictionary in it ENDS on a 16-byte boundary (the
// dict_shifted convention: dict_off[i] + dict_bytes[i] is a multiple of 16) behind at least 15 bytes that may be read.
void lz77_batch_dicts_text(const uint8_t* pool_dev, const uint32_t* dict_off_dev, const uint32_t* dict_bytes_dev, const uint8_t* packed_dev,
                           const uint32_t* starts_dev, const BatchItem* items_dev, uint32_t n_items, uint8_t* text);
// the launch shape of lz77_batch_parse for J.item_dict_bytes != nullptr (J.dict is not used): k_parse_batch_dicts
void lz77_batch_parse_dicts(const BatchParseJob& J);
// lz77_batch_dict_image: files the positions [0, dict_bytes - 3) of a text whose keys are `keys` on the scratch table (num, buckets)
// -- `num` ends up as the image's counters -- and lists the covered entries: entries[2 * i], entries[2 * i + 1], *n_entries.
void lz77_batch_dict_image(const Lz77Params& P, const uint16_t* keys, uint32_t dict_bytes, uint16_t* num, uint32_t* buckets,
                           uint32_t* entries, uint32_t* n_entries);
// The images of a group behind a dictionary per item, built in the group's own arrays.  Image j is that of the dictionary whose
// plan[j].bytes bytes start at text position plan[j].text_at (its copy in front of the first item that names it; J.keys holds the
// keys of that copy, and the filed positions [0, bytes - 3) hash dictionary bytes only).  One wavefront per image files them on
// table j % J.tables of the job -- the parse launch behind it empties or overwrites every counter of a table in front of every item,
// so the tables serve as the scratch -- and one listing launch with an image dimension copies the counters to num[j] and lists the
// covered entries from entries[2 * plan[j].entries_at] on, n_entries[j] of them.  More images than tables: rounds of J.tables images.
// plan: [n_images], device; num: [n_images][1 << bucket_bits]; entries: room for two words per dictionary byte of all images;
// n_entries: [n_images], zeroed by the caller.  A dictionary shorter than the hashed length gives an image with zero entries and
// zero counters.  What a chain replays is BatchDictImage{bytes, num + j << bucket_bits, entries + 2 * entries_at, n_entries + j}.
struct BatchImagePlan {
  uint32_t text_at;     // where the dictionary's copy starts in the group's padded text
  uint32_t bytes;       // D
  uint32_t entries_at;  // its list starts at entry entries_at of `entries`; it has room for `bytes` entries
  uint32_t pad;
};
void lz77_batch_dict_images(const BatchParseJob& J, uint32_t n_images, const BatchImagePlan* plan_dev, uint16_t* num, uint32_t* entries,
                            uint32_t* n_entries);
// out[offsets[i] ..) = the finished commands of item i (Command::init) and its trailing insert-only command
void lz77_batch_gather(const BatchParseJob& J, const uint32_t* offsets_dev, Command* out);

// ---- host
// What encoder_compress does with the stream its encoder made (encode.rs:1521-1538), decided from sizes alone: the stream goes out
// if it fits the buffer and is no larger than BrotliEncoderMaxCompressedSize; otherwise the input goes out as a stored stream if
// the buffer holds BrotliEncoderMaxCompressedSize bytes; otherwise the item fails.  One copy for every sink: the host buffers of
// the batch and one-shot calls (cabi.cpp: OneShotDeliver) and the device buffers of BrotliMi355xCompressBatchDevice.
enum class Delivery { kStream, kStored, kFails };
inline Delivery DeliveryRule(size_t stream_size, size_t input_size, size_t capacity) {
  const size_t max_out_size = MaxCompressedSize(input_size);
  if (stream_size <= capacity && !(max_out_size != 0 && stream_size > max_out_size)) return Delivery::kStream;
  return (max_out_size != 0 && capacity >= max_out_size) ? Delivery::kStored : Delivery::kFails;
}
// What the stream API owes a caller who offers `capacity` bytes for a finished stream (the dictionary batch calls: item i is
// BrotliEncoderSetCustomDictionary + one FINISH): the stream goes out if and only if it fits.  There is no stored stream to fall
// back to and no BrotliEncoderMaxCompressedSize to hold it against; input_size is not looked at.  The same signature as
// DeliveryRule, so that a sink names the one its call is owed.
inline Delivery StreamDeliveryRule(size_t stream_size, size_t /*input_size*/, size_t capacity) {
  return stream_size <= capacity ? Delivery::kStream : Delivery::kFails;
}
// The device mode of the Batch*Compress calls below (BrotliMi355xCompressBatchDevice, BrotliMi355xCompressBatchWithDictionariesDevice):
// inputs[i] is a device address, the group's items come out of device memory (batch_device.h: batch_stage_device,
// batch_stage_dicts_device) and its output stays there; no stream comes to the host (`streams` stays empty).  Every item the route
// answers -- all but the demoted ones and those the reference fails on -- gets sizes[i] and results[i] by `rule`, and its stream,
// or the stored stream of its input, at outputs[i].
struct BatchDeviceSink {
  uint8_t* const* outputs;   // [count] device addresses, any alignment
  const size_t* capacities;  // [count]
  size_t* sizes;             // [count], result
  int32_t* results;          // [count], result: 1 = the item's stream lies at outputs[i], 0 = it fails alone
  Delivery (*rule)(size_t stream_size, size_t input_size, size_t capacity) = DeliveryRule;  // the dictionary calls: StreamDeliveryRule
};
// MakeUncompressedStream (encode.rs:1388-1433) for an input that lies on the device: the header bytes go down with dev_h2d and the
// body with dev_d2d, one pair per chunk of at most 1 << 24 bytes, and the final byte 3.  Returns the stream's size; the caller's
// buffer holds BrotliEncoderMaxCompressedSize(input_size) bytes.
size_t StoredStreamToDevice(const uint8_t* input_dev, size_t input_size, uint8_t* output_dev);
// Does this item go side by side?  `params`: the caller's parameters as set (quality, lgwin, mode), not finalized.
bool BatchGreedyEligible(const EncoderParams& params, size_t input_size);
// The streams of `count` eligible items.  Throws std::runtime_error on a device error.  *groups: device groups run.
void BatchGreedyCompress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                         std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// The same with a custom dictionary of 2 .. 65536 bytes (after the reference's truncation): item i is the stream of
// BrotliEncoderSetCustomDictionary + one BrotliEncoderCompressStream(FINISH).  (*reference_fails)[i] != 0: the reference itself
// fails on item i (a copy of one byte at the dictionary end); its stream stays empty.
bool BatchDictionaryEligible(const EncoderParams& params, size_t dict_size, size_t input_size);
void BatchGreedyCompressWithDictionary(const EncoderParams& params, const uint8_t* dict, size_t dict_size, size_t count,
                                       const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                       std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// The same with a dictionary per item: item i lies behind dicts[i] (dict_sizes[i] bytes, after the reference's truncation; several
// items may share a pointer -- dictionaries are told apart by pointer and size, and each goes up once per group).  Every
// (dict_sizes[i], sizes[i]) is BatchDictionaryEligible.  A dictionary that at least BatchDictImageMinItems() items of a group name
// gets an image, built once for the group (at most kBatchGroupImages, the most named first); those items' chains replay it.
// sink != nullptr, for both: the device mode (BatchDeviceSink, with StreamDeliveryRule) -- `dict`, dicts[i] and inputs[i] are device
// addresses of any alignment; every item reads its dictionary where it lies (batch_device.h: batch_stage_dicts_device), and the
// shared dictionary reaches its image by a copy on the device.
void BatchGreedyCompressWithDictionaries(const EncoderParams& params, size_t count, const uint8_t* const* dicts, const size_t* dict_sizes,
                                         const uint8_t* const* inputs, const size_t* sizes, std::vector<std::vector<uint8_t>>* streams,
                                         std::vector<uint8_t>* reference_fails, uint32_t* groups, const BatchDeviceSink* sink = nullptr);
// BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS, read once per process: the items of a group that must name a dictionary for it to get
// an image.  0, or BROTLI_MI355X_BATCH_DICT_SELF_FILE=1: no images.  A dictionary named once never gets one, whatever the value.
size_t BatchDictImageMinItems();
// What BrotliMi355xLastBatchImageInfo reports, counted by the routes into a record of the calling thread: the caller empties it in
// front of a call and reads it behind one.
struct BatchImageCounts {
  uint64_t images;    // dictionary images built, summed over the groups
  uint64_t replayed;  // side-by-side items whose chain replayed an image
  uint64_t filed;     // side-by-side items whose chain filed its own dictionary
};
BatchImageCounts& BatchImageTally();
// Items of several blocks, each one chain: 1 << lgblock < size <= kBatchLongBytes, otherwise as BatchGreedyEligible.
bool BatchLongEligible(const EncoderParams& params, size_t input_size);
// (*demoted)[i] != 0: a meta-block of item i that is not its last took the size fallback (encode.rs:2141-2163), which the chain
// cannot know: the stream stays empty and the caller redoes the item through the one-shot path.
void BatchLongCompress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                       std::vector<std::vector<uint8_t>>* streams, std::vector<uint8_t>* demoted, uint32_t* groups, const BatchDeviceSink* sink = nullptr);

// Qualities 9 and 10 (BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS): an item of at most one input block under the H9 hasher, lgwin 17 .. 24,
// is one live chain on a private H9 table (64 KiB of counters, 32 MiB of buckets) and one meta-block, like an H5 item.  Quality 10
// is taken as quality 9 first, as BrotliEncoderCompress does (encode.rs:1468-1481).  No item is demoted and none fails.
bool BatchQ9Eligible(const EncoderParams& params, size_t input_size);
void BatchQ9Compress(const EncoderParams& params, size_t count, const uint8_t* const* inputs, const size_t* sizes,
                     std::vector<std::vector<uint8_t>>* streams, uint32_t* groups, const BatchDeviceSink* sink = nullptr);

// One group through the meta-block stage (encoder.cpp): an entry is one meta-block; the meta-blocks of an item follow each other
// and make a complete stream of their own.  An item of one meta-block leaves the fields behind `uncompressed` at zero.
struct BatchStreamItem {
  uint32_t start, bytes;         // in the group's packed text (items back to back)
  uint32_t cmd_offset, n_cmds;   // in the gathered command array
  uint32_t n_lits;
  uint32_t uncompressed;
  uint32_t follows;              // not the first meta-block of its item: it goes on at the bit where the one in front ended
  uint32_t more;                 // not the last meta-block of its item
  uint32_t item_bytes;           // the item's size, the size hint of its stream (0: `bytes`)
  uint8_t prev_byte, prev_byte2; // follows != 0: the two text bytes in front of `start`
  uint8_t demoted;               // result, on an item's first entry: a meta-block with `more` set took the size fallback -- the
                                 // parse behind it does not hold, the item's stream is not to be used
  uint64_t out_byte, out_bytes;  // result, on an item's first entry: where its stream lies in `out`
};
// keep != nullptr: the group's output is not downloaded (`out` stays empty); it stays on the device in a block of keep->owner, and
// keep->bytes says where: BatchStreamItem::out_byte counts from there.
class DevBlocks;
struct BatchOutputOnDevice {
  DevBlocks* owner;
  const uint8_t* bytes;  // result
};
void EncodeBatchMetaBlocks(const EncoderParams& finalized, const uint8_t* packed_text_dev, const Command* cmds_dev, uint32_t n_cmds,
                           std::vector<BatchStreamItem>* items, std::vector<uint8_t>* out, BatchOutputOnDevice* keep = nullptr);

}  // namespace brotli_mi355x
#endif
