/* brotli_mi355x.h -- C ABI of the MI355X (gfx950) brotli encoder hot path.
 *
 * Drop-in for the encoder half of rust-brotli's C ABI: every entry point below has the same name,
 * signature and meaning as the one the reference exports from its cdylib (headers c/brotli/encode.h and
 * c/brotli/multiencode.h, implementation src/ffi/compressor.rs and src/ffi/multicompress/mod.rs).  The
 * reference location each function replaces is cited next to it.  Plain pointers and sizes only.
 *
 * Behavioural contract: for the accelerated configurations -- every quality 0..11 at every window the reference takes: the
 * H5 / H5q5 / H6 / H9 greedy path of qualities 5..9; quality 10 / 11 with BROTLI_PARAM_Q9_5 through the stream API (the
 * reference's "9.5": the H9 search with the quality >= 10 meta-block builder, metablock.rs:133-307) and without it (H10 + Zopfli);
 * qualities 2..4 (BasicHasher family) and 0 / 1 (the fragment compressors, on the fragment path and, for catable streams / custom
 * dictionaries / shards, block by block like the reference's ring-buffer path) -- the produced
 * stream is byte-identical to the reference encoder fed the same way.  Everything runs on the GPU through HIP; there is no CPU fallback: calls with
 * parameters outside the accelerated set, or on a machine without a usable gfx950 device, fail
 * (BROTLI_FALSE / 0 / NULL) and print the reason on stderr.
 *
 * Streaming (bounded memory): input handed over with BROTLI_OPERATION_PROCESS is copied into the encoder (as the
 * reference copies it into its ring buffer).  Where the reference runs encode_data whenever a 64 KiB input block is
 * full (encode.rs:2959-2964), this encoder waits until a batch has piled up (64 MiB; BROTLI_MI355X_STREAM_BATCH bytes),
 * then encodes the meta-blocks that the reference's flush rule (encode.rs:2454-2477) closes within the whole blocks
 * received so far and makes their bytes available at once: BrotliEncoderHasMoreOutput() becomes true in the middle of a
 * stream, before any FLUSH / FINISH.  Of what has been encoded only a window is kept as the LZ77 prefix of the next
 * piece (one to two ring-buffer sizes, 8..16 MiB at lgwin 22), together with the state the reference carries: distance
 * cache, static-dictionary throttle counters, which window positions are in the hash table, the per-key insertion
 * counters, the open last byte of the output.  Memory is therefore bounded by window + batch however long the stream;
 * the bytes are those of the reference's stream encoder fed with the same writes (tests/test_streaming.py).
 * BROTLI_OPERATION_FLUSH encodes everything received so far (byte-identical to the reference's flush,
 * encode.rs:2940-2975 + 1541-1566) at a cost proportional to window + new input; BROTLI_OPERATION_EMIT_METADATA
 * (encode.rs:2579-2685) flushes pending input the same way and writes the payload (<= 16 MiB) as a metadata block.
 * A stream of quality 5..9 (and "9.5") may be of any length: the hasher reset of the reference at its position wraps
 * (3, 5, 7 ... GiB, encode.rs:1623-1631, 1705-1710) is reproduced; qualities 0 / 1 keep no hasher between fragments and have no
 * such limit either.  Limits: a stream of quality 2..4 or 10 / 11 must stay below the first wrap (3 GiB) -- their hashers (the
 * BasicHasher table, the H10 trees) travel through the stream as they are and the reset is not reproduced for them: the call
 * that would cross the wrap fails (BrotliMi355xLastError says why; the state is unusable afterwards, like after any failed
 * call), and BrotliEncoderCompress refuses such an input up front, before any work is done.  Streams with a custom
 * dictionary or in the catable / appendable modes stream and flush the same way, piece by piece in bounded memory
 * (tests/test_streaming_dictionary.py).  All input offered to a call is always consumed (*available_in becomes 0).
 *
 * BrotliEncoderCompress (one shot) takes inputs of any size: above 1 GiB (BROTLI_MI355X_ONESHOT_STREAM_ABOVE bytes) the
 * call runs through the same stream state machine in batches -- encoder_compress is a loop over compress_stream with
 * FINISH (encode.rs:1484-1520) -- so its device memory stays bounded as well and the bytes are the reference's one-shot
 * stream (tests/test_oneshot_streamed.py, tests/test_large_gpu.py::test_one_shot_above_2GiB).
 */
#ifndef BROTLI_MI355X_H_
#define BROTLI_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BROTLI_BOOL int
#define BROTLI_TRUE 1
#define BROTLI_FALSE 0

/* c/brotli/types.h:71,81 */
typedef void* (*brotli_alloc_func)(void* opaque, size_t size);
typedef void (*brotli_free_func)(void* opaque, void* address);

/* c/brotli/encode.h:45-61 (+ the reference's extra prior modes, src/ffi/compressor.rs:30-38) */
typedef enum BrotliEncoderMode {
  BROTLI_MODE_GENERIC = 0,
  BROTLI_MODE_TEXT = 1,
  BROTLI_MODE_FONT = 2,
  BROTLI_FORCE_LSB_PRIOR = 3,
  BROTLI_FORCE_MSB_PRIOR = 4,
  BROTLI_FORCE_UTF8_PRIOR = 5,
  BROTLI_FORCE_SIGNED_PRIOR = 6
} BrotliEncoderMode;

/* c/brotli/encode.h:71-135 */
typedef enum BrotliEncoderOperation {
  BROTLI_OPERATION_PROCESS = 0,
  BROTLI_OPERATION_FLUSH = 1,
  BROTLI_OPERATION_FINISH = 2,
  BROTLI_OPERATION_EMIT_METADATA = 3
} BrotliEncoderOperation;

/* c/brotli/encode.h:138-232, src/enc/parameters.rs:3-33.  BrotliEncoderSetParameter refuses ids 7, 8 and 170 as the reference does
 * (its setter has no arm for them, src/enc/encode.rs:196-286), although the enum names them. */
typedef enum BrotliEncoderParameter {
  BROTLI_PARAM_MODE = 0,
  BROTLI_PARAM_QUALITY = 1,
  BROTLI_PARAM_LGWIN = 2,
  BROTLI_PARAM_LGBLOCK = 3,
  BROTLI_PARAM_DISABLE_LITERAL_CONTEXT_MODELING = 4,
  BROTLI_PARAM_SIZE_HINT = 5,
  BROTLI_PARAM_LARGE_WINDOW = 6,
  BROTLI_PARAM_NPOSTFIX = 7,
  BROTLI_PARAM_NDIRECT = 8,
  BROTLI_PARAM_Q9_5 = 150,
  BROTLI_METABLOCK_CALLBACK = 151,
  BROTLI_PARAM_STRIDE_DETECTION_QUALITY = 152,
  BROTLI_PARAM_HIGH_ENTROPY_DETECTION_QUALITY = 153,
  BROTLI_PARAM_LITERAL_BYTE_SCORE = 154,
  BROTLI_PARAM_CDF_ADAPTATION_DETECTION = 155,
  BROTLI_PARAM_PRIOR_BITMASK_DETECTION = 156,
  BROTLI_PARAM_SPEED = 157,
  BROTLI_PARAM_SPEED_MAX = 158,
  BROTLI_PARAM_CM_SPEED = 159,
  BROTLI_PARAM_CM_SPEED_MAX = 160,
  BROTLI_PARAM_SPEED_LOW = 161,
  BROTLI_PARAM_SPEED_LOW_MAX = 162,
  BROTLI_PARAM_CM_SPEED_LOW = 164,
  BROTLI_PARAM_CM_SPEED_LOW_MAX = 165,
  BROTLI_PARAM_AVOID_DISTANCE_PREFIX_SEARCH = 166,
  BROTLI_PARAM_CATABLE = 167,
  BROTLI_PARAM_APPENDABLE = 168,
  BROTLI_PARAM_MAGIC_NUMBER = 169,
  BROTLI_PARAM_NO_DICTIONARY = 170,
  BROTLI_PARAM_FAVOR_EFFICIENCY = 171,
  BROTLI_PARAM_BYTE_ALIGN = 172,
  BROTLI_PARAM_BARE_STREAM = 173
} BrotliEncoderParameter;

typedef struct BrotliEncoderStateStruct BrotliEncoderState;
typedef struct BrotliEncoderWorkPoolStruct BrotliEncoderWorkPool;

/* ---- single-stream encoder: c/brotli/encode.h:256-457 ---- */
/* src/ffi/compressor.rs:72 */
BrotliEncoderState* BrotliEncoderCreateInstance(brotli_alloc_func alloc_func, brotli_free_func free_func, void* opaque);
/* src/ffi/compressor.rs:115 (returns BROTLI_FALSE once the encoder has started, encode.rs:289-295) */
BROTLI_BOOL BrotliEncoderSetParameter(BrotliEncoderState* state, BrotliEncoderParameter p, uint32_t value);
/* src/ffi/compressor.rs:128 (NULL is accepted) */
void BrotliEncoderDestroyInstance(BrotliEncoderState* state);
/* src/ffi/compressor.rs:190, src/enc/encode.rs:1276-1299 */
size_t BrotliEncoderMaxCompressedSize(size_t input_size);
/* src/ffi/compressor.rs:194, src/enc/encode.rs:1436-1538 */
BROTLI_BOOL BrotliEncoderCompress(int quality, int lgwin, BrotliEncoderMode mode, size_t input_size,
                                  const uint8_t* input_buffer, size_t* encoded_size, uint8_t* encoded_buffer);
/* src/ffi/compressor.rs:280, src/enc/encode.rs:2873-2995 */
BROTLI_BOOL BrotliEncoderCompressStream(BrotliEncoderState* state, BrotliEncoderOperation op, size_t* available_in,
                                        const uint8_t** next_in, size_t* available_out, uint8_t** next_out,
                                        size_t* total_out);
/* src/ffi/compressor.rs:260 */
BROTLI_BOOL BrotliEncoderCompressStreaming(BrotliEncoderState* state, BrotliEncoderOperation op, size_t* available_in,
                                           const uint8_t* next_in, size_t* available_out, uint8_t* next_out);
/* src/ffi/compressor.rs:144,153,179 */
BROTLI_BOOL BrotliEncoderIsFinished(BrotliEncoderState* state);
BROTLI_BOOL BrotliEncoderHasMoreOutput(BrotliEncoderState* state);
const uint8_t* BrotliEncoderTakeOutput(BrotliEncoderState* state, size_t* size);
/* src/ffi/compressor.rs:162, src/enc/encode.rs:1196-1270 */
void BrotliEncoderSetCustomDictionary(BrotliEncoderState* state, size_t size, const uint8_t* dict);
/* src/ffi/compressor.rs:186: 0x01000f01 */
uint32_t BrotliEncoderVersion(void);
/* src/ffi/compressor.rs:359-417 */
uint8_t* BrotliEncoderMallocU8(BrotliEncoderState* state, size_t size);
void BrotliEncoderFreeU8(BrotliEncoderState* state, uint8_t* data, size_t size);
size_t* BrotliEncoderMallocUsize(BrotliEncoderState* state, size_t size);
void BrotliEncoderFreeUsize(BrotliEncoderState* state, size_t* data, size_t size);

/* ---- multi-chunk encoder: c/brotli/multiencode.h:41-127 ---- */
/* src/ffi/multicompress/mod.rs:49 */
size_t BrotliEncoderMaxCompressedSizeMulti(size_t input_size, size_t num_threads);
/* src/ffi/multicompress/mod.rs:93: the input is split into desired_num_threads (<= 16) chunks exactly as the
   reference's compress_multi does (src/enc/threading/mod.rs:333-411); chunks are compressed on the GPU and
   stitched with the BroCatli rules (src/concat/mod.rs). */
int32_t BrotliEncoderCompressMulti(size_t num_params, const BrotliEncoderParameter* param_keys, const uint32_t* param_values,
                                   size_t input_size, const uint8_t* input_buffer, size_t* encoded_size, uint8_t* encoded,
                                   size_t desired_num_threads, brotli_alloc_func alloc_func, brotli_free_func free_func,
                                   void** alloc_opaque_per_thread);
/* src/ffi/multicompress/mod.rs:240,294,312: the work pool owns no threads here (the GPU is the pool) */
BrotliEncoderWorkPool* BrotliEncoderCreateWorkPool(size_t num_threads, brotli_alloc_func alloc_func, brotli_free_func free_func,
                                                   void** alloc_opaque_per_thread);
void BrotliEncoderDestroyWorkPool(BrotliEncoderWorkPool* work_pool);
int32_t BrotliEncoderCompressWorkPool(BrotliEncoderWorkPool* work_pool, size_t num_params, const BrotliEncoderParameter* param_keys,
                                      const uint32_t* param_values, size_t input_size, const uint8_t* input_buffer,
                                      size_t* encoded_size, uint8_t* encoded, size_t desired_num_threads,
                                      brotli_alloc_func alloc_func, brotli_free_func free_func, void** alloc_opaque_per_thread);

/* ---- extensions of this implementation (not part of the reference ABI) ---- */
/* Compresses chunk `thread_index` of `num_threads` of a compress_multi job (what one reference worker thread
   does in compress_part, src/enc/threading/mod.rs:337-411).  input_on_device != 0: input_buffer is a device
   pointer (data resident in HBM).  Used to spread the chunks over several GPUs (one process per GPU). */
int32_t BrotliMi355xCompressChunk(size_t num_params, const BrotliEncoderParameter* param_keys, const uint32_t* param_values,
                                  size_t input_size, const uint8_t* input_buffer, int input_on_device, size_t thread_index,
                                  size_t num_threads, size_t* encoded_size, uint8_t* encoded);
/* Stitches already compressed chunks (in order) into one stream: BroCatli new_brotli_file/stream/finish,
   src/enc/threading/mod.rs:565-660.  Returns 1 on success. */
int32_t BrotliMi355xConcatChunks(size_t num_chunks, const uint8_t* const* chunks, const size_t* chunk_sizes,
                                 size_t* encoded_size, uint8_t* encoded);
/* The same for chunks whose bodies live elsewhere (device memory): only the first and last min(8, size) bytes of every
   chunk are given (heads[8 * i ..], tails[8 * i ..]).  The junction bytes are written into `encoded`; for chunk i the
   caller then copies body_copies[3 * i + 2] bytes from offset body_copies[3 * i + 1] of the chunk to offset
   body_copies[3 * i] of `encoded`. */
int32_t BrotliMi355xConcatChunkEnds(size_t num_chunks, const uint8_t* heads, const uint8_t* tails,
                                    const size_t* chunk_sizes, size_t* encoded_size, uint8_t* encoded,
                                    size_t* body_copies);
/* One-shot compression of a buffer that is already resident in device memory; per-stage timings (ms) are
   returned in stats[0..32) (may be NULL).  Same stream as BrotliEncoderCompress on the same bytes.
   Ordering: the call works on the calling thread's stream; whatever produced the input must be complete before the call (it does
   not wait for other streams), and the call returns when the stream is in `encoded_host`. */
BROTLI_BOOL BrotliMi355xCompressDevice(int quality, int lgwin, BrotliEncoderMode mode, size_t input_size,
                                       const uint8_t* input_device, size_t* encoded_size, uint8_t* encoded_host,
                                       double* stats);
/* Many inputs in one call, each a complete stream of its own: item i gets exactly what
   BrotliEncoderCompress(quality, lgwin, mode, input_sizes[i], inputs[i], &output_sizes[i], outputs[i]) gives -- bytes, size,
   success or failure.  output_sizes[i] holds the capacity of outputs[i] on entry and the size of the stream on return.
   An item that fails (capacity 0, or a buffer too small) fails alone: its size becomes 0 and item_results[i] (may be NULL)
   becomes 0, the other items are still produced.  Returns 1 if every item succeeded (count == 0 included), 0 otherwise.  A
   device error fails the whole call: every size becomes 0 and BrotliMi355xLastError says why.  Inputs are host memory.
   This is the call for many small payloads.  Which items run side by side on the device:
     qualities 0 and 1: every item; the fragments of all items share one upload and one download per group of up to 4096;
     qualities 5 .. 8:  the items of at most one input block (65 536 bytes) at lgwin 17 .. 24 -- one parse chain and one
                        meta-block each, thousands of them in flight, one upload and one download per group of up to 4096 items.
   Every other item -- qualities 2 .. 4 (but see BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS of BrotliMi355xCompressBatchEx) and
   9 .. 11 (but see BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS and BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS there), lgwin <= 16 or > 24, items longer than one input block -- is accepted and
   runs by itself through the one-shot path on the calling thread, in the same call and in the caller's order: the same bytes,
   no gain in speed.  Both kinds may be mixed in one call; BrotliMi355xLastBatchInfo tells how a call was taken.
   Environment (read once per process): BROTLI_MI355X_BATCH_GROUP_ITEMS / BROTLI_MI355X_BATCH_GROUP_BYTES bound a group of
   qualities 5 .. 8 (4096 items, 64 MiB), BROTLI_MI355X_BATCH_TABLES the number of hash tables, i.e. of chains in flight
   (default: as many as stay resident, within 8 GiB; a table is 1 MiB at quality 5 and 16 MiB at quality 8, 32 MiB at qualities
   9 and 10 under BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS). */
int32_t BrotliMi355xCompressBatch(int quality, int lgwin, BrotliEncoderMode mode, size_t count, const uint8_t* const* inputs,
                                  const size_t* input_sizes, uint8_t* const* outputs,
                                  size_t* output_sizes /* in: capacity, out: size */, int32_t* item_results /* may be NULL */);
/* The batch call with one custom dictionary shared by every item -- the call for thousands of small payloads of one kind (messages,
   records, API responses), whose redundancy lies in what they share with each other rather than in themselves.
   Item i is exactly the stream of: BrotliEncoderCreateInstance; BrotliEncoderSetParameter(QUALITY, LGWIN, MODE);
   BrotliEncoderSetCustomDictionary(dict_size, dict); one BrotliEncoderCompressStream(BROTLI_OPERATION_FINISH) with all of
   inputs[i] and enough room -- in bytes, size, success or failure.  A decoder needs the same dictionary.  The rules are the stream
   API's: no size hint is set and there is no fallback to a stored stream above BrotliEncoderMaxCompressedSize (give every item
   BrotliEncoderMaxCompressedSize(size) + 1024 bytes of room); a dictionary longer than (1 << lgwin) - 16 bytes is cut to its last
   (1 << lgwin) - 16; with dict_size <= 1 and at qualities 0 / 1 the reference takes no dictionary and only makes the stream
   catable and appendable.  dict may be NULL when dict_size is 0.  count == 0 returns 1.
   An item whose stream does not fit its capacity fails alone (size 0, item_results[i] = 0), the others are produced and the call
   returns 0.  So does an item on which the reference itself fails -- a match cut to one byte at the end of the dictionary, a copy
   the format cannot express: BrotliMi355xLastError then says "the reference encoder fails on this input".  A device error fails
   the whole call.
   Side by side on the device (one upload of the dictionary per call, the text dictionary | item laid out there, one chain per
   item on a hash table already holding the dictionary): qualities 5 .. 8, lgwin 17 .. 24, 2 <= dict_size <= 65536 and
   1 <= input_sizes[i] <= 65536.  Everything else -- other qualities and windows, longer items, longer or shorter dictionaries, the
   empty item -- is accepted and runs by itself through the stream path on the calling thread, in the same call and in the
   caller's order: the same bytes, no gain in speed (qualities 2 .. 4: see BrotliMi355xCompressBatchWithDictionaryEx).  The environment of BrotliMi355xCompressBatch applies; a group's byte limit
   counts one copy of the dictionary per item. */
int32_t BrotliMi355xCompressBatchWithDictionary(int quality, int lgwin, BrotliEncoderMode mode, size_t dict_size, const uint8_t* dict,
                                                size_t count, const uint8_t* const* inputs, const size_t* input_sizes,
                                                uint8_t* const* outputs, size_t* output_sizes /* in: capacity, out: size */,
                                                int32_t* item_results /* may be NULL */);
/* BrotliMi355xCompressBatch with routes the caller opts into.  routes == 0 is BrotliMi355xCompressBatch in every respect.  A bit
   this build does not know fails the whole call like a device error does (returns 0, every size 0, BrotliMi355xLastError says so,
   only info[0] of BrotliMi355xLastBatchInfo is set), so a caller can probe for routes of later builds.
   BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS: item i still gets exactly what BrotliEncoderCompress gives, by the rules above.  In
   addition to the items the plain call takes side by side, an item of more than one and at most four input blocks
   (65 536 < input_sizes[i] <= 262 144) at qualities 5 .. 8, lgwin 17 .. 24 runs on the device as ONE parse chain that walks from
   block to block, side by side with the other such items of the call (groups of their own, under the same environment limits),
   and leaves up to four meta-blocks.  Every other item goes as in the plain call.  When a meta-block that is not the item's last
   turns out longer coded than stored, the reference stores it and parses on from another distance cache, which the chain could
   not know: that item is redone through the one-shot path in the same call (info[6]).
   When to set it: a chain is one wavefront bound by its own dependent loads, so a long item takes as long as a lone chain needs
   for it however many run beside it; the one-shot path is faster per item and serial.  The route pays with many long items in a
   call, or with data on which the one-shot path needs many rounds (see INTEGRATION.md for measured figures); with a few long
   items of text it loses.  Not combined with a shared dictionary.
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: item i still gets exactly what BrotliEncoderCompress gives.  In addition to the items
   the plain call takes side by side, an item of at most one input block at quality 2, 3 or 4 and lgwin 10 .. 24 -- that is
   1 <= input_sizes[i] <= 16 384 at quality 2 / 3 and <= 65 536 at quality 4 -- runs on the device as ONE chain on a private
   BasicHasher table (H2 / H3 / H4; 256 KiB, at quality 4 512 KiB), side by side with the other such items of the call (groups of
   their own, under the same environment limits; 4096 tables by default), and leaves one meta-block.  Every other item goes as in
   the plain call: longer items at these qualities still run one by one, with BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS set as well
   (BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS takes those of up to four blocks).
   The bit changes nothing at qualities 0, 1 and 5 .. 11.  Such items count in info[1], their groups in info[4]; info[6] and
   info[7] stay 0 for them.  When to set it: with hundreds of small items of one kind in a call (dynamic responses at the levels
   servers use for them); a chain is one wavefront bound by its own dependent loads, so a call of a few items is no faster
   than the one-by-one path (see INTEGRATION.md for measured figures).  With a shared dictionary:
   BrotliMi355xCompressBatchWithDictionaryEx.
   BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS: item i still gets exactly what BrotliEncoderCompress gives.  In addition, an item
   of more than one and at most four input blocks at quality 2, 3 or 4 and lgwin 10 .. 24 -- that is
   16 385 <= input_sizes[i] <= 65 536 at quality 2 / 3 and 65 537 <= input_sizes[i] <= 262 144 at quality 4 -- runs on the device
   as ONE chain on a private BasicHasher table that walks from block to block, side by side with the other such items of the call
   (groups of their own, under the same environment limits), and leaves up to four meta-blocks.  The bit is independent of
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: alone it takes the items of several blocks only and the shorter ones run one by one;
   both bits take both.  It changes nothing at qualities 0, 1 and 5 .. 11, and BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS together with
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS does NOT stand for it.  Such items count in info[1] and info[7], their groups in info[4].
   When a meta-block that is not the item's last turns out longer coded than stored, the item is redone through the one-shot path
   in the same call (info[6]), as under BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS.  When to set it: a chain is one wavefront bound by
   its own dependent loads, so an item of several blocks takes a lone chain's time however many items run beside it; the route
   pays with many such items in a call (dynamic responses of 20 to 64 KiB at quality 2 / 3; see INTEGRATION.md for measured
   figures) and loses with a few.  Not combined with a shared dictionary.
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS: item i still gets exactly what BrotliEncoderCompress gives.  In addition, an item with
   1 <= input_sizes[i] <= 65 536 at quality 11 and lgwin 10 .. 24 -- always at most one input block, lgblock is at least 16 at
   this quality -- runs on the device as ONE wavefront that walks the item the reference's way (H10 trees, matches and the Zopfli
   shortest-path programme position by position) on private trees, side by side with the other such items of the call (groups of
   their own, of at most 1024 items: what the quality >= 10 meta-block builder sets aside per item; as many tables as stay
   resident, 256, within 8 GiB, a table sized by its group's largest item), and leaves one meta-block.  Every other item goes as in
   the plain call.  The bit changes nothing at qualities 0 .. 10.  Quality 10 is not taken: BrotliEncoderCompress runs it at
   quality 9, as the reference's one-shot entry does, so the bytes an item of quality 10 is owed are not those of a Zopfli walk
   (BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS takes such items).  Such
   items count in info[1], their groups in info[4]; nothing is redone, info[6] and info[7] stay 0 for them.  An item on which the
   reference encoder itself panics fails alone with "the reference encoder fails on this input", as under
   BrotliMi355xCompressBatchWithDictionary.  When to set it: with hundreds of small static files in a call (pre-compression at
   the level used for it).  A walk is one wavefront bound by its own dependent loads and takes a lone walk's time however many
   run beside it (about 37 us per byte: 150 ms for 4 KiB, 2.4 s for 64 KiB), so the call lasts as long as its largest item's walk
   times the items per table.  Measured: 1024 items of 4 KiB in 0.6 s against 89 s one by one, 16 of them in 0.16 s against 1.4 s.
   When not: for one or two items the one-shot path, which finds a lone item's matches side by side, is as fast or faster; and a
   handful of small items is done sooner on one CPU core than on the device either way (see INTEGRATION.md for measured
   figures).  Not combined with a shared dictionary.
   BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS: item i still gets exactly what BrotliEncoderCompress gives.  In addition, an item of at
   most one input block at quality 9 or 10 and lgwin 17 .. 24 -- that is 1 <= input_sizes[i] <= 131 072 at lgwin 17 and
   <= 262 144 from lgwin 18 on -- runs on the device as ONE chain on a private H9 hash table (32 768 keys with rings 256 deep:
   64 KiB of counters and 32 MiB of buckets), side by side with the other such items of the call (groups of their own, under the
   same environment limits; 255 tables by default, what 8 GiB hold), and leaves one meta-block.  Quality 10 goes as quality 9:
   BrotliEncoderCompress runs it so, as the reference's one-shot entry does.  Every other item goes as in the plain call; at
   lgwin <= 16 the reference selects another hasher and the items stay one by one.  The bit changes nothing at qualities 0 .. 8
   and 11, so with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS beside it quality 10 goes this way and quality 11 the Zopfli way.  Such
   items count in info[1], their groups in info[4]; nothing is redone and no item fails like the reference, info[5] .. info[7]
   stay 0 for them.  When to set it: with dozens to thousands of small items in a call at the strongest greedy
   level.  A chain is one wavefront bound by its own dependent loads -- about 1.07 us per byte of text, 6 ms for 4 KiB, 70 ms for
   64 KiB, 258 ms for 256 KiB -- and takes a lone chain's time however many run beside it, so the call lasts as long as its
   largest item's chain times the items per table; the one-by-one path takes about 2 ms per item whatever its size.  Measured:
   4096 items of 4 KiB in 0.10 s against 6.8 s one by one, 1024 of 16 KiB in 0.10 s against 1.8 s, 256 of 64 KiB in 0.14 s against
   0.47 s, 16 of 4 KiB in 6.7 ms against 26 ms.  When not: 64 items of 256 KiB of text LOSE (258 ms against 142 ms one by one, 74 ms
   from four threads), and so does a call of one or two items of any size; by the same figures the break-even is near 40 items of
   64 KiB and 120 of 256 KiB (see INTEGRATION.md for measured figures).  Not combined with a shared dictionary.
   The bits may be combined.  The values 2, 8 and 64 are reserved: they name no route and fail the call like any unknown bit, as
   do 256 and above. */
#define BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS 1u
#define BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS 4u /* (2u is reserved and stays an unknown route) */
#define BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS 16u /* (8u stays an unknown route, like 2u) */
#define BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS 32u
#define BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS 128u /* (64u stays an unknown route, like 2u and 8u) */
int32_t BrotliMi355xCompressBatchEx(int quality, int lgwin, BrotliEncoderMode mode, uint32_t routes, size_t count,
                                    const uint8_t* const* inputs, const size_t* input_sizes, uint8_t* const* outputs,
                                    size_t* output_sizes /* in: capacity, out: size */, int32_t* item_results /* may be NULL */);
/* BrotliMi355xCompressBatchEx on device memory: many items that lie in device memory, their streams left in device memory.  It is
   that call in every respect but one: inputs_device[i] and outputs_device[i] are device addresses on the calling thread's current
   device.  The four arrays themselves (inputs_device, input_sizes, outputs_device, output_sizes) and item_results are host memory,
   as there.  The addresses may have any alignment, and several may point into one allocation (one tensor of items, one of streams).
   Per item: exactly what BrotliEncoderCompress(quality, lgwin, mode, input_sizes[i], <the bytes at inputs_device[i]>,
   &output_sizes[i], ...) gives -- bytes, size, success or failure: the empty item is the byte 0x06 (written to device memory), an
   item of capacity 0 or with a buffer too small fails alone (size 0), and an item whose stream exceeds
   BrotliEncoderMaxCompressedSize goes out as the stored stream of its input where the capacity allows (produced on the device).
   `routes` takes the same five bits with the same eligibility rules, the same reserved or unknown values fail the whole call,
   BrotliMi355xLastBatchInfo means what it means there, and a device error fails the whole call in the same way.
   On the side-by-side routes (info[1], qualities 2 .. 11) no item byte and no stream byte crosses the bus: one launch gathers a
   group's items from their addresses, one launch scatters its streams to theirs.  The other items:
     - at qualities 2 .. 11 an item that does not go side by side runs through the device one-shot path by itself, as
       BrotliMi355xCompressDevice does; its stream passes through host memory on its way to outputs_device[i];
     - at qualities 0 and 1 the fragment path takes its input from host memory: the items are downloaded once per call and their
       streams uploaded -- the same bytes and the same info as the host call, and no gain over it.
   Memory contract.  The library reads only the aligned 4-byte words that hold at least one byte of an item; it never reads behind an
   item's last word.  On return it has written exactly outputs_device[i][0 .. output_sizes[i]), and never a byte outside
   [0, capacity); an item that fails leaves the contents of its buffer unspecified, but stays inside it.  Outputs must not overlap
   each other or any input; they may abut.
   Ordering.  The call works on the calling thread's stream and returns after everything it wrote has landed (one synchronisation
   at the end).  Whatever produced the inputs must be complete before the call: it does not wait for other streams.
   No dictionary: behind a dictionary per item, or one shared by all, the call is BrotliMi355xCompressBatchWithDictionariesDevice;
   the other dictionary batch calls take host memory only.
   When to use it: when the payloads already lie in device memory, or the streams are wanted there.  Measured on an MI355X against
   BrotliMi355xCompressBatchEx on the same items from page-locked host memory, min .. max of five alternating runs, text: 4096 items
   of 4 KiB at quality 5 in 12.3 .. 12.4 ms against 16.0 .. 16.3 ms (and 16.7 .. 17.1 ms for download + host call + upload), at
   quality 2 with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS 11.1 .. 11.2 against 14.8 .. 14.9 ms, 1024 items of 16 KiB at quality 5
   18.0 .. 18.1 against 20.8 .. 21.1 ms.  Where the parse dominates the staging is nothing: 256 items of 64 KiB at quality 9 with
   BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS 137.3 .. 137.9 against 139.8 .. 144.9 ms, 64 items of 4 KiB at quality 5 4.31 .. 4.33 against
   4.30 .. 4.33 ms -- no gain there, and none at qualities 0 and 1.  No measured shape is slower than the host call. */
int32_t BrotliMi355xCompressBatchDevice(int quality, int lgwin, BrotliEncoderMode mode, uint32_t routes, size_t count,
                                        const uint8_t* const* inputs_device, const size_t* input_sizes, uint8_t* const* outputs_device,
                                        size_t* output_sizes /* in: capacity, out: size */, int32_t* item_results /* may be NULL */);
/* BrotliMi355xCompressBatchWithDictionary with routes the caller opts into.  routes == 0 is that call in every respect.  The
   routes this call knows are BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS (4), BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096,
   defined and described with BrotliMi355xCompressBatchWithDictionaries below) and
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (8192, defined there, described here); they may be combined, and
   since a call has one quality at most one of them takes items.  Any other bit -- the other routes of
   BrotliMi355xCompressBatchEx, 512 and 1024 of the per-item calls, and the reserved values 2, 8 and 64 included -- fails the whole call as an unknown route fails that one
   (returns 0, every size 0, BrotliMi355xLastError says so, only info[0] of BrotliMi355xLastBatchInfo is set).
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: item i is still exactly the stream of BrotliEncoderSetCustomDictionary + one
   BrotliEncoderCompressStream(BROTLI_OPERATION_FINISH), by the rules above -- in bytes, size, success or failure.  In addition
   to the items that call takes side by side, an item of at most one input block at quality 2, 3 or 4 and lgwin 10 .. 24 -- that
   is 1 <= input_sizes[i] <= 16 384 at quality 2 / 3 and <= 65 536 at quality 4 -- behind a dictionary of dict_size >= 2 of which
   at most 65 536 bytes are in use (min(dict_size, (1 << lgwin) - 16): the reference's truncation) runs on the device as ONE chain
   on a private BasicHasher table (H2 / H3 / H4; 256 KiB, at quality 4 512 KiB), side by side with the other such items of the
   call.  The dictionary goes up once per call, and so does the table the reference's prepend leaves for it; every chain copies
   that table over its own in front of every item (the cost of the zero fill of the plain route), parses dictionary | item with
   positions counted from the dictionary's first byte, and leaves one meta-block.  Every other item -- the empty one, items
   longer than one input block, dict_size <= 1 -- runs by itself through the stream path on the calling thread, in the same call
   and in the caller's order.  The bit changes nothing at qualities 0, 1 and 5 .. 11: at qualities 5 .. 8 the items still take the
   dictionary route of the plain call.  Such items count in info[1], their groups in info[4]; info[5] is the dictionary bytes in
   use; info[6] and info[7] stay 0.  An item on which the reference fails ("the reference encoder fails on this input") fails
   alone, as does one whose stream does not fit; a device error fails the call.  At quality 2 on text behind a dictionary of the
   same kind about 3 in 1000 items of 4 KiB are such inputs: pass item_results and expect a call of thousands
   of items to return 0 with a few of them failed alone.  The environment of BrotliMi355xCompressBatch
   applies (4096 tables by default; a group's byte limit counts one copy of the dictionary per item).
   When to set it: with hundreds of small items of one kind in a call that share a dictionary (dynamic responses, messages,
   records at the levels servers use for them).  When not: with a few items -- a chain is one wavefront bound by its own
   dependent loads, so a call of a few items is no faster than the one-by-one path (see INTEGRATION.md for measured figures).
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (8192; known to this call only -- it is to
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS, 1024, what 4 here is to 512 there, and 1024 stays an unknown route of this
   call): item i is still exactly the stream of BrotliEncoderSetCustomDictionary + one FINISH, at quality 10 AND at quality 11 --
   through the stream API both are Zopfli.  An item of 1 <= input_sizes[i] <= 65 536 bytes at quality 10 or 11 and lgwin 10 .. 24
   behind a dictionary of dict_size >= 2 of which at most 65 536 bytes are in use (min(dict_size, (1 << lgwin) - 16)) runs on the
   device as ONE wavefront on H10 trees of its own, side by side with the other such items of the call.  The dictionary's part of
   those trees hangs on the dictionary alone (a stored position compares at most 128 bytes, all inside it), so the call builds ONE
   image of it -- 512 KiB of buckets and 8 bytes of forest per dictionary byte, at most 1 MiB, by 1024 lanes of 16 workgroups
   that each own a class of hash keys -- and in front of every item a chain copies the image over its table and zeroes the item's
   part of the forest, where the per-item route files the dictionary anew; then it stitches and walks the item from position D as
   that route does.  Every other item -- the empty one, longer items, dict_size <= 1, more than 65 536 bytes in use -- runs by
   itself through the stream path, as every item of these qualities does without the bit (65 .. 440 ms apiece).  The bit changes
   nothing at qualities 0 .. 9.  Such items count in info[1], their groups (at most 1024 items) in info[4]; info[5] is the
   dictionary bytes in use; info[6] and info[7] stay 0.  BrotliMi355xCompressBatchWithDictionaries and its device form with 1024
   take the same path when every item names one index: same bytes, equal info.  Memory is that route's: a table per item in
   flight, at most 256, plus the image.
   When to set it: tens to thousands of small items behind one dictionary at the level static files are pre-compressed at.
   Measured (text, lgwin 22, quality 10 / 11, min .. max of five alternating runs; profiles/r29_batch_dictionary_zopfli.json; the
   one-by-one baseline timed on 8 items and scaled): 1024 items of 4 KiB behind 16 KiB in 244 .. 245 / 546 .. 547 ms against
   302 .. 304 / 603 .. 604 ms for the parent build's BrotliMi355xCompressBatchWithDictionaries with 1024 and one index, where
   every chain filed its own copy (1.24 / 1.11 x), and 66 .. 67 / 110 .. 112 s for this call without the bit; 256 items of 16 KiB
   behind 64 KiB in 283 .. 284 / 575 .. 577 against 338 .. 339 / 629 .. 631 ms (1.19 / 1.09 x; without the bit 65 .. 66 / 112 ..
   113 s); 256 items of 4 KiB behind 64 KiB in 100 .. 101 / 172 .. 173 against 154 .. 155 / 227 .. 228 ms (1.54 / 1.31 x; 43 /
   54 .. 55 s); 16 items of 4 KiB behind 16 KiB in 73 .. 74 / 144 .. 146 against 85 / 155 .. 156 ms (1.15 / 1.07 x; 1.04 .. 1.05 /
   1.72 .. 1.75 s).  BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 (every chain files the dictionary itself, for A/B runs) reproduces the
   parent's figures within 1 %.  No measured shape is slower than self-filing or than the call without the bit.  The image's
   build takes 3.7 .. 4.0 ms for 16 KiB and 17.7 .. 19.2 ms for 64 KiB, once per call; a lone chain files them in 15.0 .. 15.2 and
   65.5 .. 68.7 ms wave-wide (17.6 .. 18.0 and 120 .. 122 ms on lane 0), in front of every item.
   When not: a call of a few items -- a walk is one wavefront and lasts its item's time however many run beside it (about 70 /
   140 ms for 4 KiB behind 16 KiB): one such item through the route takes 70 .. 71 / 138 .. 141 ms, no faster than the stream
   path by itself (65 / 107 ms), and 16 of them still lose to one CPU core (29 / 61 ms in
   profiles/r27_batch_dictionaries_zopfli.json).  The image does not change that: it removes the filing, not the walk. */
int32_t BrotliMi355xCompressBatchWithDictionaryEx(int quality, int lgwin, BrotliEncoderMode mode, uint32_t routes, size_t dict_size,
                                                  const uint8_t* dict, size_t count, const uint8_t* const* inputs,
                                                  const size_t* input_sizes, uint8_t* const* outputs,
                                                  size_t* output_sizes /* in: capacity, out: size */,
                                                  int32_t* item_results /* may be NULL */);
/* The batch call with a custom dictionary PER ITEM -- the call for delta compression of many resources, each against its own
   previous version ("dictionary = the old file"), for records of several kinds in one call, each kind with its dictionary, and for
   per-tenant or per-route dictionaries on a server.
   Item i is exactly the stream of: BrotliEncoderCreateInstance; BrotliEncoderSetParameter(QUALITY, LGWIN, MODE);
   BrotliEncoderSetCustomDictionary(dict_sizes[k], dicts[k]) with k = item_dicts[i]; one
   BrotliEncoderCompressStream(BROTLI_OPERATION_FINISH) with all of inputs[i] and enough room -- in bytes, size, success or failure.
   Every rule of BrotliMi355xCompressBatchWithDictionary holds per item: no size hint, no fallback to a stored stream (give every
   item BrotliEncoderMaxCompressedSize(size) + 1024 bytes of room), a dictionary cut to its last (1 << lgwin) - 16 bytes, no
   dictionary taken with dict_sizes[k] <= 1 or at qualities 0 / 1 (the stream is then only catable and appendable); an item whose
   stream does not fit fails alone, as does one on which the reference itself fails ("the reference encoder fails on this input"),
   and the call then returns 0; a device error fails the whole call.
   item_dicts == NULL: item i takes dicts[i], and num_dicts must be count.  Several items may name one index.  Dictionaries are
   told apart by index, not by content.  dicts[k] may be NULL when dict_sizes[k] is 0.  count == 0 returns 1.
   An index >= num_dicts, item_dicts == NULL with num_dicts != count, or any bit in routes other than
   BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS and
   BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS fails the whole call before any work is done, as an unknown route fails BrotliMi355xCompressBatchEx (returns 0, every size 0, BrotliMi355xLastError
   says why, only info[0] of BrotliMi355xLastBatchInfo is set).  routes == 0 is the call as described below in every respect.
   The three routes this call knows, so a caller can probe; they may be combined, and since a call has one quality at most one
   of them takes items.
   BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS (512; the bits of the other batch calls, 4 and 256 among them, stay unknown
   here, and 512 stays unknown there): item i is still exactly the stream described above.  In addition to the items the call
   takes side by side without it, an item of at most one input block at quality 2, 3 or 4 and lgwin 10 .. 24 -- 1 <=
   input_sizes[i] <= 16 384 at quality 2 / 3 and <= 65 536 at quality 4 -- behind a dictionary of dict_sizes[k] >= 2 of which at
   most 65 536 bytes are in use (the rule of BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS of BrotliMi355xCompressBatchWithDictionaryEx,
   applied per item) runs on the device as ONE chain on a private BasicHasher table.  A dictionary that enough items of a device group
   name gets a table image, built once for that group (BrotliMi355xLastBatchImageInfo below has the rule, the threshold variable and
   the cap of 64 images, 256 / 512 KiB each); the chain of an item that names it copies the image over its table.  Every other chain
   zeroes its table and files the item's dictionary itself, 64 positions per step with an atomic maximum (what the reference's
   prepend leaves in a slot is the largest position filed under it).  Either way it then parses the item.  Every other item -- the empty one, longer items, dict_sizes[k] <= 1, more than
   65 536 bytes in use -- runs by itself through the stream path with its own dictionary.  The bit changes nothing at qualities 0,
   1 and 5 .. 11.  Such items count in info[1], their groups in info[4]; info[2], info[5] as below; info[6] and info[7] stay 0.
   When every item names one index the call is BrotliMi355xCompressBatchWithDictionaryEx with
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS and that dictionary (same bytes, same info, the shared image).  As there, at quality 2 on
   text behind a dictionary of the same kind a few in 1000 items are inputs the reference fails on: pass item_results.
   When to set it: hundreds to thousands of small items at these qualities whose dictionaries differ.  Measured (text, lgwin 22,
   every item behind a dictionary of its own; profiles/r21_batch_dictionaries_quick.json): 4096 items of 4 KiB behind 16 KiB each
   at quality 2 / 3 / 4 in 24 .. 26 / 25 .. 27 / 31 .. 33 ms against 3.8 .. 5.4 s for the same call without the bit and 1.8 .. 2.4 s
   for the loop of stream calls from four threads (one CPU core: 0.55 .. 0.63 s); 1024 items of 16 KiB behind 64 KiB each in 34 ..
   45 ms against 1.0 .. 1.6 s; 1024 items of 64 KiB behind 64 KiB each at quality 4 in 146 .. 149 ms against 1.8 .. 1.9 s (5.3 x the
   four threads, 6.1 x one core: the narrowest large shape); 4096 items of 512 bytes behind 16 KiB each in 12 .. 16 ms against
   3.3 .. 4.2 s.  No measured shape loses to the call without the bit or to one CPU core.  When not: a call of a few items -- a
   chain is one wavefront bound by its own dependent loads; 64 items of 4 KiB take 3.5 .. 4.9 ms, 18 x the call without the bit
   but only 2.0 .. 2.4 x one CPU core, and fewer items gain less -- and items that share ONE dictionary, for which
   BrotliMi355xCompressBatchWithDictionaryEx copies one image instead of filing the dictionary per item: self-filing is within
   5 % of it where the item is at least as long as the dictionary, 1.13 .. 1.15 x slower for 4 KiB items behind 16 KiB, and
   1.4 .. 1.6 x slower for 512-byte items behind 16 KiB.
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS (1024; unknown to the other five batch entry points): item i is still exactly
   the stream described above, at quality 10 AND at quality 11 -- through the stream API, which defines these items, both qualities
   are Zopfli (the one-shot entry runs quality 10 as the parse of quality 9, which is why BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS
   takes quality 11 alone; this route takes both).  An item of 1 <= input_sizes[i] <= 65 536 bytes at quality 10 or 11 and lgwin
   10 .. 24 behind a dictionary of dict_sizes[k] >= 2 of which at most 65 536 bytes are in use (min(dict_sizes[k], (1 << lgwin) -
   16)) runs on the device as ONE wavefront: it empties H10 trees of its own, files its item's dictionary into them -- every
   position with 127 bytes behind it, the 64 lanes each owning the hash keys of one class, which leaves exactly the trees of the
   reference's one loop --, stitches, and walks the item the reference's way from position D.  There is no tree image per
   dictionary.  A call in which every item names ONE index has one: it is BrotliMi355xCompressBatchWithDictionaryEx with
   BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS and that dictionary -- the image of its trees is built once per call
   and every chain copies it over its own table instead of filing the dictionary (same bytes; equal info between the calls).  Every
   other item -- the empty one, longer items, dict_sizes[k] <= 1, more than 65 536 bytes in use -- runs by itself through the
   stream path.  The bit changes nothing at qualities 0 .. 9.  Such items count in info[1], their groups (at most 1024 items) in
   info[4]; info[2], info[5] as below; info[6] and info[7] stay 0.  An item on which the reference's quality 10 / 11 parse itself
   fails fails alone ("the reference encoder fails on this input"); none was met in 316 000 drawn pairs.
   Memory: a table per item in flight, at most 256 -- 512 KiB of buckets, 8 bytes of forest per byte of the group's largest
   dictionary + item (at most 8 << lgwin) and about 1.05 KiB per byte of its largest item: 4.8 MiB for 4 KiB items behind 16 KiB,
   17.7 MiB for 16 KiB items behind 64 KiB, 67.8 MiB for 64 KiB items behind 64 KiB.
   When to set it: tens to thousands of small (old version, new file) pairs at the level static files are pre-compressed at.
   Measured (text, lgwin 22, every item behind a dictionary of its own, min .. max of five alternating runs;
   profiles/r27_batch_dictionaries_zopfli.json; the one-by-one baselines timed on 8 items and scaled): 1024 items of 4 KiB behind
   16 KiB each at quality 10 / 11 in 320 .. 321 / 587 .. 588 ms against 67 / 110 .. 112 s for the same call without the bit (the
   parent build), 30 .. 50 / 58 .. 77 s for the loop of stream calls from four threads and 1.8 / 3.9 s on one CPU core; 256 items
   of 16 KiB behind 64 KiB each in 338 / 629 .. 633 ms against 65 .. 66 / 112 .. 114 s (one core 2.0 / 4.2 s); 256 items of 4 KiB
   behind 64 KiB each in 155 .. 159 / 228 .. 229 ms against 43 / 55 s (one core 1.2 / 1.7 s); 64 items of 4 KiB behind 16 KiB each
   in 85 .. 86 / 156 .. 157 ms against 4.2 / 6.9 .. 7.0 s -- and only 1.3 / 1.5 x one CPU core.  When not: a call of a few items --
   a walk is one wavefront and lasts its item's time however many run beside it: 16 items of 4 KiB behind 16 KiB each take 84 ..
   85 / 155 .. 156 ms, 11 .. 12 x faster than without the bit and still LOSE to one CPU core (29 / 61 ms, 0.34 / 0.39 x).  No
   measured shape loses to the call without the bit or to the four-thread loop.  (The wave-wide filing against lane 0 filing the
   dictionary alone inside the same kernel: 1.04 .. 1.08 x faster with 16 KiB dictionaries, 1.32 .. 1.47 x with 64 KiB.)
   BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096; known to this call, its device form and
   BrotliMi355xCompressBatchWithDictionaryEx; an unknown route of BrotliMi355xCompressBatchEx and BrotliMi355xCompressBatchDevice; 2048
   is no route of any call): item i is still exactly the stream described above, at quality 9 -- the strongest greedy level, for
   (old version, new file) pairs where the Zopfli qualities are too slow.  An item of 1 <= input_sizes[i] <= 65 536 bytes at quality
   9 and lgwin 17 .. 24 behind a dictionary of dict_sizes[k] >= 2 of which at most 65 536 bytes are in use (min(dict_sizes[k],
   (1 << lgwin) - 16)) runs on the device as ONE wavefront: a live chain on a private H9 table (64 KiB of ring counters, 32 MiB of
   rings 256 deep; at most 255 tables, 8 GiB, per group) that empties the counters, files its item's dictionary wave-wide in the
   reference's order -- or, where enough items of the group name that dictionary, replays the image the group has built of it
   (BrotliMi355xLastBatchImageInfo below: at most 64 per group, 64 KiB of counters and 8 bytes per dictionary byte each) --,
   stitches, and parses dictionary | item from position D.  Dictionary + item stay inside the first half of the
   smallest ring buffer of these windows, so the chain meets neither a masked position nor H9's ring-end case.  When every item
   names one index -- and in BrotliMi355xCompressBatchWithDictionaryEx, where there is one dictionary -- the chains replay one image
   of the dictionary, made once per call, instead of filing it (same bytes; equal info between the two calls).  Every other item --
   the empty one, longer items, dict_sizes[k] <= 1, more than 65 536 bytes in use, lgwin <= 16 -- runs by itself through the stream
   path.  Without the bit quality 9 runs one by one as before; the bit changes nothing at qualities 0 .. 8, 10 and 11.  Such items
   count in info[1], their groups in info[4]; info[2], info[5] as below; info[6] and info[7] stay 0.  An item on which the
   reference fails (a match cut to one byte at the dictionary's end: "the reference encoder fails on this input") fails alone,
   11 of 4000 drawn pairs; so does one whose stream does not fit; a device error fails the call.
   When to set it: dozens to thousands of small items at quality 9.  Measured (text, lgwin 22, every item behind a dictionary
   of its own, min .. max of five alternating rounds; profiles/r28_batch_dictionaries_q9.json; the one-by-one baselines timed on 32
   items and scaled): 4096 items of 4 KiB behind 16 KiB each in 108 .. 109 ms against 5.8 .. 6.2 s for the same call without the
   bit (the parent build), 5.2 .. 6.4 s for the loop of stream calls from four threads and 10.7 s on one CPU core; 1024 items of
   16 KiB behind 64 KiB each in 108 .. 109 ms against 1.41 .. 1.48 s (loop 1.13 .. 1.39 s, one core 4.4 s); 256 items of 64 KiB
   behind 64 KiB each in 115 .. 116 ms against 388 .. 406 ms (loop 304 .. 375 ms, one core 1.6 s); 64 items of 4 KiB behind 16 KiB
   each in 6.4 .. 6.5 ms against 83 .. 89 ms; 16 of them in 6.3 .. 6.4 ms against 21 .. 22 ms (one core 42 ms).  Behind ONE shared
   16 KiB dictionary 4096 items of 4 KiB take 86 .. 88 ms with the image and 105 .. 107 ms with every chain filing it
   (BROTLI_MI355X_BATCH_DICT_SELF_FILE=1): the image is 1.22 x faster.
   When not: a call of a few items -- a chain is one wavefront and lasts its item's time however many run beside it, about 6 ms
   for 4 KiB behind 16 KiB.  4 such items take 6.2 .. 6.3 ms and LOSE to the call without the bit (5.2 .. 5.5 ms, 0.84 x); 1 item
   takes 6.1 .. 6.2 ms against 1.3 .. 1.4 ms (0.21 x) and loses to one CPU core as well (2.7 ms, 0.44 x).  Few long items lose too:
   16 items of 64 KiB behind 64 KiB each take 65 .. 66 ms against 23 .. 25 ms without the bit (0.36 x) and 28 .. 34 ms for the
   four-thread loop (0.47 x).  The break-even lies between 4 and 16 items of 4 KiB, and between 16 and 256 items of 64 KiB.
   Side by side on the device: quality 5 .. 8, lgwin 17 .. 24, 2 <= D_i <= 65536 (the bytes of the item's dictionary in use) and
   1 <= input_sizes[i] <= 65536.  A group uploads its items and, once each, the dictionaries they name; the text
   dictionary | item is laid out on the device per item, and one chain per item parses the item on a private hash table that holds
   the item's dictionary.  A dictionary that at least BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS (default 16) items of a device group
   name gets an image of what the reference's prepend leaves in a hash table, built once for that group from the dictionary's copy
   in front of the first item that names it; the chains of those items replay the image, as the chains behind one shared
   dictionary do.  At most 64 images per group, the most named dictionaries first; an image is 32 KiB of ring counters (64 KiB at
   quality 9) and 8 bytes per dictionary byte.  Every other chain files its dictionary itself, so its time grows with
   D_i + input_sizes[i].  BrotliMi355xLastBatchImageInfo tells what a call did.  Every other item -- other qualities and windows, the empty item, longer items, longer or
   shorter dictionaries -- is accepted and runs by itself through the stream path with its own dictionary, on the calling thread,
   in the same call and in the caller's order: the same bytes, no gain in speed.  info[0] .. info[4] mean what they mean for
   BrotliMi355xCompressBatchWithDictionary; info[5] is the sum of the dictionary bytes in use over the distinct indices that at
   least one item names; info[6] and info[7] stay 0.  When every item names one and the same index the call IS
   BrotliMi355xCompressBatchWithDictionary with that dictionary (same bytes, same info, the shared image).  The environment of
   BrotliMi355xCompressBatch applies; a group's byte limit counts every item's dictionary.
   When to use it: hundreds to thousands of small items in a call whose dictionaries differ.  When not: items that all share
   one dictionary (BrotliMi355xCompressBatchWithDictionary: its chains replay one image instead of filing 64 KiB each), and calls of
   a few items -- a chain is one wavefront bound by its own dependent loads.  Measured (text, lgwin 22, every
   item behind a dictionary of its own, qualities 5 .. 8; profiles/r20_batch_dictionaries.json): 4096 items of 4 KiB behind 16 KiB each at quality 5
   in 26 ms against 5.6 s for the loop of stream calls and 2.4 s from four threads (one CPU core: 0.80 s), at quality 8 in 63 ms;
   1024 items of 16 KiB behind 64 KiB each in 39 / 68 ms at quality 5 / 8 against 1.4 / 1.7 s (four threads 0.64 / 0.68 s); 64 items
   of 4 KiB behind 16 KiB each in 4.7 / 6.1 ms against 88 / 97 ms -- and only 2.7 / 3.6 x one CPU core.  No measured shape loses to
   the loop or to one core.  Against the shared image, on the same items behind ONE dictionary given as count indices: level at
   4 KiB of dictionary, 1.14 .. 1.22 x slower at 16 KiB with 4 KiB items, 1.20 x at 64 KiB with 16 KiB items. */
/* known to BrotliMi355xCompressBatchWithDictionaries and its device form only; 4u and 256u stay unknown routes of this call */
#define BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS 512u
/* known to BrotliMi355xCompressBatchWithDictionaries and its device form only, like 512u; may be combined with it (a call has one
   quality, so at most one of the two takes items) */
#define BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS 1024u
/* known to BrotliMi355xCompressBatchWithDictionaryEx, BrotliMi355xCompressBatchWithDictionaries and its device form; an unknown
   route of BrotliMi355xCompressBatchEx and BrotliMi355xCompressBatchDevice.  (2048u is taken by no route and stays unknown.) */
#define BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS 4096u
/* known to BrotliMi355xCompressBatchWithDictionaryEx only: there it is what 1024u is here, as 4u there is what 512u is here.  An
   unknown route of this call, of its device form and of every other batch entry point. */
#define BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS 8192u
int32_t BrotliMi355xCompressBatchWithDictionaries(int quality, int lgwin, BrotliEncoderMode mode, uint32_t routes, size_t num_dicts,
                                                  const uint8_t* const* dicts, const size_t* dict_sizes, size_t count,
                                                  const size_t* item_dicts /* may be NULL */, const uint8_t* const* inputs,
                                                  const size_t* input_sizes, uint8_t* const* outputs,
                                                  size_t* output_sizes /* in: capacity, out: size */,
                                                  int32_t* item_results /* may be NULL */);
/* BrotliMi355xCompressBatchWithDictionaries on device memory: items and dictionaries that lie in device memory -- the new and the
   previous version of many resources, say -- and their streams left in device memory.  It is that call in every respect but one:
   dicts_device[k], inputs_device[i] and outputs_device[i] are device addresses on the calling thread's current device, with any
   alignment; several may point into one allocation.  All the arrays themselves (dicts_device, dict_sizes, item_dicts,
   inputs_device, input_sizes, outputs_device, output_sizes) and item_results are host memory, as there.
   Per item: the same bytes, size, success or failure as the host call on the same bytes -- item i is the stream of
   BrotliEncoderSetCustomDictionary(<the bytes at dicts_device[item_dicts[i]]>) followed by one FINISH, under the stream API's rules:
   no size hint, NO fallback to a stored stream and no BrotliEncoderMaxCompressedSize cap (an item goes out if and only if its
   stream fits its capacity, otherwise it fails alone with size 0), a dictionary cut to its last (1 << lgwin) - 16 bytes, no
   dictionary taken with dict_sizes[k] <= 1 or at qualities 0 and 1.  The rules of the call are the host call's: `routes` knows
   BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS and BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS only; item_dicts == NULL means item i takes dicts_device[i] and num_dicts must be
   count; any other route bit, an index >= num_dicts, or item_dicts == NULL with num_dicts != count fails the whole call before any
   work is done (returns 0, every size 0, only info[0] set, nothing written to device memory); when every item names one index the
   call takes the shared-image path (the shared route of qualities 5 .. 8, with their bits the quick shared route and the shared
   route of quality 9, and with its bit the Zopfli route of qualities 10 / 11, whose image is the dictionary's H10 trees), the dictionary reaching its image by one copy on the device; BrotliMi355xLastBatchInfo means what it means for the host call and has the same
   values on the same data; BrotliMi355xLastError carries "the reference encoder fails on this input" for the items that fail that way.
   On the side-by-side routes (info[1]) nothing crosses the bus: one launch per group reads every item and every dictionary
   where it lies -- no page-locked staging, no dictionary pool, no upload -- and lays out dictionary | item per item on the device;
   one launch scatters the group's streams to their addresses.  Every other item -- the empty one, items longer than one input
   block, other qualities or windows, dict_sizes[k] <= 1, more than 65 536 dictionary bytes in use, qualities 2 .. 4, 9 and 10 / 11
   without their bits -- is downloaded, the bytes in use of the dictionary it names are downloaded once per call however many items name it, the item
   runs through the stream path in the caller's order and its stream is uploaded if it fits: the same bytes and the same info as the
   host call, and no gain over it.  If every item of a call goes this way no dictionary is touched on the device but by these downloads.
   Memory contract.  The library reads only the aligned 4-byte words that hold at least one byte of an item or of the part of a
   dictionary in use: it never reads the bytes in front of a truncated dictionary's last (1 << lgwin) - 16 (beyond the word that
   holds the first byte in use), and never behind the last word of an item or a dictionary.  On return it has written exactly
   outputs_device[i][0 .. output_sizes[i]), and never a byte outside [0, capacity); an item that fails leaves the contents of its
   buffer unspecified, but stays inside it.  Outputs must not overlap each other, any input or any dictionary; they may abut.
   Inputs and dictionaries may overlap each other freely: an item may lie behind a dictionary that is the previous item.
   Ordering.  As for BrotliMi355xCompressBatchDevice: the call works on the calling thread's stream and returns after everything it
   wrote has landed (one synchronisation at the end); whatever produced the inputs and dictionaries must be complete before it.
   When to use it: when both versions already lie in device memory, or the streams are wanted there.
   Measured on an MI355X against the same job done the way there was before -- dictionaries and items down to page-locked memory, the
   parent commit's BrotliMi355xCompressBatchWithDictionaries, the streams up -- min .. max of five alternating runs, text, lgwin 22
   (profiles/r24_batch_dictionaries_device.json): 4096 items of 4 KiB behind 16 KiB each at quality 5 in 17.0 .. 17.3 ms against
   25.1 .. 26.0 ms (the host call alone, from page-locked memory: 23.1 .. 23.8 ms), at quality 2 with
   BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS 16.0 .. 16.3 against 24.0 .. 25.2 ms; 1024 items of 16 KiB behind 64 KiB each at
   quality 5 31.6 .. 31.7 against 38.6 .. 39.0 ms; 4096 items of 4 KiB behind ONE shared 16 KiB dictionary 15.6 .. 15.9 against
   18.5 .. 18.7 ms.  No measured shape is slower.  When not: a call of a few items -- 64 items of 4 KiB behind 16 KiB each take
   4.55 .. 4.60 ms against 4.68 .. 4.73 ms, launches and round trips either way -- and the items that run one by one, which are staged
   through the host by the call itself. */
int32_t BrotliMi355xCompressBatchWithDictionariesDevice(int quality, int lgwin, BrotliEncoderMode mode, uint32_t routes, size_t num_dicts,
                                                        const uint8_t* const* dicts_device, const size_t* dict_sizes, size_t count,
                                                        const size_t* item_dicts /* may be NULL */, const uint8_t* const* inputs_device,
                                                        const size_t* input_sizes, uint8_t* const* outputs_device,
                                                        size_t* output_sizes /* in: capacity, out: size */,
                                                        int32_t* item_results /* may be NULL */);
/* The last BrotliMi355xCompressBatch / BrotliMi355xCompressBatchEx / BrotliMi355xCompressBatchWithDictionary /
   BrotliMi355xCompressBatchWithDictionaryEx / BrotliMi355xCompressBatchWithDictionaries call (or device form of one) of the calling
   thread: info[0] items, [1] items encoded side by side on the device, [2] items run one by one (the one-shot path; with a
   dictionary the stream path), [3] items answered without an encoder (empty input, capacity 0; none with a dictionary), [4] device
   groups (those of long items included), [5] dictionary bytes in use after the reference's truncation (0 for the plain call; with a
   dictionary per item their sum over the indices named),
   [6] items that began side by side and were redone one by one (counted in [2], not in [1]), [7] of the items counted in [1],
   those longer than one input block; [6] and [7] are zero unless BrotliMi355xCompressBatchEx was called with
   BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS or BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS (the items of
   BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS, BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS and BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS count in
   [1] and [4] only).  After a call that failed as a whole only info[0] is set. */
void BrotliMi355xLastBatchInfo(uint64_t info[8]);
/* The dictionary images of the same call.  Behind a dictionary per item (BrotliMi355xCompressBatchWithDictionaries and its device
   form; qualities 5 .. 8, and 2 .. 4 / 9 with their bits) a dictionary that at least BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS
   side-by-side items of a device group name gets an image of what the reference's prepend leaves in a hash table, built once for
   that group; the chains of those items replay it instead of filing the dictionary, every other chain files its own.  The variable
   is read once per process; its default is 16, 0 means no images, and a dictionary that one item of a group names never gets one
   whatever the value (BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 means no images either, also for the shared calls).  A group builds at
   most 64 images, the most named dictionaries first, ties to the one that appears first in the group; dictionaries are told apart by
   pointer and size in use.  The streams, sizes, failures and BrotliMi355xLastBatchInfo do not depend on any of this.
   Measured (text, lgwin 22, 4096 items of 4 KiB dealt round robin to K dictionaries of 16 KiB, min .. max of two alternating
   rounds against the parent build through the same call; profiles/r30_batch_dictionaries_images.json): K = 4 .. 64 at quality 8
   in 50 .. 54 against 59 .. 63 ms, at quality 2 / 4 in 17 .. 18 / 24 .. 26 against 20 .. 21 / 27 .. 28 ms, at quality 9 in 86 .. 89
   against 103 .. 105 ms, within 1 .. 4 % of the shared call behind ONE dictionary; 512-byte items behind 16 dictionaries at
   quality 2 in 4.6 .. 5.6 against 7.6 .. 8.1 ms.  K = 4096 builds nothing and stays inside the parent's spread.  When not:
   quality 5, where a replay costs a chain about what filing 16 KiB does -- level with the parent at K <= 64, and SLOWER with many
   dictionaries of a few dozen items each: K = 128 in 22.1 .. 23.9 against 20.7 .. 22.7 ms (0.95 x), and K = 256 under a
   threshold of 2 in 23.8 .. 25.3 against 21.3 .. 22.7 ms (0.89 x; the default of 16 builds nothing there).  Such a call sets the
   variable to 0.  The default is the top of the allowed range because the sweep found no smaller value that never loses; the
   image build's own time was not measured.
   out[0] images built, summed over the call's groups (a shared-dictionary call: 1 when it built its one image), [1] side-by-side
   items whose chain replayed an image, [2] side-by-side items whose chain filed its own dictionary (all of them on the Zopfli
   per-item route, which builds no image per dictionary), [3] 0, reserved.  All zeros after a call without a dictionary and after a
   call that failed as a whole; items that run one by one count in neither [1] nor [2]. */
void BrotliMi355xLastBatchImageInfo(uint64_t out[4]);
/* Human-readable description of the device backing the library ("hip:gfx950 (...)"). */
const char* BrotliMi355xDeviceName(void);
/* Message of the last failure on the calling thread ("" if none). */
const char* BrotliMi355xLastError(void);

/* ---- BroCatli: concatenation of catable / appendable brotli streams, fed and drained piecewise --------------------
 * c/brotli/broccoli.h, src/ffi/broccoli.rs:55-175 (state machine src/concat/mod.rs:274-608).  Same names, signatures
 * and result codes as the reference; the state object is the same 256-byte by-value struct. */
typedef struct BroccoliState_ {
  void* unused;
  unsigned char data[248];
} BroccoliState;

typedef enum BroccoliResult_ {
  BroccoliSuccess = 0,
  BroccoliNeedsMoreInput = 1,
  BroccoliNeedsMoreOutput = 2,
  BroccoliBrotliFileNotCraftedForAppend = 124,
  BroccoliInvalidWindowSize = 125,
  BroccoliWindowSizeLargerThanPreviousFile = 126,
  BroccoliBrotliFileNotCraftedForConcatenation = 127
} BroccoliResult;

BroccoliState BroccoliCreateInstance(void);                                   /* broccoli.rs:56 */
BroccoliState BroccoliCreateInstanceWithWindowSize(uint8_t window_size);      /* broccoli.rs:60 */
void BroccoliDestroyInstance(BroccoliState state);                            /* broccoli.rs:67 */
void BroccoliNewBrotliFile(BroccoliState* state);                             /* broccoli.rs:70 */
BroccoliResult BroccoliConcatStream(BroccoliState* state, size_t* available_in, const uint8_t** input_buf_ptr,
                                    size_t* available_out, uint8_t** output_buf_ptr);  /* broccoli.rs:82 */
BroccoliResult BroccoliConcatStreaming(BroccoliState* state, size_t* available_in, const uint8_t* input_buf,
                                       size_t* available_out, uint8_t* output_buf);    /* broccoli.rs:110 */
BroccoliResult BroccoliConcatFinish(BroccoliState* state, size_t* available_out, uint8_t** output_buf);   /* broccoli.rs:133 */
BroccoliResult BroccoliConcatFinished(BroccoliState* state, size_t* available_out, uint8_t* output_buf);  /* broccoli.rs:156 */

/* returns the device memory the calling thread's encoder calls have pooled (and do not use at the moment) to the
 * driver; the number of bytes released.  Not part of the reference ABI. */
size_t BrotliMi355xTrimPool(void);

#ifdef __cplusplus
}
#endif
#endif /* BROTLI_MI355X_H_ */
