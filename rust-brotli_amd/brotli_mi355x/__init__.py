"""brotli_mi355x -- Python host-side binding of the MI355X brotli encoder library (C ABI via ctypes).

Mirrors the encoder half of the reference's own ctypes binding (c/py/brotli.py:67-195): same function
names, argument meaning and error behaviour (BrotliCompress, BrotliEncoderCompressWorkPool,
BrotliEncoderCreateWorkPool, BrotliEncoderMaxCompressedSizeMulti, BrotliEncoderVersion), plus a
streaming class over BrotliEncoderCompressStream and helpers for device-resident buffers / multi-GPU
chunking that the reference does not have.

The library is HIP only: there is no CPU fallback.  Importing fails loudly if the shared object has
not been built, and every call fails loudly (BrotliCompressorException) if no gfx950 device is usable.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int32, c_size_t, c_uint32, c_uint64, c_void_p


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BROTLI_MI355X_LIB") or os.path.join(os.path.dirname(_HERE), "libbrotli_mi355x.so")  # (the override is for profiling builds)

# BrotliEncoderParameter ids (c/brotli/encode.h:138-232)
BROTLI_PARAM_MODE = 0
BROTLI_PARAM_QUALITY = 1
BROTLI_PARAM_LGWIN = 2
BROTLI_PARAM_LGBLOCK = 3
BROTLI_PARAM_DISABLE_LITERAL_CONTEXT_MODELING = 4
BROTLI_PARAM_SIZE_HINT = 5
BROTLI_PARAM_LARGE_WINDOW = 6
BROTLI_PARAM_CATABLE = 167
BROTLI_PARAM_APPENDABLE = 168
BROTLI_PARAM_MAGIC_NUMBER = 169
BROTLI_PARAM_BYTE_ALIGN = 172
BROTLI_PARAM_BARE_STREAM = 173
BROTLI_OPERATION_PROCESS = 0
BROTLI_OPERATION_FLUSH = 1
BROTLI_OPERATION_FINISH = 2
BROTLI_OPERATION_EMIT_METADATA = 3


class BrotliCompressorException(Exception):
    pass


def _bind(lib):
    lib.BrotliEncoderVersion.restype = c_uint32
    lib.BrotliEncoderMaxCompressedSize.restype = c_size_t
    lib.BrotliEncoderMaxCompressedSize.argtypes = [c_size_t]
    lib.BrotliEncoderMaxCompressedSizeMulti.restype = c_size_t
    lib.BrotliEncoderMaxCompressedSizeMulti.argtypes = [c_size_t, c_size_t]
    lib.BrotliEncoderCreateInstance.restype = c_void_p
    lib.BrotliEncoderCreateInstance.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.BrotliEncoderDestroyInstance.restype = None
    lib.BrotliEncoderDestroyInstance.argtypes = [c_void_p]
    lib.BrotliEncoderSetParameter.restype = c_int
    lib.BrotliEncoderSetParameter.argtypes = [c_void_p, c_int, c_uint32]
    lib.BrotliEncoderSetCustomDictionary.restype = None
    lib.BrotliEncoderSetCustomDictionary.argtypes = [c_void_p, c_size_t, c_char_p]
    lib.BrotliEncoderCompressStream.restype = c_int
    lib.BrotliEncoderCompressStream.argtypes = [c_void_p, c_int, POINTER(c_size_t), POINTER(c_void_p), POINTER(c_size_t),
                                                POINTER(c_void_p), POINTER(c_size_t)]
    lib.BrotliEncoderIsFinished.restype = c_int
    lib.BrotliEncoderIsFinished.argtypes = [c_void_p]
    lib.BrotliEncoderHasMoreOutput.restype = c_int
    lib.BrotliEncoderHasMoreOutput.argtypes = [c_void_p]
    lib.BrotliEncoderTakeOutput.restype = c_void_p
    lib.BrotliEncoderTakeOutput.argtypes = [c_void_p, POINTER(c_size_t)]
    lib.BrotliEncoderCompress.restype = c_int
    lib.BrotliEncoderCompress.argtypes = [c_int, c_int, c_int, c_size_t, c_char_p, POINTER(c_size_t), c_char_p]
    lib.BrotliEncoderCompressMulti.restype = c_int32
    lib.BrotliEncoderCompressMulti.argtypes = [c_size_t, POINTER(c_int), POINTER(c_uint32), c_size_t, c_char_p,
                                               POINTER(c_size_t), c_char_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.BrotliEncoderCreateWorkPool.restype = c_void_p
    lib.BrotliEncoderCreateWorkPool.argtypes = [c_size_t, c_void_p, c_void_p, c_void_p]
    lib.BrotliEncoderDestroyWorkPool.restype = None
    lib.BrotliEncoderDestroyWorkPool.argtypes = [c_void_p]
    lib.BrotliEncoderCompressWorkPool.restype = c_int32
    lib.BrotliEncoderCompressWorkPool.argtypes = [c_void_p, c_size_t, POINTER(c_int), POINTER(c_uint32), c_size_t, c_char_p,
                                                  POINTER(c_size_t), c_char_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.BrotliMi355xCompressChunk.restype = c_int32
    lib.BrotliMi355xCompressChunk.argtypes = [c_size_t, POINTER(c_int), POINTER(c_uint32), c_size_t, c_void_p, c_int,
                                              c_size_t, c_size_t, POINTER(c_size_t), c_char_p]
    lib.BrotliMi355xConcatChunks.restype = c_int32
    lib.BrotliMi355xConcatChunks.argtypes = [c_size_t, POINTER(c_char_p), POINTER(c_size_t), POINTER(c_size_t), c_char_p]
    lib.BrotliMi355xConcatChunkEnds.restype = c_int32
    lib.BrotliMi355xConcatChunkEnds.argtypes = [c_size_t, c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_size_t), c_void_p, POINTER(c_size_t)]
    lib.BrotliMi355xCompressDevice.restype = c_int
    lib.BrotliMi355xCompressDevice.argtypes = [c_int, c_int, c_int, c_size_t, c_void_p, POINTER(c_size_t), c_char_p,
                                               POINTER(c_double)]
    lib.BrotliMi355xCompressBatch.restype = c_int32
    lib.BrotliMi355xCompressBatch.argtypes = [c_int, c_int, c_int, c_size_t, POINTER(c_char_p), POINTER(c_size_t), POINTER(c_void_p),
                                              POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchWithDictionary"):  # (absent from libraries built before the call existed)
        lib.BrotliMi355xCompressBatchWithDictionary.restype = c_int32
        lib.BrotliMi355xCompressBatchWithDictionary.argtypes = [c_int, c_int, c_int, c_size_t, c_char_p, c_size_t, POINTER(c_char_p), POINTER(c_size_t),
                                                                POINTER(c_void_p), POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchEx"):
        lib.BrotliMi355xCompressBatchEx.restype = c_int32
        lib.BrotliMi355xCompressBatchEx.argtypes = [c_int, c_int, c_int, c_uint32, c_size_t, POINTER(c_char_p), POINTER(c_size_t), POINTER(c_void_p),
                                                    POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchWithDictionaryEx"):
        lib.BrotliMi355xCompressBatchWithDictionaryEx.restype = c_int32
        lib.BrotliMi355xCompressBatchWithDictionaryEx.argtypes = [c_int, c_int, c_int, c_uint32, c_size_t, c_char_p, c_size_t, POINTER(c_char_p),
                                                                  POINTER(c_size_t), POINTER(c_void_p), POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchWithDictionaries"):
        lib.BrotliMi355xCompressBatchWithDictionaries.restype = c_int32
        lib.BrotliMi355xCompressBatchWithDictionaries.argtypes = [c_int, c_int, c_int, c_uint32, c_size_t, POINTER(c_char_p), POINTER(c_size_t), c_size_t,
                                                                  POINTER(c_size_t), POINTER(c_char_p), POINTER(c_size_t), POINTER(c_void_p),
                                                                  POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchDevice"):
        lib.BrotliMi355xCompressBatchDevice.restype = c_int32
        lib.BrotliMi355xCompressBatchDevice.argtypes = [c_int, c_int, c_int, c_uint32, c_size_t, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p),
                                                        POINTER(c_size_t), POINTER(c_int32)]
    if hasattr(lib, "BrotliMi355xCompressBatchWithDictionariesDevice"):
        lib.BrotliMi355xCompressBatchWithDictionariesDevice.restype = c_int32
        lib.BrotliMi355xCompressBatchWithDictionariesDevice.argtypes = [c_int, c_int, c_int, c_uint32, c_size_t, POINTER(c_void_p), POINTER(c_size_t),
                                                                        c_size_t, POINTER(c_size_t), POINTER(c_void_p), POINTER(c_size_t),
                                                                        POINTER(c_void_p), POINTER(c_size_t), POINTER(c_int32)]
    lib.BrotliMi355xDeviceName.restype = c_char_p
    lib.BrotliMi355xLastError.restype = c_char_p
    return lib


class Library(object):
    """All entry points bound to one shared object (the product library by default)."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise ImportError("%s is missing; build it with `make -C rust-brotli_amd` (or __graft_entry__.build()). "
                              "There is no CPU fallback." % path)
        self.path = path
        self.lib = _bind(ctypes.CDLL(path))

    # ---- c/py/brotli.py:54 ----
    def BrotliEncoderVersion(self):
        return self.lib.BrotliEncoderVersion()

    def BrotliEncoderMaxCompressedSizeMulti(self, input_size, num_threads):
        return self.lib.BrotliEncoderMaxCompressedSizeMulti(input_size, num_threads)

    def device_name(self):
        return self.lib.BrotliMi355xDeviceName().decode()

    def last_error(self):
        return self.lib.BrotliMi355xLastError().decode()

    @staticmethod
    def _options(compression_options_map):
        items = list(compression_options_map.items()) if hasattr(compression_options_map, "items") else list(compression_options_map)
        keys = (c_int * max(1, len(items)))(*[int(k) for k, _ in items])
        vals = (c_uint32 * max(1, len(items)))(*[int(v) for _, v in items])
        return len(items), keys, vals

    # ---- c/py/brotli.py:155-195 ----
    def BrotliCompress(self, any_input, compression_options_map={}, num_threads=4):
        data = bytes(any_input)
        n, keys, vals = self._options(compression_options_map)
        max_size = self.lib.BrotliEncoderMaxCompressedSizeMulti(len(data), num_threads)
        encoded = ctypes.create_string_buffer(max_size)
        encoded_size = c_size_t(max_size)
        ret = self.lib.BrotliEncoderCompressMulti(n, keys, vals, len(data), data, byref(encoded_size), encoded, num_threads,
                                                  None, None, None)
        if ret == 0:
            raise BrotliCompressorException("Insufficient space %d to compress %d bytes with %d threads (%s)" %
                                            (max_size, len(data), num_threads, self.last_error()))
        return bytearray(encoded.raw[:encoded_size.value])

    # ---- c/py/brotli.py:67-121 ----
    def BrotliEncoderCreateWorkPool(self, num_workers):
        return self.lib.BrotliEncoderCreateWorkPool(num_workers, None, None, None)

    def BrotliEncoderDestroyWorkPool(self, pool):
        self.lib.BrotliEncoderDestroyWorkPool(pool)

    def BrotliEncoderCompressWorkPool(self, work_pool, any_input, compression_options_map={}, num_threads=4):
        data = bytes(any_input)
        n, keys, vals = self._options(compression_options_map)
        max_size = self.lib.BrotliEncoderMaxCompressedSizeMulti(len(data), num_threads)
        encoded = ctypes.create_string_buffer(max_size)
        encoded_size = c_size_t(max_size)
        ret = self.lib.BrotliEncoderCompressWorkPool(work_pool, n, keys, vals, len(data), data, byref(encoded_size), encoded,
                                                     num_threads, None, None, None)
        if ret == 0:
            raise BrotliCompressorException("Insufficient space %d to compress %d bytes with %d threads (%s)" %
                                            (max_size, len(data), num_threads, self.last_error()))
        return bytearray(encoded.raw[:encoded_size.value])

    # ---- one-shot BrotliEncoderCompress (c/brotli/encode.h:318) ----
    def compress(self, data, quality=5, lgwin=22, mode=0):
        data = bytes(data)
        cap = self.lib.BrotliEncoderMaxCompressedSize(len(data)) + 16
        out = ctypes.create_string_buffer(cap)
        n = c_size_t(cap)
        if not self.lib.BrotliEncoderCompress(quality, lgwin, mode, len(data), data, byref(n), out):
            raise BrotliCompressorException("BrotliEncoderCompress failed: " + self.last_error())
        return ctypes.string_at(out, n.value)

    BATCH_ROUTE_LONG_ITEMS = 1  # BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS
    BATCH_ROUTE_QUICK_ITEMS = 4  # BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS (2 is reserved)
    BATCH_ROUTE_QUICK_LONG_ITEMS = 16  # BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS (8 is reserved)
    BATCH_ROUTE_ZOPFLI_ITEMS = 32  # BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS
    BATCH_ROUTE_Q9_ITEMS = 128  # BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS (64 is reserved)
    BATCH_ROUTE_QUICK_DICTIONARY_ITEMS = 512  # BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS (compress_batch_with_dictionaries only)
    BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS = 1024  # BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS (compress_batch_with_dictionaries only)
    BATCH_ROUTE_Q9_DICTIONARY_ITEMS = 4096  # BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (the dictionary calls, shared and per item; 2048 is no route)
    BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS = 8192  # BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (compress_batch_with_dictionary only)

    def compress_batch(self, items, quality=0, lgwin=22, mode=0, dictionary=None, long_items=False, quick_items=False, quick_long_items=False,
                       zopfli_items=False, q9_items=False):
        """BrotliMi355xCompressBatch: every item becomes a stream of its own, the same bytes as compress(item, quality, lgwin,
        mode), in one call.  Side by side on the device (the call for many small payloads): every item at qualities 0 and 1, and
        at qualities 5 to 8 the items of at most 65 536 bytes at lgwin 17 to 24.  Everything else runs item by item in the same
        call; last_batch_info() tells how the items of the last call were taken.  Returns a list of bytes.

        dictionary (bytes): BrotliMi355xCompressBatchWithDictionary -- every item is the stream of an Encoder(params, dictionary)
        that gets the item in one finish(); a decoder needs the same dictionary.  Side by side at qualities 5 to 8, lgwin 17 to 24,
        a dictionary of 2 to 65 536 bytes and items of 1 to 65 536 bytes.

        long_items=True: BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS -- at qualities 5 to 8 and lgwin 17
        to 24 the items of 65 537 to 262 144 bytes run side by side as well, one chain each (the same bytes).  It pays with many
        such items in a call; a few dozen long items of text are faster without it.  Not combined with a dictionary.

        quick_items=True: BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS -- at qualities 2 to 4 and lgwin 10
        to 24 the items of at most one input block (16 384 bytes at quality 2 and 3, 65 536 at quality 4) run side by side, one
        chain on a private hash table each (the same bytes).  Without it these qualities run item by item; longer items at these
        qualities still do.  It pays with hundreds of small items in a call.  May be combined with long_items, not with a
        dictionary (that is compress_batch_with_dictionary(..., quick_items=True)).

        quick_long_items=True: BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS -- at qualities 2 to 4 and
        lgwin 10 to 24 the items of more than one and at most four input blocks (16 385 to 65 536 bytes at quality 2 and 3, 65 537
        to 262 144 at quality 4) run side by side, one chain each that walks from block to block (the same bytes).  Independent of
        quick_items: alone it takes these items only, together they take both.  A chain is one wavefront, so such an item takes a
        lone chain's time however many run beside it: it pays with many such items in a call.  Not combined with a dictionary.

        zopfli_items=True: BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS -- at quality 11 and lgwin 10 to
        24 the items of at most 65 536 bytes run side by side, one wavefront each that walks the item the reference's way on H10
        trees of its own (the same bytes).  Without it this quality runs item by item; quality 10 is not taken by it (compress() runs it
        at quality 9, as the reference's one-shot entry does).  A walk takes a lone walk's time however many run beside it (about
        37 us per byte): it pays with hundreds of small items in a call (pre-compressing static files: 1024 items of 4 KiB in
        0.6 s against 89 s); for one or two items the one-by-one path is as fast or faster.  May be combined with the other
        flags, not with a dictionary.

        q9_items=True: BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS -- at qualities 9 and 10 and lgwin 17 to
        24 the items of at most one input block (131 072 bytes at lgwin 17, 262 144 from lgwin 18 on) run side by side, one chain
        each on a private H9 hash table of 32 MiB (the same bytes; quality 10 is quality 9 for compress(), as for the reference's
        one-shot entry).  Without it these qualities run item by item.  A chain takes a lone chain's time however many run beside it (about
        1 us per byte of text): it pays with dozens to thousands of small items in a call (4096 items of 4 KiB in 0.10 s against
        6.8 s, 16 of them in 6.7 ms against 26 ms); 64 items of 256 KiB of text lose (258 ms against 142 ms), as do one or two
        items of any size.  May be combined with the other flags (with
        zopfli_items quality 10 goes this way and quality 11 the Zopfli way), not with a dictionary."""
        if q9_items and dictionary is not None:
            raise ValueError("q9_items and dictionary cannot be combined: BrotliMi355xCompressBatchWithDictionary has no routes")
        if zopfli_items and dictionary is not None:
            raise ValueError("zopfli_items and dictionary cannot be combined: BrotliMi355xCompressBatchWithDictionary has no routes")
        if quick_long_items and dictionary is not None:
            raise ValueError("quick_long_items and dictionary cannot be combined: BrotliMi355xCompressBatchWithDictionary has no routes")
        if long_items and dictionary is not None:
            raise ValueError("long_items and dictionary cannot be combined: BrotliMi355xCompressBatchWithDictionary has no routes")
        if quick_items and dictionary is not None:
            raise ValueError("quick_items and dictionary cannot be combined: BrotliMi355xCompressBatchWithDictionary has no routes "
                             "(compress_batch_with_dictionary(..., quick_items=True) calls BrotliMi355xCompressBatchWithDictionaryEx)")
        routes = (self.BATCH_ROUTE_LONG_ITEMS if long_items else 0) | (self.BATCH_ROUTE_QUICK_ITEMS if quick_items else 0)
        routes |= self.BATCH_ROUTE_QUICK_LONG_ITEMS if quick_long_items else 0
        routes |= self.BATCH_ROUTE_ZOPFLI_ITEMS if zopfli_items else 0
        routes |= self.BATCH_ROUTE_Q9_ITEMS if q9_items else 0
        if dictionary is not None:
            dictionary = bytes(dictionary)

        def call(count, inputs, in_sizes, outputs, out_sizes, results):
            if routes:
                return "BrotliMi355xCompressBatchEx", self.lib.BrotliMi355xCompressBatchEx(quality, lgwin, mode, routes, count, inputs, in_sizes, outputs,
                                                                                           out_sizes, results)
            if dictionary is None:
                return "BrotliMi355xCompressBatch", self.lib.BrotliMi355xCompressBatch(quality, lgwin, mode, count, inputs, in_sizes, outputs, out_sizes, results)
            return "BrotliMi355xCompressBatchWithDictionary", self.lib.BrotliMi355xCompressBatchWithDictionary(
                quality, lgwin, mode, len(dictionary), dictionary, count, inputs, in_sizes, outputs, out_sizes, results)

        # (the stream API has no fallback to a stored stream at BrotliEncoderMaxCompressedSize: room beyond it)
        return self._batch(items, 16 if dictionary is None else 1024, call)

    def _batch(self, items, room, call):
        """The buffers of a batch call, the call, its streams: every item gets BrotliEncoderMaxCompressedSize + `room` bytes;
        call(count, inputs, in_sizes, outputs, out_sizes, results) -> (entry name, return value).  Where the call returns 0 the
        exception carries what it left: .failed (the indices of the items that failed) and .streams (the streams of the others,
        None for a failed item; all None after a call that failed as a whole)."""
        items = [bytes(x) for x in items]
        count = len(items)
        if count == 0:
            return []
        sizes = [len(x) for x in items]
        caps = [self.lib.BrotliEncoderMaxCompressedSize(n) + room for n in sizes]
        starts = [0] * count
        at = 0
        for i, cap in enumerate(caps):
            starts[i] = at
            at += (cap + 15) & ~15
        out = ctypes.create_string_buffer(at)
        base = ctypes.addressof(out)
        inputs = (c_char_p * count)(*items)
        in_sizes = (c_size_t * count)(*sizes)
        outputs = (c_void_p * count)(*[base + s for s in starts])
        out_sizes = (c_size_t * count)(*caps)
        results = (c_int32 * count)()
        name, ok = call(count, inputs, in_sizes, outputs, out_sizes, results)
        view = memoryview(out)
        streams = [bytes(view[starts[i]:starts[i] + out_sizes[i]]) if ok or results[i] else None for i in range(count)]
        if not ok:
            failed = [i for i in range(count) if not results[i]]
            e = BrotliCompressorException("%s failed (items %s): %s" % (name, failed[:8], self.last_error()))
            e.failed, e.streams = failed, streams
            raise e
        return streams

    def compress_batch_with_dictionary(self, items, dictionary, quality=5, lgwin=22, mode=0, quick_items=False, q9_items=False, zopfli_items=False):
        """BrotliMi355xCompressBatchWithDictionaryEx: every item is the stream of an Encoder(params, dictionary) that gets the item
        in one finish(), as compress_batch(..., dictionary=dictionary) gives it; a decoder needs the same dictionary.  Returns a
        list of bytes.

        quick_items=False: BrotliMi355xCompressBatchWithDictionary in every respect -- side by side at qualities 5 to 8 only.

        quick_items=True: BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS -- at qualities 2 to 4 and lgwin 10 to 24 the items of at most one
        input block (16 384 bytes at quality 2 and 3, 65 536 at quality 4) behind a dictionary of at least 2 bytes, of which at
        most 65 536 are in use, run side by side, one chain each on a private hash table that starts as the dictionary's (the same
        bytes).  Without it these qualities run item by item; longer items and the empty item still do.  It pays with hundreds of
        small items of one kind in a call, not with a few: a chain is one wavefront.

        q9_items=True: BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS -- at quality 9 and lgwin 17 to 24 the items of 1 to 65 536
        bytes behind a dictionary of at least 2 bytes, of which at most 65 536 are in use, run side by side, one chain each on a
        private H9 hash table of 32 MiB over which it replays the dictionary's image (the same bytes).  Without it quality 9 runs
        item by item; longer items and the empty item still do.  It changes nothing at the other qualities and may be combined
        with quick_items.  A chain lasts its item's time however many run beside it: see include/brotli_mi355x.h for when it pays.

        zopfli_items=True: BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS -- at qualities 10 AND 11 (through the stream
        API, which defines these items, both are Zopfli) and lgwin 10 to 24 the items of 1 to 65 536 bytes behind a dictionary of
        at least 2 bytes, of which at most 65 536 are in use, run side by side: one wavefront each on H10 trees of its own, over
        which it copies the ONE image of the dictionary's trees that the call builds, and then walks the item the reference's way
        (the same bytes).  Without it these qualities run item by item; longer items and the empty item still do.  It changes
        nothing at qualities 0 to 9 and may be combined with the other two.  A walk is one wavefront and lasts tens of
        microseconds per byte: it pays with hundreds of items in a call, see include/brotli_mi355x.h.

        Items the reference itself fails on: behind a dictionary a match cut to one byte at the dictionary's end is a copy the
        reference cannot encode, and its stream call fails.  Such an item fails alone in the C call, which then returns 0 -- and
        this method raises BrotliCompressorException although every other stream was produced.  It is not rare at quality 2 on
        text behind a dictionary of the same kind: about 3 in 1000 items of 4 KiB in the measured runs, so
        a call of thousands of such items is expected to raise.  The exception carries .failed (their indices) and .streams (the
        streams of the others, None for a failed item): catch it, and send the failed items through another quality or without
        the dictionary."""
        routes = self.BATCH_ROUTE_QUICK_ITEMS if quick_items else 0
        routes |= self.BATCH_ROUTE_Q9_DICTIONARY_ITEMS if q9_items else 0
        routes |= self.BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS if zopfli_items else 0
        dictionary = bytes(dictionary)

        def call(count, inputs, in_sizes, outputs, out_sizes, results):
            return "BrotliMi355xCompressBatchWithDictionaryEx", self.lib.BrotliMi355xCompressBatchWithDictionaryEx(
                quality, lgwin, mode, routes, len(dictionary), dictionary, count, inputs, in_sizes, outputs, out_sizes, results)

        return self._batch(items, 1024, call)

    def compress_batch_with_dictionaries(self, items, dictionaries, item_dictionaries=None, quality=5, lgwin=22, mode=0, quick_items=False,
                                         zopfli_items=False, q9_items=False):
        """BrotliMi355xCompressBatchWithDictionaries: item i is the stream of an Encoder(params, dictionaries[k]) with
        k = item_dictionaries[i] that gets the item in one finish(); a decoder needs that dictionary.  item_dictionaries=None:
        item i takes dictionaries[i], and there must be as many dictionaries as items.  Several items may name one index.
        Returns a list of bytes.

        Side by side at qualities 5 to 8, lgwin 17 to 24, items of 1 to 65 536 bytes behind dictionaries of 2 to 65 536 bytes: one
        chain per item that files the item's dictionary into a table of its own and then parses the item (the same bytes).
        Everything else runs item by item in the same call.  When every item names the same index the call is
        compress_batch_with_dictionary(items, that dictionary).  It pays with hundreds of small items whose dictionaries differ
        (delta compression against previous versions, records of several kinds: 4096 items of 4 KiB behind 16 KiB each at quality 5
        in 26 ms against 5.6 s for the loop of stream calls, 64 of them in 4.7 ms against 88 ms); items that share one dictionary
        are up to 1.2 x faster through compress_batch_with_dictionary, whose chains replay one image of the dictionary.

        quick_items=False: side by side at qualities 5 to 8 only.

        quick_items=True: BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS -- at qualities 2 to 4 and lgwin 10 to 24 the items of
        at most one input block (16 384 bytes at quality 2 and 3, 65 536 at quality 4) behind a dictionary of at least 2 bytes, of
        which at most 65 536 are in use, run side by side too: one chain each on a private hash table that the chain zeroes and
        into which it files its item's dictionary itself (the same bytes).  Without it these qualities run item by item; longer
        items, the empty item and dictionaries of 0 or 1 bytes still do.  It changes nothing at the other qualities.  When every
        item names the same index the call is compress_batch_with_dictionary(items, that dictionary, quick_items=True).

        zopfli_items=True: BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS -- at qualities 10 AND 11 (through the stream API,
        which defines these items, both are Zopfli) and lgwin 10 to 24 the items of 1 to 65 536 bytes behind a dictionary of at
        least 2 bytes, of which at most 65 536 are in use, run side by side: one wavefront each that empties H10 trees of its
        own, files its item's dictionary into them wave-wide and walks the item the reference's way (the same bytes).  Without it
        these qualities run item by item.  There is no tree image per dictionary; when every item names the same index the call
        is compress_batch_with_dictionary(items, that dictionary, zopfli_items=True), whose chains replay one image of it.  It
        changes nothing at qualities 0 to 9 and may be combined with quick_items.  A walk is one
        wavefront and lasts tens of microseconds per byte: it pays with hundreds of items in a call, see include/brotli_mi355x.h.

        q9_items=True: BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS -- at quality 9 and lgwin 17 to 24 the items of 1 to 65 536
        bytes behind a dictionary of at least 2 bytes, of which at most 65 536 are in use, run side by side: one chain each on a
        private H9 hash table of 32 MiB that the chain empties and into which it files its item's dictionary itself (the same
        bytes).  Without it quality 9 runs item by item.  It changes nothing at the other qualities and may be combined with the
        other two flags.  When every item names the same index the call is compress_batch_with_dictionary(items, that
        dictionary, q9_items=True).  The strongest greedy level for (old version, new file) pairs where Zopfli is too slow.

        zopfli_items=True: BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS -- at qualities 10 AND 11 (through the stream
        API, which defines these items, both are Zopfli) and lgwin 10 to 24 the items of 1 to 65 536 bytes behind a dictionary of
        at least 2 bytes, of which at most 65 536 are in use, run side by side: one wavefront each on H10 trees of its own, over
        which it copies the ONE image of the dictionary's trees that the call builds, and then walks the item the reference's way
        (the same bytes).  Without it these qualities run item by item; longer items and the empty item still do.  It changes
        nothing at qualities 0 to 9 and may be combined with the other two.  A walk is one wavefront and lasts tens of
        microseconds per byte: it pays with hundreds of items in a call, see include/brotli_mi355x.h.

        Items the reference itself fails on: behind a dictionary a match cut to one byte at the dictionary's end is a copy the
        reference cannot encode, and its stream call fails.  Such an item fails alone in the C call, which then returns 0 -- and
        this method raises BrotliCompressorException although every other stream was produced.  It is not rare at quality 2 on
        text behind a dictionary of the same kind: about 3 in 1000 items of 4 KiB in the measured runs, so
        a call of thousands of such items is expected to raise.  The exception carries .failed (their indices) and .streams (the
        streams of the others, None for a failed item): catch it, and send the failed items through another quality or without
        the dictionary.

        Raises BrotliCompressorException like compress_batch_with_dictionary (.failed, .streams), also for an index out of range
        and for a dictionary count that does not match -- both fail the whole call."""
        routes = self.BATCH_ROUTE_QUICK_DICTIONARY_ITEMS if quick_items else 0
        routes |= self.BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS if zopfli_items else 0
        routes |= self.BATCH_ROUTE_Q9_DICTIONARY_ITEMS if q9_items else 0
        items = list(items)
        dictionaries = [bytes(d) for d in dictionaries]
        num = len(dictionaries)
        dicts = (c_char_p * max(1, num))(*dictionaries)
        dict_sizes = (c_size_t * max(1, num))(*[len(d) for d in dictionaries])
        if item_dictionaries is None:
            item_dicts = ctypes.cast(None, POINTER(c_size_t))
        else:
            item_dictionaries = [int(k) for k in item_dictionaries]
            if len(item_dictionaries) != len(items):
                raise ValueError("item_dictionaries names %d items, there are %d" % (len(item_dictionaries), len(items)))
            if any(k < 0 for k in item_dictionaries):
                raise ValueError("a dictionary index is negative")
            item_dicts = (c_size_t * max(1, len(item_dictionaries)))(*item_dictionaries)

        def call(count, inputs, in_sizes, outputs, out_sizes, results):
            return "BrotliMi355xCompressBatchWithDictionaries", self.lib.BrotliMi355xCompressBatchWithDictionaries(
                quality, lgwin, mode, routes, num, dicts, dict_sizes, count, item_dicts, inputs, in_sizes, outputs, out_sizes, results)

        return self._batch(items, 1024, call)

    def compress_batch_device(self, inputs, outputs, quality=5, lgwin=22, mode=0, long_items=False, quick_items=False, quick_long_items=False,
                              zopfli_items=False, q9_items=False):
        """BrotliMi355xCompressBatchDevice: compress_batch for items that lie in device memory, their streams left in device
        memory.  inputs: a sequence of (address, size), outputs: a sequence of (address, capacity), all plain integers (e.g.
        t.data_ptr() + offset); the addresses may have any alignment and may point into one tensor each, outputs must not
        overlap each other or any input.  Item i becomes the bytes compress(item, quality, lgwin, mode) gives, at outputs[i];
        the flags are those of compress_batch, and last_batch_info() tells how the items were taken.  On the side-by-side
        routes nothing crosses the bus; qualities 0 and 1 are staged through the host once per call (no gain over
        compress_batch), and no dictionary is taken (behind dictionaries:
        compress_batch_with_dictionaries_device).  Whatever produced the inputs must be complete before the call
        (torch.cuda.synchronize()); the call returns when every stream has landed.  Returns the list of stream sizes.

        An item whose capacity is too small fails alone in the C call, which then returns 0: this method raises
        BrotliCompressorException with .failed (the indices) and .sizes (the sizes of the others, 0 for a failed item; all 0
        after a call that failed as a whole)."""
        routes = (self.BATCH_ROUTE_LONG_ITEMS if long_items else 0) | (self.BATCH_ROUTE_QUICK_ITEMS if quick_items else 0)
        routes |= self.BATCH_ROUTE_QUICK_LONG_ITEMS if quick_long_items else 0
        routes |= self.BATCH_ROUTE_ZOPFLI_ITEMS if zopfli_items else 0
        routes |= self.BATCH_ROUTE_Q9_ITEMS if q9_items else 0
        inputs, outputs = list(inputs), list(outputs)
        count = len(inputs)
        if len(outputs) != count:
            raise ValueError("%d inputs, %d outputs" % (count, len(outputs)))
        if count == 0:
            return []
        in_ptrs = (c_void_p * count)(*[int(a) for a, _ in inputs])
        in_sizes = (c_size_t * count)(*[int(n) for _, n in inputs])
        out_ptrs = (c_void_p * count)(*[int(a) for a, _ in outputs])
        out_sizes = (c_size_t * count)(*[int(n) for _, n in outputs])
        results = (c_int32 * count)()
        ok = self.lib.BrotliMi355xCompressBatchDevice(quality, lgwin, mode, routes, count, in_ptrs, in_sizes, out_ptrs, out_sizes, results)
        sizes = [int(out_sizes[i]) if ok or results[i] else 0 for i in range(count)]
        if not ok:
            failed = [i for i in range(count) if not results[i]]
            e = BrotliCompressorException("BrotliMi355xCompressBatchDevice failed (items %s): %s" % (failed[:8], self.last_error()))
            e.failed, e.sizes = failed, sizes
            raise e
        return sizes

    def compress_batch_with_dictionaries_device(self, inputs, outputs, dictionaries, item_dictionaries=None, quality=5, lgwin=22, mode=0,
                                                quick_items=False, zopfli_items=False, q9_items=False):
        """BrotliMi355xCompressBatchWithDictionariesDevice: compress_batch_with_dictionaries for items and dictionaries that lie
        in device memory (the new and the previous version of many resources, say), their streams left in device memory.
        inputs and dictionaries: sequences of (address, size), outputs: a sequence of (address, capacity), all plain integers as
        for compress_batch_device; any alignment.  Inputs and dictionaries may overlap each other (item i - 1 may be item i's
        dictionary); outputs must not overlap each other, any input or any dictionary.  item_dictionaries, quick_items, zopfli_items and q9_items are
        those of compress_batch_with_dictionaries; item i becomes the bytes that method gives, at outputs[i], under the stream
        API's rules: there is no fallback to a stored stream, an item whose stream does not fit its capacity fails alone.  On the
        side-by-side routes nothing crosses the bus; every other item (see compress_batch_with_dictionaries) is staged through
        the host with the dictionary it names -- the same bytes, no gain.  Whatever produced the inputs must be complete before
        the call (torch.cuda.synchronize()); the call returns when every stream has landed.  Returns the list of stream sizes.

        Raises BrotliCompressorException like compress_batch_device, with .failed (the indices) and .sizes (the sizes of the
        others, 0 for a failed item; all 0 after a call that failed as a whole: an index out of range, a dictionary count that
        does not match).  As with compress_batch_with_dictionaries, a call of thousands of text items at quality 2 is expected
        to hold a few the reference itself fails on."""
        routes = self.BATCH_ROUTE_QUICK_DICTIONARY_ITEMS if quick_items else 0
        routes |= self.BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS if zopfli_items else 0
        routes |= self.BATCH_ROUTE_Q9_DICTIONARY_ITEMS if q9_items else 0
        inputs, outputs, dictionaries = list(inputs), list(outputs), list(dictionaries)
        count, num = len(inputs), len(dictionaries)
        if len(outputs) != count:
            raise ValueError("%d inputs, %d outputs" % (count, len(outputs)))
        if item_dictionaries is None:
            item_dicts = ctypes.cast(None, POINTER(c_size_t))
        else:
            item_dictionaries = [int(k) for k in item_dictionaries]
            if len(item_dictionaries) != count:
                raise ValueError("item_dictionaries names %d items, there are %d" % (len(item_dictionaries), count))
            if any(k < 0 for k in item_dictionaries):
                raise ValueError("a dictionary index is negative")
            item_dicts = (c_size_t * max(1, count))(*item_dictionaries)
        if count == 0:
            return []
        dict_ptrs = (c_void_p * max(1, num))(*[int(a) for a, _ in dictionaries])
        dict_sizes = (c_size_t * max(1, num))(*[int(n) for _, n in dictionaries])
        in_ptrs = (c_void_p * count)(*[int(a) for a, _ in inputs])
        in_sizes = (c_size_t * count)(*[int(n) for _, n in inputs])
        out_ptrs = (c_void_p * count)(*[int(a) for a, _ in outputs])
        out_sizes = (c_size_t * count)(*[int(n) for _, n in outputs])
        results = (c_int32 * count)()
        ok = self.lib.BrotliMi355xCompressBatchWithDictionariesDevice(quality, lgwin, mode, routes, num, dict_ptrs, dict_sizes, count, item_dicts, in_ptrs,
                                                                      in_sizes, out_ptrs, out_sizes, results)
        sizes = [int(out_sizes[i]) if ok or results[i] else 0 for i in range(count)]
        if not ok:
            failed = [i for i in range(count) if not results[i]]
            e = BrotliCompressorException("BrotliMi355xCompressBatchWithDictionariesDevice failed (items %s): %s" % (failed[:8], self.last_error()))
            e.failed, e.sizes = failed, sizes
            raise e
        return sizes

    def compress_batch_with_dictionary_device(self, inputs, outputs, dictionary, quality=5, lgwin=22, mode=0, quick_items=False, zopfli_items=False,
                                              q9_items=False):
        """compress_batch_with_dictionaries_device with ONE dictionary, (address, size) in device memory, named by every item: the
        call takes the shared-image path -- the streams of compress_batch_with_dictionary(items, dictionary, ..., quick_items),
        the dictionary reaching its image by one copy on the device (zopfli_items=True at qualities 10 and 11: one image of the
        dictionary's H10 trees, built once per call and copied by every chain over its own table; q9_items=True at quality 9: the
        image replayed over H9 tables).  Returns the list of stream sizes."""
        inputs = list(inputs)
        return self.compress_batch_with_dictionaries_device(inputs, outputs, [dictionary], [0] * len(inputs), quality, lgwin, mode, quick_items, zopfli_items, q9_items)

    def last_batch_info(self):
        """BrotliMi355xLastBatchInfo: the last compress_batch / compress_batch_with_dictionary / compress_batch_with_dictionaries call of this thread as a list of 8 integers -- [0] items, [1] items
        encoded side by side on the device, [2] items run one by one, [3] items answered without an encoder, [4] device groups, [5] dictionary bytes in use (0 without one; with a dictionary per item their sum over the indices named),
        [6] items that began side by side and were redone one by one (counted in [2]), [7] of the items in [1], those longer than one
        input block ([6] and [7]: long_items=True and quick_long_items=True only; the items quick_items=True, zopfli_items=True and
        q9_items=True take side by side count in [1] and [4], and so do those of compress_batch_with_dictionaries(...,
        quick_items=True), (..., zopfli_items=True) and (..., q9_items=True))."""
        info = (c_uint64 * 8)()
        self.lib.BrotliMi355xLastBatchInfo.restype = None
        self.lib.BrotliMi355xLastBatchInfo.argtypes = [POINTER(c_uint64)]
        self.lib.BrotliMi355xLastBatchInfo(info)
        return list(info)

    def last_batch_image_info(self):
        """BrotliMi355xLastBatchImageInfo: the dictionary images of the last batch call of this thread as a list of 4 integers --
        [0] images built, summed over the call's groups (a shared-dictionary call: 1 when it built its image), [1] side-by-side items
        whose chain replayed an image, [2] side-by-side items whose chain filed its own dictionary, [3] 0.  All zeros after a call
        without a dictionary and after one that failed as a whole."""
        info = (c_uint64 * 4)()
        self.lib.BrotliMi355xLastBatchImageInfo.restype = None
        self.lib.BrotliMi355xLastBatchImageInfo.argtypes = [POINTER(c_uint64)]
        self.lib.BrotliMi355xLastBatchImageInfo(info)
        return list(info)

    def compress_device(self, device_ptr, nbytes, quality=5, lgwin=22, mode=0, out_buffer=None):
        """One-shot compression of `nbytes` at device address `device_ptr` (e.g. tensor.data_ptr()).
        Returns (bytes, stats list of 32 doubles)."""
        cap = self.lib.BrotliEncoderMaxCompressedSize(nbytes) + 16
        out = out_buffer if out_buffer is not None else ctypes.create_string_buffer(cap)
        n = c_size_t(cap)
        stats = (c_double * 32)()
        if not self.lib.BrotliMi355xCompressDevice(quality, lgwin, mode, nbytes, c_void_p(device_ptr), byref(n), out, stats):
            raise BrotliCompressorException("BrotliMi355xCompressDevice failed: " + self.last_error())
        return ctypes.string_at(out, n.value), list(stats)

    # ---- multi-GPU helpers: one chunk per process, stitched on rank 0 ----
    def compress_chunk(self, data_or_ptr, nbytes, thread_index, num_threads, compression_options_map={}, on_device=False):
        n, keys, vals = self._options(compression_options_map)
        chunk_bytes = ((thread_index + 1) * nbytes) // num_threads - (thread_index * nbytes) // num_threads
        cap = self.lib.BrotliEncoderMaxCompressedSize(chunk_bytes) + 16
        out = ctypes.create_string_buffer(cap)
        size = c_size_t(cap)
        if on_device:
            src = c_void_p(data_or_ptr)
            keep = None
        else:
            keep = ctypes.create_string_buffer(bytes(data_or_ptr), max(1, nbytes))
            src = ctypes.cast(keep, c_void_p)
        ret = self.lib.BrotliMi355xCompressChunk(n, keys, vals, nbytes, src, 1 if on_device else 0, thread_index, num_threads,
                                                 byref(size), out)
        if ret == 0:
            raise BrotliCompressorException("BrotliMi355xCompressChunk failed: " + self.last_error())
        return ctypes.string_at(out, size.value)

    def concat_chunks(self, chunks):
        arr = (c_char_p * len(chunks))(*[bytes(c) for c in chunks])
        sizes = (c_size_t * len(chunks))(*[len(c) for c in chunks])
        cap = sum(len(c) for c in chunks) + 64
        out = ctypes.create_string_buffer(cap)
        n = c_size_t(cap)
        if not self.lib.BrotliMi355xConcatChunks(len(chunks), arr, sizes, byref(n), out):
            raise BrotliCompressorException("BrotliMi355xConcatChunks failed: " + self.last_error())
        return ctypes.string_at(out, n.value)

    def concat_chunk_views(self, views):
        """like concat_chunks, but on (address, size) pairs of host memory and without copying the result: returns a
        memoryview of a buffer owned by the Library (valid until the next call)"""
        n_chunks = len(views)
        arr = (c_void_p * n_chunks)(*[c_void_p(a) for a, _ in views])
        sizes = (c_size_t * n_chunks)(*[s for _, s in views])
        cap = sum(s for _, s in views) + 64
        if getattr(self, "_concat_buf", None) is None or len(self._concat_buf) < cap:
            self._concat_buf = ctypes.create_string_buffer(cap)
        n = c_size_t(len(self._concat_buf))
        if not self.lib.BrotliMi355xConcatChunks(n_chunks, ctypes.cast(arr, ctypes.POINTER(c_char_p)), sizes, byref(n), self._concat_buf):
            raise BrotliCompressorException("BrotliMi355xConcatChunks failed: " + self.last_error())
        return memoryview(self._concat_buf)[:n.value]

    def concat_chunk_ends(self, heads, tails, sizes, out_address, out_capacity):
        """BrotliMi355xConcatChunkEnds: heads / tails are (n, 8) uint8 host tensors (or anything with data_ptr()) holding the
        first / last bytes of every chunk; junction bytes go to out_address.  Returns (total size, [(dst, src, count)])"""
        n_chunks = len(sizes)
        csizes = (c_size_t * n_chunks)(*sizes)
        bodies = (c_size_t * (3 * n_chunks))()
        n = c_size_t(out_capacity)
        if not self.lib.BrotliMi355xConcatChunkEnds(n_chunks, c_void_p(heads.data_ptr()), c_void_p(tails.data_ptr()), csizes, byref(n),
                                                    c_void_p(out_address), bodies):
            raise BrotliCompressorException("BrotliMi355xConcatChunkEnds failed: " + self.last_error())
        return n.value, [(bodies[3 * i], bodies[3 * i + 1], bodies[3 * i + 2]) for i in range(n_chunks)]

    def encoder(self, **params):
        return Encoder(self, **params)


class Encoder(object):
    """Streaming encoder over BrotliEncoderCompressStream (what CompressorWriter does in the reference,
    src/enc/writer.rs:183-313): write() hands input over, finish() returns the stream."""

    def __init__(self, library, params=(), dictionary=None):
        self._l = library
        self._s = library.lib.BrotliEncoderCreateInstance(None, None, None)
        if not self._s:
            raise BrotliCompressorException("BrotliEncoderCreateInstance failed")
        items = params.items() if hasattr(params, "items") else params
        for k, v in items:
            if not library.lib.BrotliEncoderSetParameter(self._s, int(k), int(v)):
                raise BrotliCompressorException("invalid parameter %r=%r" % (k, v))
        if dictionary is not None:
            library.lib.BrotliEncoderSetCustomDictionary(self._s, len(dictionary), bytes(dictionary))
        self._out = bytearray()

    def _stream(self, op, data):
        buf = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
        avail_in = c_size_t(len(data))
        next_in = c_void_p(ctypes.addressof(buf))
        chunk = ctypes.create_string_buffer(1 << 16)
        while True:
            avail_out = c_size_t(len(chunk))
            next_out = c_void_p(ctypes.addressof(chunk))
            total = c_size_t(0)
            ok = self._l.lib.BrotliEncoderCompressStream(self._s, op, byref(avail_in), byref(next_in), byref(avail_out),
                                                         byref(next_out), byref(total))
            if not ok:
                raise BrotliCompressorException("BrotliEncoderCompressStream failed: " + self._l.last_error())
            self._out += chunk.raw[:len(chunk) - avail_out.value]
            if avail_in.value == 0 and not self._l.lib.BrotliEncoderHasMoreOutput(self._s):
                break

    def write(self, data):
        self._stream(BROTLI_OPERATION_PROCESS, data)

    def flush(self, data=b""):
        """BROTLI_OPERATION_FLUSH (CompressorWriter::flush, src/enc/writer.rs): everything written so far becomes
        decodable; returns the bytes produced since the last flush / start"""
        self._stream(BROTLI_OPERATION_FLUSH, data)
        piece = bytes(self._out)
        self._flushed = getattr(self, "_flushed", b"") + piece
        self._out = bytearray()
        return piece

    def emit_metadata(self, payload):
        """BROTLI_OPERATION_EMIT_METADATA: pending input is flushed, then `payload` (at most 16 MiB) goes out as a
        metadata block, which decoders skip; returns the bytes produced"""
        self._stream(BROTLI_OPERATION_EMIT_METADATA, payload)
        piece = bytes(self._out)
        self._out = bytearray()
        return piece

    def set_parameter(self, key, value):
        return bool(self._l.lib.BrotliEncoderSetParameter(self._s, int(key), int(value)))

    def finish(self, data=b""):
        """BROTLI_OPERATION_FINISH, with the last of the input if any"""
        self._stream(BROTLI_OPERATION_FINISH, data)
        assert self._l.lib.BrotliEncoderIsFinished(self._s)
        return bytes(self._out)  # (after flush() calls: the remainder of the stream)

    def close(self):
        if self._s:
            self._l.lib.BrotliEncoderDestroyInstance(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None


def default_library():
    global _default
    if _default is None:
        _default = Library()
    return _default


def BrotliEncoderVersion():
    return default_library().BrotliEncoderVersion()


def BrotliEncoderMaxCompressedSizeMulti(input_size, num_threads):
    return default_library().BrotliEncoderMaxCompressedSizeMulti(input_size, num_threads)


def BrotliCompress(any_input, compression_options_map={}, num_threads=4):
    return default_library().BrotliCompress(any_input, compression_options_map, num_threads)


def BrotliEncoderCreateWorkPool(num_workers):
    return default_library().BrotliEncoderCreateWorkPool(num_workers)


def BrotliEncoderDestroyWorkPool(pool):
    return default_library().BrotliEncoderDestroyWorkPool(pool)


def BrotliEncoderCompressWorkPool(work_pool, any_input, compression_options_map={}, num_threads=4):
    return default_library().BrotliEncoderCompressWorkPool(work_pool, any_input, compression_options_map, num_threads)


# fail loudly at import time when the product library is absent
if not os.path.exists(LIB_PATH):
    raise ImportError("libbrotli_mi355x.so is missing; build it with `make -C rust-brotli_amd` "
                      "(or __graft_entry__.build()). There is no CPU fallback.")
