#!/usr/bin/env python3
"""tools/batch_probe.py -- what BrotliMi355xCompressBatch buys for many small payloads (--qualities, default 0 and 1; lgwin 22).

For every class of items (seeded markov text and synth.mixed):
  batch     the batch call on all items (host clock around the synchronous call, warm-up, median and spread of the repeats)
  loop      the same items as a loop of BrotliEncoderCompress from 1 and from 4 threads, on the library given with --parent-lib (a
            build of the parent commit) -- on the first --loop-items items of the class, scaled to the class by item count
  cpu       the oracle (oracle/liborc_fast.so) on one core of the same host, on the same first items, scaled likewise
            (the items of a class are independent draws, so the first ones are a fair sample of it)
and the A/B of the two homes of a small fragment's hash table: the classes whose tables fit workgroup memory -- 512 B items (2^9
words) and 2 KiB items (2^11 words) -- and the log-uniform mix, with BROTLI_MI355X_BATCH_LDS_BITS=0 and =11, alternating.

With --qualities 5,8 (the items of one input block side by side, batch_greedy.h) the baseline of the parent commit is the same
BrotliMi355xCompressBatch call on its library -- there a loop over the one-shot path -- on the first --loop-items items, scaled by
item count, and the loop from 4 threads; --rounds 3 alternates this build and the parent (one child each) and records whether every
run of this build beats every run of the parent.  The table-home A/B belongs to qualities 0 and 1 and is skipped otherwise.

With --dictionary BYTES (and --qualities 5,8) the call measured is BrotliMi355xCompressBatchWithDictionary: the dictionary is drawn from
the same generator and seed family as the items; the baseline of the parent commit is a loop of stream-API calls with
BrotliEncoderSetCustomDictionary on its library, from 1 and from 4 threads, alternating with this build --rounds times; the CPU
baseline is the oracle's dictionary stream; and this build's plain batch call on the same items gives the cost (in time) and the
gain (in bytes) of the dictionary.

With --long-items (and --qualities 5,8) this build is called through BrotliMi355xCompressBatchEx with
BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS: the items of two to four input blocks go side by side as well, one chain each.  The parent's
library is still measured through its plain batch call and its 4-thread loop.  The classes 1024x128KiB and 256x256KiB (--only) are
all long items.

With --quick-items (and --qualities 2,3,4) this build is called through BrotliMi355xCompressBatchEx with
BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: the items of at most one input block (16 KiB at quality 2 and 3, 64 KiB at quality 4) go side by
side, one chain on a private BasicHasher table each.  The parent's library is measured through its plain batch call (a loop over the
one-shot path) and its 4-thread loop.  The classes are 4096x4KiB, 4096x16KiB (at quality 2 and 3 every item exactly at the limit),
1024x64KiB (side by side at quality 4 only), 4096x512B and the log-uniform mix.

With --quick-long-items this build is called with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS | BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS: at
qualities 2 to 4 the items of two to four input blocks go side by side as well, one chain each that walks from block to block.  The
parent's library is measured through BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS on the same items, which takes them one by one.  The
classes are 1024x32KiB and 1024x64KiB at quality 2 and 3, 1024x128KiB and 256x256KiB at quality 4, and the count sweep
{16, 64, 256, 1024}x48KiB at quality 2 (QUICK_LONG_QUALITIES); --skip cpu,loop leaves out the oracle and the 4-thread loop.

With --dictionary BYTES --quick-items (and --qualities 2,3,4) this build is called through BrotliMi355xCompressBatchWithDictionaryEx with
BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: behind the shared dictionary the items of at most one input block go side by side, one chain each on
a table that starts as the dictionary's.  The parent's library is measured through BrotliMi355xCompressBatchWithDictionary on the first
--loop-items items, scaled by item count -- there every item runs one by one through the stream path -- alternating with this build --rounds
times; the CPU baseline is the oracle's dictionary stream.  The items the call fails alone (reference_fails_on_items) are checked
against the oracle one by one: it must fail on each of them.  The classes are 4096x4KiB and 4096x512B, 1024x16KiB (qualities 2 and 3: one
input block) and 64x4KiB, the few-items case.

With --zopfli-items (and --qualities 11) this build is called through BrotliMi355xCompressBatchEx with
BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS: the items of at most 65 536 bytes go side by side, one wavefront each that walks its item the
reference's way on H10 trees of its own.  The parent's library is measured through its plain batch call, which takes these items one by
one (on the first --loop-items items, scaled by item count).  The classes are 1024x4KiB, 256x16KiB, 64x64KiB and 16x4KiB, the few-items
case.  (--qualities 10,11 is accepted: BrotliEncoderCompress runs quality 10 at quality 9, and it goes one by one in both builds.)

With --q9-items (and --qualities 9,10) this build is called through BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS:
the items of at most one input block (256 KiB at lgwin 22) go side by side, one chain each on a private H9 table of 32 MiB, 255 of
them in flight.  The parent's library is measured through its plain batch call, which takes these items one by one (on the first
--loop-items items, scaled by item count), and through its 4-thread loop; the CPU baseline is the oracle on one core.  The classes
are 4096x4KiB, 1024x16KiB, 256x64KiB and 64x256KiB, the few-items cases 16x4KiB and 64x4KiB, and the log-uniform mix.

With --same-call (and any of the above) the parent's library is measured through the very call this build is measured through, route bits
and dictionary included, alternating with it --rounds times: the A/B of a change that keeps the routes.  Per class the result holds the
medians of both, their difference, and the parent's own spread between its rounds as the margin; nothing else is measured.  With
--dictionary N the classes are those --only names; with --dicts the call is BrotliMi355xCompressBatchWithDictionaries on the
DICTS_CLASSES, every item behind its own dictionary.

With --dicts (and --qualities 5,8, or 2,3,4) the call measured is BrotliMi355xCompressBatchWithDictionaries, a custom dictionary per item: text items,
and per item a dictionary that is another draw from the items' own source (DICTS_CLASSES: 4096 items of 4 KiB behind 4 and 16 KiB, 1024 of
16 KiB behind 16 and 64 KiB, 64 of 4 KiB behind 16 KiB).  It is measured against the only way the parent commit has -- the loop of stream
calls with BrotliEncoderSetCustomDictionary, each item with its own dictionary, on the calling thread and from four threads (--parent-lib, or
this build's library: the loop is the same code), on the first --loop-items items, scaled by item count -- against the oracle's dictionary
stream on one core, and against the shared-dictionary call on the same items: for that ONE dictionary is given as `count` distinct
indices (the chains file it themselves) and to BrotliMi355xCompressBatchWithDictionary (the chains replay its image), which prices
self-filing against the image.  At qualities 2 to 4 this build is called with BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, and the shared call
is BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS; two more classes are measured there (4096 items of
512 bytes behind 16 KiB; at quality 4, where that is one input block, 1024 items of 64 KiB behind 64 KiB).
With --dicts --qualities 10,11 this build is called with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS (1024) on the classes of
DICTS_ZOPFLI_HEADLINE (1024 items of 4 KiB behind 16 KiB, 256 of 16 KiB and of 4 KiB behind 64 KiB, 64 and 16 of 4 KiB behind 16 KiB), in --rounds
alternating rounds of one run each: the route; the route with BROTLI_MI355X_ZOPFLI_PREPEND_LANE0=1 on the classes of DICTS_ZOPFLI_AB (the
dictionary filed by lane 0 alone inside the same kernel); the --parent-lib build through the same call without the bit, where every item runs
one by one (first --loop-items items, scaled by item count); the loop of stream calls from four threads (the same); then the oracle on one core.
With --dicts --qualities 9 this build is called with BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096) on the classes of DICTS_Q9_HEADLINE
(4096 items of 4 KiB behind 16 KiB, 1024 of 16 KiB and 256 of 64 KiB behind 64 KiB, 64 and 16 of 4 KiB behind 16 KiB, and the calls of few items
of DICTS_Q9_FEW: 4 and 1 of 4 KiB behind 16 KiB, 16 of 64 KiB behind 64 KiB), in --rounds alternating
rounds of one run each: the route; on the classes of DICTS_Q9_SHARED the shared form (BrotliMi355xCompressBatchWithDictionaryEx with 4096, every
item behind the first dictionary) with the image and with BROTLI_MI355X_BATCH_DICT_SELF_FILE=1; the --parent-lib build through the per-item call
without the bit (first --loop-items items, scaled); the loop of stream calls from four threads (the same); then the oracle on one core.

With --shared-zopfli (qualities 10 and 11) the call measured is BrotliMi355xCompressBatchWithDictionaryEx with
BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (8192) on the classes of SHARED_ZOPFLI_HEADLINE, every item behind the class's first
dictionary, in --rounds alternating rounds of one run each: the tree image (the default); BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 (every chain files
the dictionary itself); the --parent-lib build through BrotliMi355xCompressBatchWithDictionaries with 1024 and one index named by every item (the
self-filing baseline); this build's shared entry without the bit, one by one, on the first --loop-items items, scaled.  On SHARED_ZOPFLI_LONE (one
item of 4 KiB behind 16 and 64 KiB) the first two and BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 with BROTLI_MI355X_ZOPFLI_PREPEND_LANE0=1: a lone
chain's filing, wave-wide and on lane 0, as a difference of whole calls.  Beside them the build and the filing by themselves, through the debug
entry brotli_mi355x_debug_zopfli_prepend: modes 0 (lane 0), 1 (wave-wide, one wavefront) and 2 (the image build) at 16 and 64 KiB, less the same
entry at 2 bytes (allocation, the fill and the copies, which every mode pays).

With --dicts --kinds the call measured is BrotliMi355xCompressBatchWithDictionaries with K distinct dictionaries, the items dealt to them round
robin -- a few dictionaries that each serve many items, where this build makes an image per dictionary that enough items of a group name: this
build against --parent-lib through the same call (there every chain files its dictionary), against the shared call on the same items behind ONE
dictionary, and against this build with BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS=0, --rounds alternating rounds, one process per measurement.
--kinds all runs KINDS_SHAPES and the sweep of that variable (KINDS_SWEEP), --kinds sweep the sweep alone, --kinds 4,16 with --only and
--qualities those shapes.

With --device (and --parent-lib) the call measured is BrotliMi355xCompressBatchDevice on torch tensors -- one uint8 tensor of items in,
one of streams out -- beside the parent's BrotliMi355xCompressBatchEx on the same items from host memory and beside the "honest
alternative" a caller with device-resident payloads has without the call: the items down (one D2H), the parent's host call, the
streams up (one H2D of the output buffer's used part).  The three alternate inside one child per shape, --runs times each behind
--warmup rounds of all three; the shapes are DEVICE_SHAPES (text).  Per shape: min .. max of each, and whether the device call's
minimum stays at or below the host call's maximum (the bound: the two differ only by work that was removed).

With --device-dicts (and --parent-lib) the call measured is BrotliMi355xCompressBatchWithDictionariesDevice -- dictionaries and items in one
uint8 tensor, streams into another -- beside the only way the parent commit has for the same job: dictionaries and items down to
page-locked memory (one D2H), its BrotliMi355xCompressBatchWithDictionaries, the streams up (one H2D); and beside that host call alone,
which tells what the staging around it costs.  The shapes are DEVICE_DICTS_SHAPES (text; one of them behind ONE shared dictionary: the
shared image); the three ways alternate inside one child per shape as for --device.  Per shape: min .. max of each, and whether the
device call's minimum stays at or below the alternative's maximum.

Every measurement runs in a child process of its own (the table's home is one setting per process, read once; the parent's library
is another shared object), one after the other, each under its own time limit; the first failure ends the probe.

  python tools/batch_probe.py --parent-lib <libbrotli_mi355x.so of the parent commit> --out profiles/r07_batch_q01.json
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
LGWIN = 22

CLASSES = {
    "4096x4KiB": ("uniform", 4096, 4 << 10),
    "4096x16KiB": ("uniform", 4096, 16 << 10),
    "1024x64KiB": ("uniform", 1024, 64 << 10),
    "64xalice29": ("alice", 64, 0),
    # items of several input blocks (--long-items)
    "1024x128KiB": ("uniform", 1024, 128 << 10),
    "256x256KiB": ("uniform", 256, 256 << 10),
    "4096xlog200B-256KiB": ("log", 4096, 0),
    # one table size each (the A/B of the table's home)
    "4096x512B": ("uniform", 4096, 512),
    "4096x2KiB": ("uniform", 4096, 2 << 10),
    # items of two to four input blocks at qualities 2 to 4 (--quick-long-items)
    "1024x32KiB": ("uniform", 1024, 32 << 10),
    "16x48KiB": ("uniform", 16, 48 << 10),
    "64x48KiB": ("uniform", 64, 48 << 10),
    "256x48KiB": ("uniform", 256, 48 << 10),
    "1024x48KiB": ("uniform", 1024, 48 << 10),
    # behind a shared dictionary at qualities 2 to 4 (--dictionary N --quick-items)
    "1024x16KiB": ("uniform", 1024, 16 << 10),
    "64x4KiB": ("uniform", 64, 4 << 10),
    # small static files at quality 11 (--zopfli-items)
    "1024x4KiB": ("uniform", 1024, 4 << 10),
    "256x16KiB": ("uniform", 256, 16 << 10),
    "64x64KiB": ("uniform", 64, 64 << 10),
    "16x4KiB": ("uniform", 16, 4 << 10),
    # qualities 9 and 10 (--q9-items)
    "256x64KiB": ("uniform", 256, 64 << 10),
    "64x256KiB": ("uniform", 64, 256 << 10),
}
HEADLINE = ["4096x4KiB", "4096x16KiB", "1024x64KiB", "64xalice29", "4096xlog200B-256KiB"]
AB = ["4096x512B", "4096x2KiB", "4096xlog200B-256KiB"]
# (--quick-long-items) the qualities at which a class is made of items of two to four input blocks
QUICK_LONG_QUALITIES = {"1024x32KiB": (2, 3), "1024x64KiB": (2, 3), "1024x128KiB": (4,), "256x256KiB": (4,),
                        "16x48KiB": (2,), "64x48KiB": (2,), "256x48KiB": (2,), "1024x48KiB": (2,)}
DICT_QUICK_HEADLINE = ["4096x4KiB", "4096x512B", "1024x16KiB", "64x4KiB"]  # (--dictionary N --quick-items)
DICT_QUICK_QUALITIES = {"1024x16KiB": (2, 3)}  # (one input block at quality 2 and 3)
QUICK_HEADLINE = ["4096x4KiB", "4096x16KiB", "1024x64KiB", "4096x512B", "4096xlog200B-256KiB"]  # (--quick-items)
ZOPFLI_HEADLINE = ["1024x4KiB", "256x16KiB", "64x64KiB", "16x4KiB"]  # (--zopfli-items)
# (--dicts) class -> (items, item bytes, dictionary bytes per item)
DICTS_CLASSES = {"4096x4KiB+4KiB": (4096, 4 << 10, 4 << 10), "4096x4KiB+16KiB": (4096, 4 << 10, 16 << 10), "1024x16KiB+16KiB": (1024, 16 << 10, 16 << 10),
                 "1024x16KiB+64KiB": (1024, 16 << 10, 64 << 10), "64x4KiB+16KiB": (64, 4 << 10, 16 << 10),
                 # qualities 2 to 4 only (BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS)
                 "1024x64KiB+64KiB": (1024, 64 << 10, 64 << 10), "4096x512B+16KiB": (4096, 512, 16 << 10)}
DICTS_QUALITIES = {"1024x64KiB+64KiB": (4,), "4096x512B+16KiB": (2, 3, 4)}  # (64 KiB is one input block at quality 4 only)
# (--dicts --qualities 10,11) BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS: the classes, and the two of the prepend A/B
DICTS_CLASSES.update({"1024x4KiB+16KiB": (1024, 4 << 10, 16 << 10), "256x16KiB+64KiB": (256, 16 << 10, 64 << 10), "256x4KiB+64KiB": (256, 4 << 10, 64 << 10),
                      "16x4KiB+16KiB": (16, 4 << 10, 16 << 10)})
DICTS_ZOPFLI_HEADLINE = ["1024x4KiB+16KiB", "256x16KiB+64KiB", "256x4KiB+64KiB", "64x4KiB+16KiB", "16x4KiB+16KiB"]
DICTS_ZOPFLI_AB = ["1024x4KiB+16KiB", "256x4KiB+64KiB"]
# (--dicts --qualities 9) BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS: the classes, and the one of the shared form (image against self-filing)
DICTS_Q9_FEW = {"4x4KiB+16KiB": (4, 4 << 10, 16 << 10), "1x4KiB+16KiB": (1, 4 << 10, 16 << 10), "16x64KiB+64KiB": (16, 64 << 10, 64 << 10)}  # (where a call is expected to lose)
DICTS_CLASSES.update({"256x64KiB+64KiB": (256, 64 << 10, 64 << 10)})
DICTS_CLASSES.update(DICTS_Q9_FEW)
DICTS_Q9_HEADLINE = ["4096x4KiB+16KiB", "1024x16KiB+64KiB", "256x64KiB+64KiB", "64x4KiB+16KiB", "16x4KiB+16KiB"] + list(DICTS_Q9_FEW)
DICTS_Q9_SHARED = ["4096x4KiB+16KiB"]
# (--shared-zopfli) BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS: every item behind the class's first dictionary
DICTS_CLASSES.update({"1x4KiB+64KiB": (1, 4 << 10, 64 << 10)})
SHARED_ZOPFLI_HEADLINE = ["1024x4KiB+16KiB", "256x16KiB+64KiB", "256x4KiB+64KiB", "16x4KiB+16KiB"]
SHARED_ZOPFLI_LONE = ["1x4KiB+16KiB", "1x4KiB+64KiB"]
Q9_HEADLINE = ["4096x4KiB", "1024x16KiB", "256x64KiB", "64x256KiB", "16x4KiB", "64x4KiB", "4096xlog200B-256KiB"]  # (--q9-items)


def items_of(name, data):
    import synth
    kind, count, size = CLASSES[name]
    if kind == "alice":
        return [synth.alice()] * count
    rng = random.Random(17)
    pool = synth.markov_text(8 << 20, 5) if data == "text" else synth.mixed(8 << 20, 5)
    out = []
    for _ in range(count):
        n = size if kind == "uniform" else int(200 * ((256 << 10) / 200) ** rng.random())
        off = rng.randrange(0, len(pool) - n)
        out.append(pool[off:off + n])
    return out


def dictionary_of(data, nbytes):
    """the items' generator and seed family, another draw"""
    import synth
    pool = synth.markov_text(8 << 20, 5) if data == "text" else synth.mixed(8 << 20, 5)
    off = random.Random(18).randrange(0, len(pool) - nbytes)
    return pool[off:off + nbytes]


def dicts_of(name):
    """(items, a dictionary per item): text, the dictionaries further draws from the items' source"""
    import synth
    count, size, dict_bytes = DICTS_CLASSES[name]
    pool = synth.markov_text(8 << 20, 5)
    rng = random.Random(19)
    items, dictionaries = [], []
    for _ in range(count):
        off = rng.randrange(0, len(pool) - size)
        items.append(pool[off:off + size])
        off = rng.randrange(0, len(pool) - dict_bytes)
        dictionaries.append(pool[off:off + dict_bytes])
    return items, dictionaries


def stats(times):
    times = sorted(times)
    return {"median_ms": round(1e3 * statistics.median(times), 3), "min_ms": round(1e3 * times[0], 3), "max_ms": round(1e3 * times[-1], 3),
            "spread_pct": round(100.0 * (times[-1] - times[0]) / statistics.median(times), 2), "runs": len(times)}


def bind(path):
    L = ctypes.CDLL(path)
    L.BrotliEncoderMaxCompressedSize.restype = ctypes.c_size_t
    L.BrotliEncoderMaxCompressedSize.argtypes = [ctypes.c_size_t]
    L.BrotliEncoderCompress.restype = ctypes.c_int
    L.BrotliEncoderCompress.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
                                        ctypes.c_char_p]
    return L


def measure_batch(lib_path, items, quality, runs, warmup, dictionary=None, routes=0):
    L = bind(lib_path)
    L.BrotliMi355xCompressBatch.restype = ctypes.c_int32
    if routes:
        L.BrotliMi355xCompressBatchEx.restype = ctypes.c_int32
    if dictionary is not None:
        L.BrotliMi355xCompressBatchWithDictionary.restype = ctypes.c_int32
        if routes:
            L.BrotliMi355xCompressBatchWithDictionaryEx.restype = ctypes.c_int32
    info = (ctypes.c_uint64 * 8)()
    n = len(items)
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + (16 if dictionary is None else 1024) for x in items]
    bufs = [ctypes.create_string_buffer(c) for c in caps]
    inputs = (ctypes.c_char_p * n)(*items)
    in_sizes = (ctypes.c_size_t * n)(*[len(x) for x in items])
    outputs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (ctypes.c_size_t * n)()
    results = (ctypes.c_int32 * n)()
    L.BrotliMi355xLastError.restype = ctypes.c_char_p
    times = []
    failed = []
    for it in range(warmup + runs):
        for i in range(n):
            out_sizes[i] = caps[i]
        t = time.perf_counter()
        if routes and dictionary is not None:
            ok = L.BrotliMi355xCompressBatchWithDictionaryEx(quality, LGWIN, 0, ctypes.c_uint32(routes), ctypes.c_size_t(len(dictionary)), ctypes.c_char_p(dictionary),
                                                             ctypes.c_size_t(n), inputs, in_sizes, outputs, out_sizes, results)
        elif routes:
            ok = L.BrotliMi355xCompressBatchEx(quality, LGWIN, 0, ctypes.c_uint32(routes), ctypes.c_size_t(n), inputs, in_sizes, outputs, out_sizes, None)
        elif dictionary is None:
            ok = L.BrotliMi355xCompressBatch(quality, LGWIN, 0, ctypes.c_size_t(n), inputs, in_sizes, outputs, out_sizes, None)
        else:
            ok = L.BrotliMi355xCompressBatchWithDictionary(quality, LGWIN, 0, ctypes.c_size_t(len(dictionary)), ctypes.c_char_p(dictionary), ctypes.c_size_t(n),
                                                           inputs, in_sizes, outputs, out_sizes, results)
        dt = time.perf_counter() - t
        if dictionary is not None and ok != 1:
            # items on which the reference itself fails (a copy of one byte at the dictionary end) fail alone: counted, not fatal
            failed = [i for i in range(n) if not results[i]]
            assert 0 < len(failed) <= n // 256 + 1 and b"reference encoder fails" in L.BrotliMi355xLastError(), (failed, L.BrotliMi355xLastError())
            ok = 1
        assert ok == 1
        if it >= warmup:
            times.append(dt)
    if hasattr(L, "BrotliMi355xLastBatchInfo"):  # (the parent's library has none)
        L.BrotliMi355xLastBatchInfo(info)
    return times, sum(out_sizes), list(info), failed


def measure_dicts(lib_path, items, dictionaries, quality, runs, warmup, shared=False, routes=None, one_index=False, kinds=0):
    """BrotliMi355xCompressBatchWithDictionaries with dictionaries[i] for item i; shared: BrotliMi355xCompressBatchWithDictionary with
    dictionaries[0].  At qualities 2 to 4 both with the route that takes such items side by side (512, and 4 through the Ex entry).
    routes: the bits of the per-item call (default: 512 at qualities 2 to 4, else 0; 1024 and 4096 are the caller's to give); with
    shared they go to BrotliMi355xCompressBatchWithDictionaryEx as they are (4096: quality 9).  one_index: the per-item call with dictionaries[0]
    alone and item_dicts = {0, 0, ...}.  kinds = K: the per-item call with dictionaries[:K] and item_dicts = {0, 1, .. K - 1, 0, 1, ..}, the items
    dealt to K distinct dictionaries round robin; the returned info then carries BrotliMi355xLastBatchImageInfo behind its 8 values
    (zeros on a library without it)."""
    L = bind(lib_path)
    quick = 2 <= quality <= 4
    L.BrotliMi355xCompressBatchWithDictionaryEx.restype = ctypes.c_int32
    L.BrotliMi355xCompressBatchWithDictionaries.restype = ctypes.c_int32
    L.BrotliMi355xCompressBatchWithDictionary.restype = ctypes.c_int32
    L.BrotliMi355xLastError.restype = ctypes.c_char_p
    n = len(items)
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]
    bufs = [ctypes.create_string_buffer(c) for c in caps]
    inputs = (ctypes.c_char_p * n)(*items)
    in_sizes = (ctypes.c_size_t * n)(*[len(x) for x in items])
    outputs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (ctypes.c_size_t * n)()
    results = (ctypes.c_int32 * n)()
    dicts = (ctypes.c_char_p * n)(*dictionaries)
    dict_sizes = (ctypes.c_size_t * n)(*[len(d) for d in dictionaries])
    info = (ctypes.c_uint64 * 8)()
    named = (ctypes.c_size_t * n)() if one_index else None
    if kinds:
        named = (ctypes.c_size_t * n)(*[i % kinds for i in range(n)])
    times, failed = [], []
    for it in range(warmup + runs):
        for i in range(n):
            out_sizes[i] = caps[i]
        t = time.perf_counter()
        if shared and (quick or routes):
            ok = L.BrotliMi355xCompressBatchWithDictionaryEx(quality, LGWIN, 0, ctypes.c_uint32(routes if routes else 4), ctypes.c_size_t(len(dictionaries[0])), ctypes.c_char_p(dictionaries[0]),
                                                             ctypes.c_size_t(n), inputs, in_sizes, outputs, out_sizes, results)
        elif shared:
            ok = L.BrotliMi355xCompressBatchWithDictionary(quality, LGWIN, 0, ctypes.c_size_t(len(dictionaries[0])), ctypes.c_char_p(dictionaries[0]), ctypes.c_size_t(n),
                                                           inputs, in_sizes, outputs, out_sizes, results)
        else:
            ok = L.BrotliMi355xCompressBatchWithDictionaries(quality, LGWIN, 0, ctypes.c_uint32((512 if quick else 0) if routes is None else routes), ctypes.c_size_t(1 if one_index else kinds if kinds else n), dicts, dict_sizes,
                                                             ctypes.c_size_t(n), named, inputs, in_sizes, outputs, out_sizes, results)
        dt = time.perf_counter() - t
        if ok != 1:
            # items on which the reference itself fails (a copy of one byte at the dictionary end) fail alone: counted, not fatal
            failed = [i for i in range(n) if not results[i]]
            assert 0 < len(failed) <= n // 64 + 1 and b"reference encoder fails" in L.BrotliMi355xLastError(), (failed, L.BrotliMi355xLastError())
        if it >= warmup:
            times.append(dt)
    L.BrotliMi355xLastBatchInfo(info)
    if kinds:
        images = (ctypes.c_uint64 * 4)()
        if hasattr(L, "BrotliMi355xLastBatchImageInfo"):  # (the parent's library has none)
            L.BrotliMi355xLastBatchImageInfo(images)
        return times, sum(out_sizes), list(info) + list(images), failed
    return times, sum(out_sizes), list(info), failed


def measure_loop(lib_path, items, quality, threads, runs, warmup, dictionary=None, dictionaries=None):
    L = bind(lib_path)
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + (16 if dictionary is None else 1024) for x in items]
    bufs = [ctypes.create_string_buffer(c) for c in caps]
    L.BrotliEncoderCreateInstance.restype = ctypes.c_void_p
    L.BrotliEncoderCreateInstance.argtypes = [ctypes.c_void_p] * 3
    L.BrotliEncoderDestroyInstance.argtypes = [ctypes.c_void_p]
    L.BrotliEncoderSetParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
    L.BrotliEncoderSetCustomDictionary.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    L.BrotliEncoderCompressStream.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.BrotliEncoderIsFinished.argtypes = [ctypes.c_void_p]
    L.BrotliMi355xLastError.restype = ctypes.c_char_p
    failed = set()  # items on which the reference fails: the batch call's item_results name the same ones

    def one_stream(i):
        # what the batch call with a dictionary is defined as, per item
        s = L.BrotliEncoderCreateInstance(None, None, None)
        for k, v in ((0, 0), (1, quality), (2, LGWIN)):
            L.BrotliEncoderSetParameter(s, k, v)
        own = dictionaries[i] if dictionaries is not None else dictionary
        L.BrotliEncoderSetCustomDictionary(s, len(own), own)
        avail_in, avail_out = ctypes.c_size_t(len(items[i])), ctypes.c_size_t(caps[i])
        next_in = ctypes.c_void_p(ctypes.cast(ctypes.c_char_p(items[i]), ctypes.c_void_p).value)
        next_out = ctypes.c_void_p(ctypes.addressof(bufs[i]))
        ok = L.BrotliEncoderCompressStream(s, 2, ctypes.byref(avail_in), ctypes.byref(next_in), ctypes.byref(avail_out), ctypes.byref(next_out), None)
        done = L.BrotliEncoderIsFinished(s)
        L.BrotliEncoderDestroyInstance(s)
        if not ok:  # (the message is looked at only for a call that failed: it stays set afterwards)
            assert b"reference encoder fails" in L.BrotliMi355xLastError(), (i, L.BrotliMi355xLastError())
            failed.add(i)
        else:
            assert done, i

    def work(lo, hi):
        size = ctypes.c_size_t()
        for i in range(lo, hi):
            if dictionary is not None or dictionaries is not None:
                one_stream(i)
                continue
            size.value = caps[i]
            assert L.BrotliEncoderCompress(quality, LGWIN, 0, len(items[i]), items[i], ctypes.byref(size), bufs[i])

    times = []
    n = len(items)
    for it in range(warmup + runs):
        pool = [threading.Thread(target=work, args=(n * k // threads, n * (k + 1) // threads)) for k in range(threads)]
        t = time.perf_counter()
        for th in pool:
            th.start()
        for th in pool:
            th.join()
        dt = time.perf_counter() - t
        if it >= warmup:
            times.append(dt)
    return times, sorted(failed)


def measure_cpu(items, quality, runs, dictionary=None, dictionaries=None):
    os.environ["ORC_FAST"] = "1"
    import orc
    times = []
    total = 0
    for it in range(1 + runs):
        total = 0
        t = time.perf_counter()
        for i, x in enumerate(items):
            if dictionary is None and dictionaries is None:
                total += len(orc.compress(x, quality, LGWIN))
                continue
            try:
                total += sum(map(len, orc.stream_with_flushes(x, [(0, 0), (1, quality), (2, LGWIN)], [],
                                                              dictionary=dictionaries[i] if dictionaries is not None else dictionary)))
            except orc.ReferencePanics:
                pass  # (the reference fails on this item: the library fails it alone)
        dt = time.perf_counter() - t
        if it >= 1:
            times.append(dt)
    return times, total


def child_prepend(args):
    """--shared-zopfli: the debug entry by itself -- per dictionary size, --runs rounds of modes 0, 1 and 2 one after the other (host clock around the
    synchronous entry: allocation, upload, launches, download of 512 KiB of buckets and the forest)"""
    import synth
    L = ctypes.CDLL(args.lib)
    pool = synth.markov_text(1 << 20, 5)
    out = []
    for D in (2, 16 << 10, 64 << 10):
        text = pool[:D + 64]
        buckets = (ctypes.c_uint32 * (1 << 17))()
        forest = (ctypes.c_uint32 * (2 * ((D + 63) & ~63)))()
        times = {0: [], 1: [], 2: []}
        for it in range(args.warmup + args.runs):
            for mode in (0, 1, 2):
                t = time.perf_counter()
                ret = L.brotli_mi355x_debug_zopfli_prepend(text, ctypes.c_uint32(len(text)), ctypes.c_uint32(D), ctypes.c_uint32(LGWIN), ctypes.c_uint32(mode), buckets, forest)
                dt = time.perf_counter() - t
                assert ret == 0, (D, mode, ret)
                if it >= args.warmup:
                    times[mode].append(dt)
        row = {"dictionary_bytes": D}
        for mode, name in ((0, "lane0"), (1, "wave_wide"), (2, "image_build")):
            row[name + "_min_max_ms"] = [round(1e3 * min(times[mode]), 3), round(1e3 * max(times[mode]), 3)]
        out.append(row)
        print(json.dumps(row), flush=True)
    with open(args.child_out, "w") as f:
        json.dump(out, f)


def child_dicts(args):
    """--dicts: the children of main_dicts -- batch (own dictionaries), same (one dictionary as count indices), shared, loop, cpu"""
    out = []
    for name in args.classes.split(","):
        items, dictionaries = dicts_of(name)
        n = args.loop_items
        for quality in [int(q) for q in args.qualities.split(",")]:
            if quality not in DICTS_QUALITIES.get(name, (quality,)):
                continue
            row = {"class": name, "data": "text", "quality": quality, "items": len(items), "bytes": sum(map(len, items)), "dictionary_bytes": len(dictionaries[0])}
            if args.child in ("batch", "same", "shared", "one_index"):
                ds = dictionaries if args.child == "batch" else [dictionaries[0]] * len(items)
                times, csize, info, failed = measure_dicts(args.lib, items, ds, quality, args.runs, args.warmup, shared=args.child == "shared",
                                                           routes=args.routes if args.child != "same" and args.routes else None, one_index=args.child == "one_index")
                row.update(stats(times), compressed_bytes=csize, batch_info=info, reference_fails_on_items=failed)
            elif args.child == "shared_first":  # the shared entry without a bit on the first --loop-items items: one by one
                times, csize, info, failed = measure_dicts(args.lib, items[:n], [dictionaries[0]] * min(n, len(items)), quality, args.runs, args.warmup, shared=True)
                row.update(stats(times), measured_items=min(n, len(items)), compressed_bytes=csize, batch_info=info, reference_fails_on_items=failed)
            elif args.child == "batch_first":  # the same call on the first --loop-items items (a library whose items run one by one)
                times, csize, info, failed = measure_dicts(args.lib, items[:n], dictionaries[:n], quality, args.runs, args.warmup, routes=args.routes)
                row.update(stats(times), measured_items=min(n, len(items)), compressed_bytes=csize, batch_info=info, reference_fails_on_items=failed)
            elif args.child == "loop":
                times, failed = measure_loop(args.lib, items[:n], quality, args.threads, args.runs, 1, dictionaries=dictionaries[:n])
                row.update(stats(times), threads=args.threads, measured_items=min(n, len(items)), reference_fails_on_items=failed)
            else:
                times, csize = measure_cpu(items[:n], quality, args.runs, dictionaries=dictionaries[:n])
                row.update(stats(times), measured_items=min(n, len(items)), compressed_bytes=csize)
            out.append(row)
            print(json.dumps(row), flush=True)
    with open(args.child_out, "w") as f:
        json.dump(out, f)


# (--dicts --kinds) the per-item call with K distinct dictionaries, the items dealt to them round robin: (class, qualities, the K)
KINDS_ALL = (4, 16, 64, 256, 4096)
KINDS_SHAPES = [("4096x4KiB+16KiB", (5, 8, 2, 4, 9), KINDS_ALL), ("4096x512B+16KiB", (2,), (16,)), ("1024x16KiB+64KiB", (5,), (16,)), ("64x4KiB+16KiB", (5,), (4,))]
KINDS_SWEEP = (2, 4, 8, 16)  # BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS, on 4096x4KiB+16KiB with K = 4096 / that value


def kinds_routes(quality):
    return 512 if 2 <= quality <= 4 else 4096 if quality == 9 else 0


def child_kinds(args):
    """one measurement: `--classes` one class, `--qualities` one quality, --kinds K (0: the shared call behind the first dictionary)"""
    name, quality = args.classes, int(args.qualities)
    items, dictionaries = dicts_of(name)
    if int(args.kinds):
        times, csize, info, failed = measure_dicts(args.lib, items, dictionaries, quality, args.runs, args.warmup, routes=kinds_routes(quality), kinds=int(args.kinds))
    else:
        shared_routes = 4 if 2 <= quality <= 4 else 4096 if quality == 9 else None
        times, csize, info, failed = measure_dicts(args.lib, items, [dictionaries[0]] * len(items), quality, args.runs, args.warmup, shared=True, routes=shared_routes)
    row = {"class": name, "quality": quality, "kinds": int(args.kinds), "compressed_bytes": csize, "batch_info": info[:8], "image_info": info[8:], "reference_fails_on_items": len(failed)}
    row.update(stats(times))
    with open(args.child_out, "w") as f:
        json.dump(row, f)


def main_kinds(args, doc, save):
    """--dicts --kinds: a mixed group.  Every shape this build against the parent's library through the same call, --rounds alternating rounds, one
    process per measurement; the shared call on the same items behind ONE dictionary (the floor); this build with images off
    (BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS=0); and the sweep of that variable behind the default.  --kinds all: KINDS_SHAPES; --kinds sweep: the
    sweep alone; --kinds K[,K..] with --only and --qualities: those."""
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaries with K distinct dictionaries, the items dealt to them round robin: this build (an image per dictionary that "
                   "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS items of a group name) vs the parent commit's library through the same call (every chain files its dictionary), vs "
                   "the shared call on the same items behind one dictionary; lgwin 22")
    doc["method"] = "host clock around the synchronous call, %d warm-up runs and %d runs per process, one process per measurement, %d alternating rounds; min .. max over all runs of a setting" % (
        args.warmup, args.runs, args.rounds)
    doc["rows"], doc["sweep"] = [], []
    tmp = args.out + ".child.json"
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None

    def one(lib, name, quality, kinds, env=None):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "kinds", "--classes", name, "--qualities", str(quality), "--kinds", str(kinds),
               "--lib", lib, "--runs", str(args.runs), "--warmup", str(args.warmup), "--child-out", tmp]
        e = dict(os.environ)
        e.pop("BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS", None)
        e.update(env or {})
        r = subprocess.run(cmd, env=e)
        if r.returncode != 0:  # (a fault or a time limit: nothing more is started)
            raise SystemExit("the measurement %r ended with %d" % (cmd, r.returncode))
        with open(tmp) as f:
            return json.load(f)

    def settle(rows):
        return {"min_ms": min(r["min_ms"] for r in rows), "max_ms": max(r["max_ms"] for r in rows), "median_ms": round(statistics.median(r["median_ms"] for r in rows), 3),
                "image_info": rows[-1]["image_info"], "batch_info": rows[-1]["batch_info"], "compressed_bytes": rows[-1]["compressed_bytes"]}

    if args.kinds == "sweep":
        shapes = []
    elif args.kinds == "all":
        shapes = KINDS_SHAPES
    else:
        shapes = [(c, tuple(int(q) for q in args.qualities.split(",")), tuple(int(k) for k in args.kinds.split(","))) for c in args.only.split(",")]
    for name, qualities, all_kinds in shapes:
        for quality in qualities:
            floor = settle([one(args.lib, name, quality, 0) for _ in range(args.rounds)])
            for kinds in all_kinds:
                this, base, off = [], [], []
                for _ in range(args.rounds):
                    this.append(one(args.lib, name, quality, kinds))
                    if parent:
                        base.append(one(parent, name, quality, kinds))
                    off.append(one(args.lib, name, quality, kinds, {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "0"}))
                row = {"class": name, "quality": quality, "kinds": kinds, "this": settle(this), "images_off": settle(off), "shared_one_dictionary": floor}
                if base:
                    row["parent"] = settle(base)
                    assert row["parent"]["compressed_bytes"] == row["this"]["compressed_bytes"], row
                doc["rows"].append(row)
                print(json.dumps(row), flush=True)
                save()
    if args.kinds in ("sweep", "all"):
        name = "4096x4KiB+16KiB"
        for quality in (5, 2, 9):
            for m in KINDS_SWEEP:
                on, off = [], []
                for _ in range(args.rounds):
                    on.append(one(args.lib, name, quality, 4096 // m, {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": str(m)}))
                    off.append(one(args.lib, name, quality, 4096 // m, {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "0"}))
                row = {"class": name, "quality": quality, "min_items": m, "kinds": 4096 // m, "images_on": settle(on), "images_off": settle(off)}
                doc["sweep"].append(row)
                print(json.dumps(row), flush=True)
                save()
    if os.path.exists(tmp):
        os.remove(tmp)


# (--device) class, quality, route bits
DEVICE_SHAPES = [("4096x4KiB", 5, 0), ("4096x4KiB", 2, 4), ("1024x16KiB", 5, 0), ("256x64KiB", 9, 128), ("64x4KiB", 5, 0)]


def child_device(args):
    """--device: one shape -- the device call of this build, the parent's host call, and D2H + that host call + H2D, alternating"""
    import torch
    name, quality, routes = args.classes, int(args.qualities), args.routes
    items = items_of(name, "text")
    n = len(items)
    L, P = bind(args.lib), bind(args.parent_lib or args.lib)
    L.BrotliMi355xCompressBatchDevice.restype = ctypes.c_int32
    P.BrotliMi355xCompressBatchEx.restype = ctypes.c_int32
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    in_at, out_at, a, b = [], [], 0, 0
    for x, c in zip(items, caps):
        in_at.append(a)
        out_at.append(b)
        a += len(x)
        b += c
    src = torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).cuda()
    dst = torch.zeros(b, dtype=torch.uint8, device="cuda")
    in_sizes = (ctypes.c_size_t * n)(*[len(x) for x in items])
    out_sizes = (ctypes.c_size_t * n)()
    d_in = (ctypes.c_void_p * n)(*[src.data_ptr() + o for o in in_at])
    d_out = (ctypes.c_void_p * n)(*[dst.data_ptr() + o for o in out_at])
    # the host call's buffers: page-locked, like those of a caller that stages for a device
    h_src = torch.empty(a, dtype=torch.uint8).pin_memory()
    h_dst = torch.empty(b, dtype=torch.uint8).pin_memory()
    h_src.copy_(src)
    h_in = (ctypes.c_void_p * n)(*[h_src.data_ptr() + o for o in in_at])
    h_out = (ctypes.c_void_p * n)(*[h_dst.data_ptr() + o for o in out_at])
    P.BrotliMi355xCompressBatchEx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]
    L.BrotliMi355xCompressBatchDevice.argtypes = P.BrotliMi355xCompressBatchEx.argtypes

    def reset():
        for i in range(n):
            out_sizes[i] = caps[i]

    def device_call():
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        ok = L.BrotliMi355xCompressBatchDevice(quality, LGWIN, 0, routes, n, d_in, in_sizes, d_out, out_sizes, None)
        dt = time.perf_counter() - t
        assert ok == 1
        return dt, list(out_sizes)

    def host_call():
        reset()
        t = time.perf_counter()
        ok = P.BrotliMi355xCompressBatchEx(quality, LGWIN, 0, routes, n, h_in, in_sizes, h_out, out_sizes, None)
        dt = time.perf_counter() - t
        assert ok == 1
        return dt, list(out_sizes)

    def alternative():
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        h_src.copy_(src)  # (synchronous: device to page-locked host memory)
        ok = P.BrotliMi355xCompressBatchEx(quality, LGWIN, 0, routes, n, h_in, in_sizes, h_out, out_sizes, None)
        used = out_at[-1] + out_sizes[n - 1]
        dst[:used].copy_(h_dst[:used])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert ok == 1
        return dt, list(out_sizes)

    times = {"device": [], "host": [], "alternative": []}
    sizes = None
    for it in range(args.warmup + args.runs):
        for what, call in (("device", device_call), ("host", host_call), ("alternative", alternative)):
            dt, got = call()
            assert sizes is None or got == sizes, (what, it)  # (the same streams from every way)
            sizes = got
            if it >= args.warmup:
                times[what].append(dt)
    # the streams themselves: the device call's against the host call's
    device_call()
    image = dst.cpu().numpy().tobytes()
    host_call()
    host_image = h_dst.numpy().tobytes()
    assert all(image[o:o + k] == host_image[o:o + k] for o, k in zip(out_at, sizes))
    info = (ctypes.c_uint64 * 8)()
    device_call()
    L.BrotliMi355xLastBatchInfo(info)
    row = {"class": name, "data": "text", "quality": quality, "routes": routes, "items": n, "bytes": a, "compressed_bytes": sum(sizes), "batch_info": list(info)}
    for what in times:
        row[what] = stats(times[what])
    row["device_min_within_host_max"] = bool(row["device"]["min_ms"] <= row["host"]["max_ms"])
    print(json.dumps(row), flush=True)
    with open(args.child_out, "w") as f:
        json.dump([row], f)


def main_device(args, doc, save):
    doc["what"] = ("BrotliMi355xCompressBatchDevice (torch tensors in, tensors out) vs the parent commit's BrotliMi355xCompressBatchEx on the same items from "
                   "page-locked host memory vs D2H of the items + that host call + H2D of the streams; text, lgwin 22; alternating inside one process per shape")
    doc["method"] = "host clock around each synchronous way, %d warm-up rounds of all three, then %d rounds; min .. max of the repeats" % (args.warmup, args.runs)
    doc["shapes"] = []
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".batch_probe_child.json")
    for name, quality, routes in DEVICE_SHAPES:
        if args.only and name + "/q%d" % quality not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "device", "--classes", name, "--qualities", str(quality), "--routes", str(routes),
               "--lib", args.lib, "--runs", str(args.runs), "--warmup", str(args.warmup), "--child-out", tmp] + (["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else [])
        r = subprocess.run(cmd)
        if r.returncode != 0:
            raise SystemExit("batch_probe: the device shape %s at quality %d ended with status %d: nothing more is started" % (name, quality, r.returncode))
        doc["shapes"] += json.load(open(tmp))
        os.remove(tmp)
        save()
    doc["device_min_within_host_max_on_every_shape"] = all(r["device_min_within_host_max"] for r in doc["shapes"])
    save()
    print(json.dumps(doc, indent=1))


# (--device-dicts) DICTS_CLASSES class, quality, route bits of the device call, one shared dictionary instead of one per item
DEVICE_DICTS_SHAPES = [("4096x4KiB+16KiB", 5, 0, False), ("4096x4KiB+16KiB", 2, 512, False), ("1024x16KiB+64KiB", 5, 0, False),
                       ("4096x4KiB+16KiB", 5, 0, True), ("64x4KiB+16KiB", 5, 0, False)]


def child_device_dicts(args):
    """--device-dicts: one shape -- BrotliMi355xCompressBatchWithDictionariesDevice of this build on tensors, beside the only way the
    parent commit has for dictionaries and items in device memory: both down to page-locked memory, its host dictionary call, the
    streams up; and that host call alone (what the staging around it costs).  The three alternate."""
    import torch
    name, quality, routes, shared = args.classes, int(args.qualities), args.routes, bool(args.shared)
    items, dictionaries = dicts_of(name)
    n = len(items)
    if shared:
        dictionaries = dictionaries[:1]
    nd = len(dictionaries)
    named = [0] * n if shared else list(range(n))
    L, P = bind(args.lib), bind(args.parent_lib or args.lib)
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]
    dict_at, in_at, out_at, a, b = [], [], [], 0, 0
    for d in dictionaries:
        dict_at.append(a)
        a += len(d)
    for x, c in zip(items, caps):
        in_at.append(a)
        out_at.append(b)
        a += len(x)
        b += c
    src = torch.frombuffer(bytearray(b"".join(dictionaries) + b"".join(items)), dtype=torch.uint8).cuda()
    dst = torch.zeros(b, dtype=torch.uint8, device="cuda")
    h_src = torch.empty(a, dtype=torch.uint8).pin_memory()
    h_dst = torch.empty(b, dtype=torch.uint8).pin_memory()
    h_src.copy_(src)
    dict_sizes = (ctypes.c_size_t * nd)(*[len(d) for d in dictionaries])
    item_dicts = (ctypes.c_size_t * n)(*named)
    in_sizes = (ctypes.c_size_t * n)(*[len(x) for x in items])
    out_sizes = (ctypes.c_size_t * n)()
    results = (ctypes.c_int32 * n)()
    d_dicts = (ctypes.c_void_p * nd)(*[src.data_ptr() + o for o in dict_at])
    d_in = (ctypes.c_void_p * n)(*[src.data_ptr() + o for o in in_at])
    d_out = (ctypes.c_void_p * n)(*[dst.data_ptr() + o for o in out_at])
    h_dicts = (ctypes.c_void_p * nd)(*[h_src.data_ptr() + o for o in dict_at])
    h_in = (ctypes.c_void_p * n)(*[h_src.data_ptr() + o for o in in_at])
    h_out = (ctypes.c_void_p * n)(*[h_dst.data_ptr() + o for o in out_at])
    for lib, entry in ((L, "BrotliMi355xCompressBatchWithDictionariesDevice"), (P, "BrotliMi355xCompressBatchWithDictionaries")):
        f = getattr(lib, entry)
        f.restype = ctypes.c_int32
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def reset():
        for i in range(n):
            out_sizes[i] = caps[i]

    def answer():
        # (at quality 2 the reference fails on a few text items in a thousand: they fail alone, the same ones every way)
        return [out_sizes[i] if results[i] else 0 for i in range(n)]

    def device_call():
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        L.BrotliMi355xCompressBatchWithDictionariesDevice(quality, LGWIN, 0, routes, nd, d_dicts, dict_sizes, n, item_dicts, d_in, in_sizes, d_out, out_sizes, results)
        dt = time.perf_counter() - t
        return dt, answer()

    def host_call():
        reset()
        t = time.perf_counter()
        P.BrotliMi355xCompressBatchWithDictionaries(quality, LGWIN, 0, routes, nd, h_dicts, dict_sizes, n, item_dicts, h_in, in_sizes, h_out, out_sizes, results)
        dt = time.perf_counter() - t
        return dt, answer()

    def alternative():
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        h_src.copy_(src)  # (synchronous: dictionaries and items, device to page-locked host memory)
        P.BrotliMi355xCompressBatchWithDictionaries(quality, LGWIN, 0, routes, nd, h_dicts, dict_sizes, n, item_dicts, h_in, in_sizes, h_out, out_sizes, results)
        used = out_at[-1] + out_sizes[n - 1]
        dst[:used].copy_(h_dst[:used])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        return dt, answer()

    times = {"device": [], "host": [], "alternative": []}
    sizes = None
    for it in range(args.warmup + args.runs):
        for what, call in (("device", device_call), ("alternative", alternative), ("host", host_call)):
            dt, got = call()
            assert sizes is None or got == sizes, (what, it)  # (the same answers from every way)
            sizes = got
            if it >= args.warmup:
                times[what].append(dt)
    assert sum(1 for k in sizes if k == 0) <= n // 50, "more items fail than the reference fails on"
    # the streams themselves: the device call's against the parent's host call's
    dst.zero_()
    device_call()
    image = dst.cpu().numpy().tobytes()
    info = (ctypes.c_uint64 * 8)()
    L.BrotliMi355xLastBatchInfo(info)
    host_call()
    host_image = h_dst.numpy().tobytes()
    host_info = (ctypes.c_uint64 * 8)()
    P.BrotliMi355xLastBatchInfo(host_info)
    assert all(image[o:o + k] == host_image[o:o + k] for o, k in zip(out_at, sizes))
    assert list(info) == list(host_info), (list(info), list(host_info))
    row = {"class": name, "data": "text", "quality": quality, "routes": routes, "shared_dictionary": shared, "items": n, "item_bytes": a - in_at[0],
           "dictionary_bytes": in_at[0], "compressed_bytes": sum(sizes), "items_the_reference_fails_on": sum(1 for k in sizes if k == 0), "batch_info": list(info)}
    for what in times:
        row[what] = stats(times[what])
    row["device_min_within_alternative_max"] = bool(row["device"]["min_ms"] <= row["alternative"]["max_ms"])
    print(json.dumps(row), flush=True)
    with open(args.child_out, "w") as f:
        json.dump([row], f)


def main_device_dicts(args, doc, save):
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionariesDevice (dictionaries and items in one tensor, streams into another) vs the parent commit's only "
                   "way for the same job: dictionaries and items down to page-locked memory, its BrotliMi355xCompressBatchWithDictionaries, the streams up "
                   "('alternative'); 'host' is that host call alone from page-locked memory; text, lgwin 22; alternating inside one process per shape")
    doc["method"] = "host clock around each synchronous way, %d warm-up rounds of all three, then %d rounds; min .. max of the repeats" % (args.warmup, args.runs)
    doc["shapes"] = []
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".batch_probe_child.json")
    for name, quality, routes, shared in DEVICE_DICTS_SHAPES:
        tag = name + "/q%d" % quality + ("/shared" if shared else "")
        if args.only and tag not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "device-dicts", "--classes", name, "--qualities", str(quality),
               "--routes", str(routes), "--lib", args.lib, "--runs", str(args.runs), "--warmup", str(args.warmup), "--child-out", tmp]
        cmd += (["--shared"] if shared else []) + (["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else [])
        r = subprocess.run(cmd)
        if r.returncode != 0:
            raise SystemExit("batch_probe: the shape %s ended with status %d: nothing more is started" % (tag, r.returncode))
        doc["shapes"] += json.load(open(tmp))
        os.remove(tmp)
        save()
    doc["device_min_within_alternative_max_on_every_shape"] = all(r["device_min_within_alternative_max"] for r in doc["shapes"])
    save()
    print(json.dumps(doc, indent=1))


def child(args):
    if args.child == "device":
        return child_device(args)
    if args.child == "device-dicts":
        return child_device_dicts(args)
    if args.child == "kinds":
        return child_kinds(args)
    if args.child == "prepend":
        return child_prepend(args)
    if args.dicts:
        return child_dicts(args)
    out = []
    for name in args.classes.split(","):
        for data in (["text"] if CLASSES[name][0] == "alice" else ["text", "mixed"]):
            items = items_of(name, data)
            first = items[:args.loop_items]
            dictionary = dictionary_of(data, args.dictionary) if args.dictionary and not args.plain else None
            for quality in [int(q) for q in args.qualities.split(",")]:
                if args.quick_long_classes and quality not in QUICK_LONG_QUALITIES.get(name, ()):
                    continue
                if args.dictionary and quality not in DICT_QUICK_QUALITIES.get(name, (quality,)):
                    continue
                row = {"class": name, "data": data, "quality": quality, "items": len(items), "bytes": sum(map(len, items))}
                if args.child == "batch":
                    times, csize, info, failed = measure_batch(args.lib, first if args.first_only else items, quality, args.runs, args.warmup, dictionary,
                                                              (1 if args.long_items else 0) | (4 if args.quick_items else 0) | (16 if args.quick_long_items else 0) |
                                                              (32 if args.zopfli_items else 0) | (128 if args.q9_items else 0))
                    row.update(stats(times), compressed_bytes=csize, batch_info=info, reference_fails_on_items=failed, measured_items=len(first) if args.first_only else len(items))
                elif args.child == "loop":
                    times, failed = measure_loop(args.lib, first, quality, args.threads, args.runs, 1, dictionary)
                    row.update(stats(times), threads=args.threads, measured_items=len(first), reference_fails_on_items=failed)
                else:
                    times, csize = measure_cpu(first, quality, args.runs, dictionary)
                    row.update(stats(times), measured_items=len(first), compressed_bytes=csize)
                out.append(row)
                print(json.dumps(row), flush=True)
    with open(args.child_out, "w") as f:
        json.dump(out, f)


def run_child(args, what, classes, lib=None, lds=None, threads=1, limit=600, first_only=False, plain=False, long_items=False, quick_items=False,
              quick_long_items=False, zopfli_items=False, q9_items=False, routes=0, extra_env=None):
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_ZOPFLI_PREPEND_LANE0", None)
    env.pop("BROTLI_MI355X_BATCH_DICT_SELF_FILE", None)
    env.update(extra_env or {})
    env.pop("BROTLI_MI355X_BATCH_LDS_BITS", None)
    if lds is not None:
        env["BROTLI_MI355X_BATCH_LDS_BITS"] = str(lds)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".batch_probe_child.json")
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what, "--classes", ",".join(classes), "--lib", lib or args.lib,
           "--threads", str(threads), "--runs", str(args.runs), "--warmup", str(args.warmup), "--loop-items", str(args.loop_items), "--child-out", tmp, "--qualities", args.qualities,
           "--dictionary", str(args.dictionary)] + (["--first-only"] if first_only else []) + (["--plain"] if plain else []) + (["--long-items"] if long_items else []) + (["--quick-items"] if quick_items else [])
    cmd += (["--quick-long-items"] if quick_long_items else []) + (["--quick-long-classes"] if args.quick_long_items else [])
    cmd += ["--zopfli-items"] if zopfli_items else []
    cmd += ["--q9-items"] if q9_items else []
    cmd += ["--dicts"] if args.dicts else []
    cmd += ["--routes", str(routes)] if routes else []
    r = subprocess.run(cmd, env=env)
    if r.returncode != 0:
        raise SystemExit("batch_probe: %s (lds=%s, threads=%d) ended with status %d: nothing more is started" % (what, lds, threads, r.returncode))
    rows = json.load(open(tmp))
    os.remove(tmp)
    return rows


def key(row):
    return "%s/%s/q%d" % (row["class"], row["data"], row["quality"])


def main_dictionary(args, doc, save, classes):
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionary (%d bytes of dictionary) vs a loop of stream-API calls with BrotliEncoderSetCustomDictionary "
                   "(parent commit, 1 and 4 threads) vs the oracle's dictionary stream on one CPU core vs this build's plain batch call; lgwin 22" % args.dictionary)
    rows = {}
    for rnd in range(args.rounds):
        for row in run_child(args, "batch", classes, limit=900):
            this = {k: row[k] for k in ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")}
            if rnd == 0:
                rows[key(row)] = {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": args.dictionary, "compressed_bytes": row["compressed_bytes"],
                                  "batch_info": row["batch_info"], "reference_fails_on_items": row["reference_fails_on_items"], "batch": this}
            rows[key(row)].setdefault("batch_rounds", []).append(this)
        doc["classes"] = rows
        save()
        for row in run_child(args, "batch", classes, limit=900, plain=True):
            rows[key(row)]["compressed_bytes_plain"] = row["compressed_bytes"]
            rows[key(row)].setdefault("plain_batch_rounds", []).append({k: row[k] for k in ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")})
        save()
        for threads in (1, 4):
            if not args.parent_lib:
                continue
            for row in run_child(args, "loop", classes, lib=os.path.abspath(args.parent_lib), threads=threads, limit=900):
                scale = row["items"] / row["measured_items"]
                # (the loop runs the first items only: it must fail on exactly those of them the batch call failed on)
                assert row["reference_fails_on_items"] == [i for i in rows[key(row)]["reference_fails_on_items"] if i < row["measured_items"]], row
                rows[key(row)].setdefault("parent_loop_%dt_rounds" % threads, []).append(
                    {"median_ms_scaled": round(row["median_ms"] * scale, 3), "min_ms_scaled": round(row["min_ms"] * scale, 3), "max_ms_scaled": round(row["max_ms"] * scale, 3),
                     "spread_pct": row["spread_pct"], "measured_items": row["measured_items"]})
            save()
    for row in run_child(args, "cpu", classes, limit=900):
        scale = row["items"] / row["measured_items"]
        rows[key(row)]["cpu_one_core"] = {"median_ms_scaled": round(row["median_ms"] * scale, 3), "measured_items": row["measured_items"], "spread_pct": row["spread_pct"]}
    for k, v in rows.items():
        b = statistics.median(r["median_ms"] for r in v["batch_rounds"])
        v["batch_MBps"] = round(v["bytes"] / 1e3 / b, 1)
        v["cpu_over_batch"] = round(v["cpu_one_core"]["median_ms_scaled"] / b, 3)
        v["dictionary_over_plain_time"] = round(b / statistics.median(r["median_ms"] for r in v["plain_batch_rounds"]), 3)
        v["dictionary_over_plain_bytes"] = round(v["compressed_bytes"] / v["compressed_bytes_plain"], 4)
        loops = [v[n] for n in ("parent_loop_1t_rounds", "parent_loop_4t_rounds") if v.get(n)]
        if loops:
            better = min(loops, key=lambda rs: statistics.median(r["median_ms_scaled"] for r in rs))
            worst_batch = max(r["max_ms"] for r in v["batch_rounds"])
            best_batch = min(r["min_ms"] for r in v["batch_rounds"])
            v["better_loop_over_batch"] = {"median": round(statistics.median(r["median_ms_scaled"] for r in better) / b, 1),
                                           "min": round(min(r["min_ms_scaled"] for r in better) / worst_batch, 1),
                                           "max": round(max(r["max_ms_scaled"] for r in better) / best_batch, 1)}
            v["every_run_beats_every_parent_run"] = bool(worst_batch < min(r["min_ms_scaled"] for r in better))
        else:
            v["better_loop_over_batch"] = "not measured"
    save()
    print(json.dumps(doc, indent=1))


def verify_flagged_items(args, rows):
    """The items the batch call failed alone, against the oracle, on this host's CPU: the reference's dictionary stream must fail on
    every one of them, and on none of as many of its neighbours (the parent's loop and the CPU baseline run the first --loop-items
    items only, which need not hold any of them)."""
    os.environ["ORC_FAST"] = "1"
    import orc
    for k, v in rows.items():
        flagged = v["reference_fails_on_items"]
        v["reference_fails_on_items_verified"] = "none flagged"
        if not flagged:
            continue
        name, data, quality = k.split("/")
        items = items_of(name, data)
        dictionary = dictionary_of(data, args.dictionary)

        def fails(i):
            try:
                orc.stream_with_flushes(items[i], [(0, 0), (1, int(quality[1:])), (2, LGWIN)], [], dictionary=dictionary)
            except orc.ReferencePanics:
                return True
            return False

        neighbours = [i + 1 for i in flagged if i + 1 < len(items) and i + 1 not in flagged]
        assert all(fails(i) for i in flagged), (k, "the batch call failed an item the oracle encodes")
        assert not any(fails(i) for i in neighbours), (k, "the oracle fails on an item the batch call encoded")
        v["reference_fails_on_items_verified"] = "the oracle fails on all %d flagged items and on none of %d neighbours" % (len(flagged), len(neighbours))


def main_dictionary_quick(args, doc, save, classes):
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaryEx(BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS) behind %d bytes of dictionary vs the parent commit's "
                   "BrotliMi355xCompressBatchWithDictionary on the same items, there one by one through the stream path, vs the oracle's dictionary "
                   "stream on one CPU core; lgwin 22" % args.dictionary)
    rows = {}
    for rnd in range(args.rounds):
        for row in run_child(args, "batch", classes, limit=900, quick_items=True):
            this = {k: row[k] for k in ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")}
            if rnd == 0:
                rows[key(row)] = {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": args.dictionary, "compressed_bytes": row["compressed_bytes"],
                                  "batch_info": row["batch_info"], "reference_fails_on_items": row["reference_fails_on_items"], "batch": this}
            rows[key(row)].setdefault("batch_rounds", []).append(this)
            assert row["reference_fails_on_items"] == rows[key(row)]["reference_fails_on_items"], row  # (the same items in every round)
        doc["classes"] = rows
        save()
        if args.parent_lib:
            for row in run_child(args, "batch", classes, lib=os.path.abspath(args.parent_lib), limit=900, first_only=True):
                scale = row["items"] / row["measured_items"]
                rows[key(row)].setdefault("parent_batch_rounds", []).append({"median_ms_scaled": round(row["median_ms"] * scale, 3), "min_ms_scaled": round(row["min_ms"] * scale, 3),
                                                                           "max_ms_scaled": round(row["max_ms"] * scale, 3), "spread_pct": row["spread_pct"], "measured_items": row["measured_items"]})
            save()
    for row in ([] if "cpu" in args.skip.split(",") else run_child(args, "cpu", classes, limit=900)):
        scale = row["items"] / row["measured_items"]
        rows[key(row)]["cpu_one_core"] = {"median_ms_scaled": round(row["median_ms"] * scale, 3), "measured_items": row["measured_items"], "spread_pct": row["spread_pct"]}
    verify_flagged_items(args, rows)
    for k, v in rows.items():
        b = statistics.median(r["median_ms"] for r in v["batch_rounds"])
        # (compressed_bytes and MB/s cover the whole class: an item the reference fails on is parsed like any other and leaves no stream)
        v["batch_MBps"] = round(v["bytes"] / 1e3 / b, 1)
        v["cpu_over_batch"] = round(v["cpu_one_core"]["median_ms_scaled"] / b, 3) if "cpu_one_core" in v else "not measured"
        if v.get("parent_batch_rounds"):
            parent = v["parent_batch_rounds"]
            worst_batch, best_batch = max(r["max_ms"] for r in v["batch_rounds"]), min(r["min_ms"] for r in v["batch_rounds"])
            v["parent_batch_over_batch"] = {"median": round(statistics.median(r["median_ms_scaled"] for r in parent) / b, 2),
                                            "min": round(min(r["min_ms_scaled"] for r in parent) / worst_batch, 2),
                                            "max": round(max(r["max_ms_scaled"] for r in parent) / best_batch, 2)}
            v["every_run_beats_every_parent_run"] = bool(worst_batch < min(r["min_ms_scaled"] for r in parent))
        else:
            v["parent_batch_over_batch"] = "not measured"
    save()
    print(json.dumps(doc, indent=1))


def main_dicts(args, doc, save, classes):
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaries (a custom dictionary per item, every chain files its own) vs the loop of stream-API calls with "
                   "BrotliEncoderSetCustomDictionary, each item with its own dictionary (1 and 4 threads, first --loop-items items scaled by item count) vs the "
                   "oracle's dictionary stream on one CPU core; and, on the same items behind ONE dictionary, the call with that dictionary as `count` "
                   "distinct indices (self-filing) vs BrotliMi355xCompressBatchWithDictionary (the shared image); at qualities 2 to 4 with "
                   "BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, the shared call with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS; text, lgwin 22")
    rows = {}
    short = ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")
    for rnd in range(args.rounds):
        for what in ("batch", "same", "shared"):
            for row in run_child(args, what, classes, limit=900):
                v = rows.setdefault(key(row), {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": row["dictionary_bytes"]})
                v.setdefault(what + "_rounds", []).append({k: row[k] for k in short})
                if rnd == 0:
                    v[what + "_info"] = row["batch_info"]
                    v[what + "_compressed_bytes"] = row["compressed_bytes"]
                    v[what + "_reference_fails_on_items"] = row["reference_fails_on_items"]
            doc["classes"] = rows
            save()
        for threads in (1, 4):
            if "loop" in args.skip.split(","):
                continue
            for row in run_child(args, "loop", classes, lib=os.path.abspath(args.parent_lib) if args.parent_lib else None, threads=threads, limit=900):
                scale = row["items"] / row["measured_items"]
                rows[key(row)].setdefault("loop_%dt_rounds" % threads, []).append(
                    {"median_ms_scaled": round(row["median_ms"] * scale, 3), "min_ms_scaled": round(row["min_ms"] * scale, 3), "max_ms_scaled": round(row["max_ms"] * scale, 3),
                     "spread_pct": row["spread_pct"], "measured_items": row["measured_items"]})
            save()
    for row in ([] if "cpu" in args.skip.split(",") else run_child(args, "cpu", classes, limit=900)):
        scale = row["items"] / row["measured_items"]
        rows[key(row)]["cpu_one_core"] = {"median_ms_scaled": round(row["median_ms"] * scale, 3), "measured_items": row["measured_items"], "spread_pct": row["spread_pct"]}
    # the items the call failed alone, against the oracle on this host's CPU: its dictionary stream must fail on every one of them and
    # on none of their neighbours (the loop and the CPU baseline run the first --loop-items items only)
    os.environ["ORC_FAST"] = "1"
    import orc
    for k, v in rows.items():
        flagged = v["batch_reference_fails_on_items"]
        v["batch_reference_fails_on_items_verified"] = "none flagged"
        if not flagged:
            continue
        items, dictionaries = dicts_of(k.split("/")[0])

        def fails(i):
            try:
                orc.stream_with_flushes(items[i], [(0, 0), (1, int(k.split("/")[2][1:])), (2, LGWIN)], [], dictionary=dictionaries[i])
            except orc.ReferencePanics:
                return True
            return False

        neighbours = [i + 1 for i in flagged if i + 1 < len(items) and i + 1 not in flagged]
        assert all(fails(i) for i in flagged), (k, "the batch call failed an item the oracle encodes")
        assert not any(fails(i) for i in neighbours), (k, "the oracle fails on an item the batch call encoded")
        v["batch_reference_fails_on_items_verified"] = "the oracle fails on all %d flagged items and on none of %d neighbours" % (len(flagged), len(neighbours))
    for v in rows.values():
        med = {w: statistics.median(r["median_ms"] for r in v[w + "_rounds"]) for w in ("batch", "same", "shared")}
        v["batch_median_ms"], v["same_median_ms"], v["shared_median_ms"] = med["batch"], med["same"], med["shared"]
        v["batch_MBps"] = round(v["bytes"] / 1e3 / med["batch"], 1)
        v["self_filing_over_image"] = round(med["same"] / med["shared"], 3)
        v["same_bytes_as_shared"] = bool(v["same_compressed_bytes"] == v["shared_compressed_bytes"])
        v["cpu_over_batch"] = round(v["cpu_one_core"]["median_ms_scaled"] / med["batch"], 3) if "cpu_one_core" in v else "not measured"
        for threads in (1, 4):
            loop = v.get("loop_%dt_rounds" % threads)
            v["loop_%dt_over_batch" % threads] = round(statistics.median(r["median_ms_scaled"] for r in loop) / med["batch"], 2) if loop else "not measured"
        loops = [v[n] for n in ("loop_1t_rounds", "loop_4t_rounds") if v.get(n)]
        if loops:
            v["every_run_beats_every_loop_run"] = bool(max(r["max_ms"] for r in v["batch_rounds"]) < min(r["min_ms_scaled"] for rs in loops for r in rs))
    save()
    print(json.dumps(doc, indent=1))


def main_dicts_zopfli(args, doc, save, classes):
    """--dicts --qualities 10,11: BrotliMi355xCompressBatchWithDictionaries with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS, every item behind a
    dictionary of its own, --rounds alternating rounds of one run each: this build with the route (the wave-wide prepend), this build with
    BROTLI_MI355X_ZOPFLI_PREPEND_LANE0=1 on the A/B classes, the parent's library through the same call without the bit (its items run one by one: the
    first --loop-items items, scaled by item count), and the loop of stream calls from four threads (first --loop-items items, scaled); then the
    oracle on one core."""
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaries with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS (1024), a custom dictionary per item, text, "
                   "lgwin 22, qualities 10 and 11; min .. max over --rounds alternating rounds of one run each (one warm-up call per process).  parent: a build "
                   "of the parent commit through the same call with routes 0 -- every item one by one through the stream path -- TIMED ON THE FIRST "
                   "--loop-items ITEMS AND SCALED BY ITEM COUNT; loop_4t: the loop of stream calls with BrotliEncoderSetCustomDictionary from four threads, "
                   "first --loop-items items, scaled; cpu_one_core: the oracle's dictionary stream on one core, first --loop-items items, scaled; "
                   "prepend_lane0: this build with BROTLI_MI355X_ZOPFLI_PREPEND_LANE0=1 (the dictionary filed by lane 0 alone inside the same kernel)")
    rows = {}
    ab = [c for c in DICTS_ZOPFLI_AB if c in classes]
    one = argparse.Namespace(**vars(args))
    one.runs, one.warmup = 1, 1
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None

    def note(v, name, ms, scale=1.0):
        v.setdefault(name + "_ms", []).append(round(ms * scale, 3))

    for rnd in range(args.rounds):
        for row in run_child(one, "batch", classes, limit=900, routes=1024):
            v = rows.setdefault(key(row), {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": row["dictionary_bytes"]})
            note(v, "route", row["median_ms"])
            v["route_info"], v["route_compressed_bytes"], v["route_reference_fails_on_items"] = row["batch_info"], row["compressed_bytes"], row["reference_fails_on_items"]
        for row in (run_child(one, "batch", ab, limit=900, routes=1024, extra_env={"BROTLI_MI355X_ZOPFLI_PREPEND_LANE0": "1"}) if ab else []):
            note(rows[key(row)], "prepend_lane0", row["median_ms"])
            rows[key(row)]["prepend_lane0_same_bytes"] = bool(row["compressed_bytes"] == rows[key(row)]["route_compressed_bytes"])
        for row in (run_child(one, "batch_first", classes, lib=parent, limit=1500) if parent else []):
            note(rows[key(row)], "parent_scaled", row["median_ms"], row["items"] / row["measured_items"])
            rows[key(row)]["parent_measured_items"], rows[key(row)]["parent_info"] = row["measured_items"], row["batch_info"]
        for row in ([] if "loop" in args.skip.split(",") else run_child(one, "loop", classes, lib=parent, threads=4, limit=1500)):
            note(rows[key(row)], "loop_4t_scaled", row["median_ms"], row["items"] / row["measured_items"])
        doc["classes"] = rows
        save()
    for row in ([] if "cpu" in args.skip.split(",") else run_child(one, "cpu", classes, limit=1500)):
        rows[key(row)]["cpu_one_core_scaled_ms"] = round(row["median_ms"] * row["items"] / row["measured_items"], 3)
        rows[key(row)]["cpu_measured_items"] = row["measured_items"]
    for v in rows.values():
        for name in ("route", "prepend_lane0", "parent_scaled", "loop_4t_scaled"):
            if name + "_ms" in v:
                v[name + "_min_max_ms"] = [min(v[name + "_ms"]), max(v[name + "_ms"])]
        med = statistics.median(v["route_ms"])
        for name, out in (("parent_scaled", "parent_over_route"), ("loop_4t_scaled", "loop_4t_over_route"), ("prepend_lane0", "lane0_over_wave_wide")):
            if name + "_ms" in v:
                v[out] = round(statistics.median(v[name + "_ms"]) / med, 2)
        if "cpu_one_core_scaled_ms" in v:
            v["cpu_over_route"] = round(v["cpu_one_core_scaled_ms"] / med, 3)
    save()
    print(json.dumps(doc, indent=1))


def main_shared_zopfli(args, doc, save, classes):
    """--shared-zopfli: see the module's text"""
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (8192), every item behind ONE shared "
                   "dictionary (the class's first), text, lgwin 22, qualities 10 and 11; min .. max over --rounds alternating rounds of one run each (one warm-up "
                   "call per process).  image: the default, one tree image per call, replayed by every chain; self_file: BROTLI_MI355X_BATCH_DICT_SELF_FILE=1, "
                   "every chain files the dictionary itself; parent_one_index: a build of the parent commit through BrotliMi355xCompressBatchWithDictionaries "
                   "with 1024 and one index named by every item -- the self-filing baseline; one_by_one: this build's shared entry without the bit, TIMED ON THE "
                   "FIRST --loop-items ITEMS AND SCALED BY ITEM COUNT; on the one-item classes self_file_lane0 adds BROTLI_MI355X_ZOPFLI_PREPEND_LANE0=1, so that "
                   "self_file - image and self_file_lane0 - image are a lone chain's filing less the replay, as differences of whole calls.  prepend_entry: "
                   "brotli_mi355x_debug_zopfli_prepend by itself (host clock around the synchronous entry), modes 0 / 1 / 2 = lane 0 / wave-wide on one wavefront / "
                   "the image build; the row of 2 bytes is what every mode pays for allocation, fill and copies")
    doc["method"] = ("host clock around the synchronous call; every figure is min .. max over --rounds alternating rounds of ONE run each, each arm of a round in a child process of its own behind one warm-up call (the environment is read once per process); one_by_one on the first --loop-items items of a class, scaled by item count; prepend_entry: one child, one warm-up round, then --rounds rounds of modes 0, 1, 2 one after the other")
    rows = {}
    lone = [c for c in SHARED_ZOPFLI_LONE if not args.only or c in args.only.split(",")]
    one = argparse.Namespace(**vars(args))
    one.runs, one.warmup, one.dicts = 1, 1, True
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    self_file = {"BROTLI_MI355X_BATCH_DICT_SELF_FILE": "1"}

    def note(row, name, scale=1.0):
        v = rows.setdefault(key(row), {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": row["dictionary_bytes"]})
        v.setdefault(name + "_ms", []).append(round(row["median_ms"] * scale, 3))
        v[name + "_info"], v[name + "_compressed_bytes"] = row["batch_info"], row["compressed_bytes"]

    for rnd in range(args.rounds):
        for row in run_child(one, "shared", classes + lone, limit=900, routes=8192):
            note(row, "image")
        for row in run_child(one, "shared", classes + lone, limit=900, routes=8192, extra_env=self_file):
            note(row, "self_file")
        for row in (run_child(one, "shared", lone, limit=900, routes=8192, extra_env=dict(self_file, BROTLI_MI355X_ZOPFLI_PREPEND_LANE0="1")) if lone else []):
            note(row, "self_file_lane0")
        for row in (run_child(one, "one_index", classes, lib=parent, limit=900, routes=1024) if parent else []):
            note(row, "parent_one_index")
        for row in ([] if "loop" in args.skip.split(",") else run_child(one, "shared_first", classes, limit=1500)):
            note(row, "one_by_one_scaled", row["items"] / row["measured_items"])
            rows[key(row)]["one_by_one_measured_items"] = row["measured_items"]
        doc["classes"] = rows
        save()
    entry = argparse.Namespace(**vars(args))
    entry.runs, entry.warmup = max(args.rounds, 1), 1
    doc["prepend_entry"] = run_child(entry, "prepend", ["none"], limit=600)
    for v in rows.values():
        names = ("image", "self_file", "self_file_lane0", "parent_one_index", "one_by_one_scaled")
        for name in names:
            if name + "_ms" in v:
                v[name + "_min_max_ms"] = [min(v[name + "_ms"]), max(v[name + "_ms"])]
        med = statistics.median(v["image_ms"])
        for name in names[1:]:
            if name + "_ms" in v:
                v[name + "_over_image"] = round(statistics.median(v[name + "_ms"]) / med, 3)
        sizes = set(v[name + "_compressed_bytes"] for name in names[:4] if name + "_compressed_bytes" in v)
        v["same_compressed_bytes"] = bool(len(sizes) == 1)
        if "parent_one_index_ms" in v:
            # the rule of the default: no slower than the parent's self-filing by more than the spread of the runs
            v["image_within_parent_spread"] = bool(min(v["image_ms"]) <= max(v["parent_one_index_ms"]))
    save()
    print(json.dumps(doc, indent=1))


def main_dicts_q9(args, doc, save, classes):
    """--dicts --qualities 9: the dictionary batch calls with BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096), --rounds alternating rounds of
    one run each: this build with the route, every item behind a dictionary of its own; on the DICTS_Q9_SHARED classes the shared form (every item
    behind the first dictionary, BrotliMi355xCompressBatchWithDictionaryEx with 4096) with the image and with BROTLI_MI355X_BATCH_DICT_SELF_FILE=1;
    the parent's library through the per-item call without the bit (its items run one by one: the first --loop-items items, scaled by item
    count), and the loop of stream calls from four threads (first --loop-items items, scaled); then the oracle on one core."""
    doc["what"] = ("BrotliMi355xCompressBatchWithDictionaries with BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096), a custom dictionary per item, text, lgwin 22, "
                   "quality 9; min .. max over --rounds alternating rounds of one run each (one warm-up call per process).  shared_image / shared_self_file: "
                   "BrotliMi355xCompressBatchWithDictionaryEx with 4096, every item behind the class's first dictionary, the image replayed (the default) or "
                   "BROTLI_MI355X_BATCH_DICT_SELF_FILE=1; parent: a build of the parent commit through the per-item call with routes 0 -- every item one by one "
                   "through the stream path -- TIMED ON THE FIRST --loop-items ITEMS AND SCALED BY ITEM COUNT; loop_4t: the loop of stream calls with "
                   "BrotliEncoderSetCustomDictionary from four threads, first --loop-items items, scaled; cpu_one_core: the oracle's dictionary stream on "
                   "one core, first --loop-items items, scaled")
    rows = {}
    shared = [c for c in DICTS_Q9_SHARED if c in classes]
    one = argparse.Namespace(**vars(args))
    one.runs, one.warmup = 1, 1
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None

    def note(v, name, ms, scale=1.0):
        v.setdefault(name + "_ms", []).append(round(ms * scale, 3))

    for rnd in range(args.rounds):
        for row in run_child(one, "batch", classes, limit=900, routes=4096):
            v = rows.setdefault(key(row), {"items": row["items"], "bytes": row["bytes"], "dictionary_bytes": row["dictionary_bytes"]})
            note(v, "route", row["median_ms"])
            v["route_info"], v["route_compressed_bytes"], v["route_reference_fails_on_items"] = row["batch_info"], row["compressed_bytes"], row["reference_fails_on_items"]
        for name, env in (("shared_image", None), ("shared_self_file", {"BROTLI_MI355X_BATCH_DICT_SELF_FILE": "1"})):
            for row in (run_child(one, "shared", shared, limit=900, routes=4096, extra_env=env) if shared else []):
                note(rows[key(row)], name, row["median_ms"])
                rows[key(row)][name + "_info"], rows[key(row)][name + "_compressed_bytes"] = row["batch_info"], row["compressed_bytes"]
        for row in (run_child(one, "batch_first", classes, lib=parent, limit=1500) if parent else []):
            note(rows[key(row)], "parent_scaled", row["median_ms"], row["items"] / row["measured_items"])
            rows[key(row)]["parent_measured_items"], rows[key(row)]["parent_info"] = row["measured_items"], row["batch_info"]
        for row in ([] if "loop" in args.skip.split(",") else run_child(one, "loop", classes, lib=parent, threads=4, limit=1500)):
            note(rows[key(row)], "loop_4t_scaled", row["median_ms"], row["items"] / row["measured_items"])
        doc["classes"] = rows
        save()
    for row in ([] if "cpu" in args.skip.split(",") else run_child(one, "cpu", classes, limit=1500)):
        rows[key(row)]["cpu_one_core_scaled_ms"] = round(row["median_ms"] * row["items"] / row["measured_items"], 3)
        rows[key(row)]["cpu_measured_items"] = row["measured_items"]
    for v in rows.values():
        for name in ("route", "shared_image", "shared_self_file", "parent_scaled", "loop_4t_scaled"):
            if name + "_ms" in v:
                v[name + "_min_max_ms"] = [min(v[name + "_ms"]), max(v[name + "_ms"])]
        med = statistics.median(v["route_ms"])
        for name, out in (("parent_scaled", "parent_over_route"), ("loop_4t_scaled", "loop_4t_over_route"), ("shared_image", "shared_image_over_route")):
            if name + "_ms" in v:
                v[out] = round(statistics.median(v[name + "_ms"]) / med, 2)
        if "shared_image_ms" in v and "shared_self_file_ms" in v:
            v["self_file_over_image"] = round(statistics.median(v["shared_self_file_ms"]) / statistics.median(v["shared_image_ms"]), 3)
        if "cpu_one_core_scaled_ms" in v:
            v["cpu_over_route"] = round(v["cpu_one_core_scaled_ms"] / med, 3)
    save()
    print(json.dumps(doc, indent=1))


def main_same_call(args, doc, save, classes):
    """--same-call: this build and the parent's library through the very same call (route bits, dictionary), alternating, one child
    each -- for a change that keeps the routes and must not cost them anything.  Per class: the median of either build's round
    medians, and the parent's own run-to-run spread (the largest difference between its rounds) as the margin."""
    doc["what"] = "this build against the parent commit's library through the same batch call (%s), alternating, %d rounds; lgwin 22" % (
        ", ".join([n for n in ("long_items", "quick_items", "quick_long_items", "zopfli_items", "q9_items") if getattr(args, n)] +
                  (["a dictionary per item"] if args.dicts else ["a shared dictionary of %d bytes" % args.dictionary] if args.dictionary else [])) or "no route bit",
        args.rounds)
    routes = dict(long_items=args.long_items, quick_items=args.quick_items, quick_long_items=args.quick_long_items, zopfli_items=args.zopfli_items,
                  q9_items=args.q9_items)
    rows = {}
    for rnd in range(args.rounds):
        for name, lib in (("this_rounds", args.lib), ("parent_rounds", os.path.abspath(args.parent_lib))):
            for row in run_child(args, "batch", classes, lib=lib, limit=900, **routes):
                v = rows.setdefault(key(row), {"items": row["items"], "bytes": row["bytes"]})
                v.setdefault(name, []).append({k: row[k] for k in ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")})
                # (the same streams from both builds, in every round)
                assert v.setdefault("compressed_bytes", row["compressed_bytes"]) == row["compressed_bytes"], row
        doc["classes"] = rows
        save()
    for v in rows.values():
        this, parent = [r["median_ms"] for r in v["this_rounds"]], [r["median_ms"] for r in v["parent_rounds"]]
        v["this_median_ms"], v["parent_median_ms"] = statistics.median(this), statistics.median(parent)
        v["margin_ms"] = round(max(parent) - min(parent), 3)
        v["this_minus_parent_ms"] = round(v["this_median_ms"] - v["parent_median_ms"], 3)
        v["inside_margin"] = bool(v["this_minus_parent_ms"] <= v["margin_ms"])
    save()
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rust-brotli_amd", "libbrotli_mi355x.so"))
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit (the loop baseline); without it the loop is not measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_probe.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-items", type=int, default=256)
    ap.add_argument("--ab-rounds", type=int, default=3, help="how often the A/B alternates between the two settings")
    ap.add_argument("--skip", default="", help="comma list of: headline, ab, cpu, loop")
    ap.add_argument("--qualities", default="0,1", help="comma list of qualities")
    ap.add_argument("--rounds", type=int, default=1, help="how often this build and the parent's batch call alternate (qualities other than 0 and 1)")
    ap.add_argument("--only", default="", help="comma list of headline classes (default: all)")
    ap.add_argument("--first-only", action="store_true")
    ap.add_argument("--dictionary", type=int, default=0, help="bytes of shared custom dictionary: measures BrotliMi355xCompressBatchWithDictionary")
    ap.add_argument("--long-items", action="store_true", help="this build through BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS")
    ap.add_argument("--quick-items", action="store_true", help="this build through BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS (--qualities 2,3,4)")
    ap.add_argument("--quick-long-items", action="store_true", help="this build through routes QUICK_ITEMS | QUICK_LONG_ITEMS, the parent through QUICK_ITEMS (qualities 2,3,4 per class)")
    ap.add_argument("--zopfli-items", action="store_true", help="this build through BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS (--qualities 11)")
    ap.add_argument("--q9-items", action="store_true", help="this build through BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS (--qualities 9,10)")
    ap.add_argument("--dicts", action="store_true", help="BrotliMi355xCompressBatchWithDictionaries: a dictionary per item (--qualities 5,8; 2,3,4 through BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS; 10,11 through BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS; 9 through BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS, shared form included, "
                    "with the prepend A/B and, with --parent-lib, the parent's one-by-one path on --loop-items items)")
    ap.add_argument("--shared-zopfli", action="store_true", help="BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS: the tree image against self-filing, the parent's one-index call and one by one (qualities 10,11)")
    ap.add_argument("--device", action="store_true", help="BrotliMi355xCompressBatchDevice on torch tensors beside the parent's host call on the same items (DEVICE_SHAPES)")
    ap.add_argument("--device-dicts", action="store_true", help="BrotliMi355xCompressBatchWithDictionariesDevice on torch tensors beside download + the parent's host dictionary call + upload (DEVICE_DICTS_SHAPES)")
    ap.add_argument("--kinds", default="", help="with --dicts: K distinct dictionaries, the items dealt to them round robin -- a comma list (with --only and --qualities), "
                    "'all' (KINDS_SHAPES and the sweep of BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS) or 'sweep'; --rounds alternating rounds against --parent-lib")
    ap.add_argument("--routes", type=int, default=0, help="(child) route bits of the device shape")
    ap.add_argument("--shared", action="store_true", help="(child, device-dicts) one dictionary named by every item")
    ap.add_argument("--same-call", action="store_true", help="the parent's library through the same call as this build, alternating --rounds times (needs --parent-lib)")
    ap.add_argument("--quick-long-classes", action="store_true", help="(child) only the qualities of QUICK_LONG_QUALITIES")
    ap.add_argument("--plain", action="store_true", help="(child) the plain call although a dictionary size is given")
    ap.add_argument("--child", default=None)
    ap.add_argument("--classes", default="")
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    skip = set(args.skip.split(","))
    doc = {"what": "BrotliMi355xCompressBatch vs a loop of BrotliEncoderCompress (parent commit) vs the oracle on one CPU core; lgwin 22",
           "method": "host clock around the synchronous call, %d warm-up runs, median of %d runs; spread = (max - min) / median of the repeats; "
                     "loop and cpu on the first %d items of a class, scaled by item count" % (args.warmup, args.runs, args.loop_items)}

    def save():
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    if args.dicts and args.kinds:
        return main_kinds(args, doc, save)
    if args.device:
        return main_device(args, doc, save)
    if args.device_dicts:
        return main_device_dicts(args, doc, save)
    if args.quick_long_items:
        args.quick_items = True
        args.qualities = "2,3,4"
    headline = [c for c in (args.only.split(",") if args.only else (list(QUICK_LONG_QUALITIES) if args.quick_long_items else QUICK_HEADLINE if args.quick_items else ZOPFLI_HEADLINE if args.zopfli_items else Q9_HEADLINE if args.q9_items else HEADLINE)) if c in CLASSES]
    if args.long_items:
        doc["what"] = "BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS) vs the parent commit's batch call and 4-thread loop vs the oracle on one CPU core; lgwin 22"
    if args.quick_items:
        doc["what"] = "BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS) vs the parent commit's batch call and 4-thread loop vs the oracle on one CPU core; lgwin 22"
    if args.quick_long_items:
        doc["what"] = ("BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS | BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS) vs the parent commit's "
                       "BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS), there one by one; items of two to four input blocks; lgwin 22")
    if args.zopfli_items:
        doc["what"] = ("BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS) vs the parent commit's batch call, there one by one (on the first "
                       "--loop-items items, scaled by item count), vs the oracle on one CPU core; lgwin 22")
    if args.q9_items:
        doc["what"] = ("BrotliMi355xCompressBatchEx(BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS) vs the parent commit's batch call, there one by one (on the first "
                       "--loop-items items, scaled by item count), and its 4-thread loop vs the oracle on one CPU core; lgwin 22")
    if args.shared_zopfli:
        if not set(args.qualities.split(",")) <= {"10", "11"}:
            args.qualities = "10,11"
        return main_shared_zopfli(args, doc, save, [c for c in SHARED_ZOPFLI_HEADLINE if not args.only or c in args.only.split(",")])
    if args.dicts and not args.same_call and set(args.qualities.split(",")) <= {"10", "11"}:
        return main_dicts_zopfli(args, doc, save, [c for c in DICTS_ZOPFLI_HEADLINE if not args.only or c in args.only.split(",")])
    if args.dicts and not args.same_call and set(args.qualities.split(",")) == {"9"}:
        return main_dicts_q9(args, doc, save, [c for c in DICTS_Q9_HEADLINE if not args.only or c in args.only.split(",")])
    if args.dicts and not args.same_call:
        return main_dicts(args, doc, save, [c for c in DICTS_CLASSES if (c in args.only.split(",") if args.only else (c not in DICTS_ZOPFLI_HEADLINE and c != "256x64KiB+64KiB" and c not in DICTS_Q9_FEW) or c == "64x4KiB+16KiB")])
    if args.same_call:
        if args.dicts:  # (the per-item call, every item behind its own dictionary)
            return main_same_call(args, doc, save, [c for c in DICTS_CLASSES if not args.only or c in args.only.split(",")])
        dict_classes = DICT_QUICK_HEADLINE if args.quick_items else ["4096x4KiB", "1024x64KiB"]
        return main_same_call(args, doc, save, (headline if args.only else dict_classes) if args.dictionary else headline)
    if args.dictionary and args.quick_items:
        return main_dictionary_quick(args, doc, save, [c for c in DICT_QUICK_HEADLINE if not args.only or c in args.only.split(",")])
    if args.dictionary:
        return main_dictionary(args, doc, save, [c for c in ("4096x4KiB", "1024x64KiB") if not args.only or c in args.only.split(",")])
    fragment_qualities = set(args.qualities.split(",")) <= {"0", "1"}
    if "ab" not in skip and fragment_qualities:
        # the table's home: device memory (0) against workgroup memory (11, the largest the library keeps there), the same jobs,
        # alternating: device, workgroup, device, workgroup ... one child each
        ab = {}
        for rnd in range(args.ab_rounds):
            for lds in (0, 11):
                for row in run_child(args, "batch", AB, lds=lds):
                    ab.setdefault(key(row), {}).setdefault("lds%d_ms" % lds, []).append(row["median_ms"])
                    ab[key(row)].setdefault("spread_pct", []).append(row["spread_pct"])
        for k, v in ab.items():
            a, b = statistics.median(v["lds0_ms"]), statistics.median(v["lds11_ms"])
            v["workgroup_over_device"] = round(b / a, 4)
            # the spread a difference has to beat: the largest of the repeats inside a child and of the children of either arm
            v["repeat_spread_pct"] = round(max(max(v.pop("spread_pct")), 100.0 * (max(v["lds0_ms"]) - min(v["lds0_ms"])) / a,
                                               100.0 * (max(v["lds11_ms"]) - min(v["lds11_ms"])) / b), 2)
            v["workgroup_wins"] = bool(100.0 * (1.0 - b / a) > v["repeat_spread_pct"])
        doc["table_home_ab"] = ab
        save()
    if "headline" not in skip:
        rows = {}
        for rnd in range(args.rounds):
            for row in run_child(args, "batch", headline, limit=900, long_items=args.long_items, quick_items=args.quick_items, quick_long_items=args.quick_long_items,
                                 zopfli_items=args.zopfli_items, q9_items=args.q9_items):
                this = {k: row[k] for k in ("median_ms", "min_ms", "max_ms", "spread_pct", "runs")}
                if rnd == 0:
                    rows[key(row)] = {"items": row["items"], "bytes": row["bytes"], "compressed_bytes": row["compressed_bytes"], "batch_info": row["batch_info"], "batch": this}
                rows[key(row)].setdefault("batch_rounds", []).append(this)
            doc["classes"] = rows
            save()
            if args.parent_lib and not fragment_qualities:
                # the parent's own batch call: a loop over its one-shot path on the calling thread
                # (--quick-long-items: through the quick route, which takes these items one by one there as well)
                for row in run_child(args, "batch", headline, lib=os.path.abspath(args.parent_lib), limit=900, first_only=True, quick_items=args.quick_long_items):
                    scale = row["items"] / row["measured_items"]
                    rows[key(row)].setdefault("parent_batch_rounds", []).append({"median_ms_scaled": round(row["median_ms"] * scale, 3), "min_ms_scaled": round(row["min_ms"] * scale, 3),
                                                                               "max_ms_scaled": round(row["max_ms"] * scale, 3), "spread_pct": row["spread_pct"], "measured_items": row["measured_items"]})
                save()
        for row in ([] if "cpu" in skip else run_child(args, "cpu", headline)):
            scale = row["items"] / row["measured_items"]
            rows[key(row)]["cpu_one_core"] = {"median_ms_scaled": round(row["median_ms"] * scale, 3), "measured_items": row["measured_items"], "spread_pct": row["spread_pct"]}
        save()
        for threads in (1, 4):
            if not args.parent_lib or "loop" in skip:
                for v in rows.values():
                    v["loop_%dt" % threads] = "not measured"
                continue
            if threads == 1 and not fragment_qualities:
                continue  # (the parent's batch call above is that loop)
            for row in run_child(args, "loop", headline, lib=os.path.abspath(args.parent_lib), threads=threads, limit=900):
                scale = row["items"] / row["measured_items"]
                rows[key(row)]["loop_%dt" % threads] = {"median_ms_scaled": round(row["median_ms"] * scale, 3), "min_ms_scaled": round(row["min_ms"] * scale, 3), "measured_items": row["measured_items"], "spread_pct": row["spread_pct"]}
            save()
        for k, v in rows.items():
            b = v["batch"]["median_ms"]
            loops = [v[n]["median_ms_scaled"] for n in ("loop_1t", "loop_4t") if isinstance(v.get(n), dict)]
            v["batch_MBps"] = round(v["bytes"] / 1e3 / b, 1)
            v["cpu_over_batch"] = round(v["cpu_one_core"]["median_ms_scaled"] / b, 3) if "cpu_one_core" in v else "not measured"
            v["better_loop_over_batch"] = round(min(loops) / b, 2) if loops else "not measured"
            if v.get("parent_batch_rounds"):
                parent = v["parent_batch_rounds"]
                v["parent_batch_over_batch"] = round(statistics.median(r["median_ms_scaled"] for r in parent) / statistics.median(r["median_ms"] for r in v["batch_rounds"]), 2)
                v["every_run_beats_every_parent_run"] = bool(max(r["max_ms"] for r in v["batch_rounds"]) < min(r["min_ms_scaled"] for r in parent))
            if isinstance(v.get("loop_4t"), dict) and "min_ms_scaled" in v["loop_4t"]:
                v["every_run_beats_every_loop_4t_run"] = bool(max(r["max_ms"] for r in v["batch_rounds"]) < v["loop_4t"]["min_ms_scaled"])
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
