"""BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS (8192): many small items
behind ONE shared custom dictionary at qualities 10 and 11, side by side on one tree image.

Item i is the stream of BrotliEncoderSetCustomDictionary(dict) + one BrotliEncoderCompressStream(FINISH): the oracle's stream API
with that dictionary.  With the route set, at lgwin 10 to 24, an item of 1 to 65 536 bytes behind a dictionary of at least 2 bytes
of which at most 65 536 are in use runs side by side on the device.  The dictionary's part of the H10 trees hangs on the dictionary
alone, so the call builds ONE image of it (buckets and forest: lanes of several workgroups, each owning a class of hash keys) and
every chain copies it over its own table in front of every item, where the per-item call files the dictionary per chain
(batch_zopfli.h).  The per-item calls take the same path when every item names one index.  Every other item goes one by one through
the stream path in the same call.  No item is skipped or tolerated: every stream equals the oracle's, and an oracle failure on one
of these inputs is a test error.  BrotliMi355xLastBatchInfo proves which path was taken.  The image and its replay are also pinned
by themselves (brotli_mi355x_debug_zopfli_prepend, modes 2 and 3) against the one-lane loop.  The CPU tests run the emulation
library -- the same host plan and item code, the image build class by class --, the GPU tests the product library; there no
side-by-side item exceeds 8 KiB and no dictionary 20 000 bytes, the 64 KiB sizes run on the emulation only."""
import ctypes
import hashlib
import os
import subprocess
import sys
import threading
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_uint32, c_void_p

import pytest

import synth
import test_batch_device
import test_cabi
from test_batch_dictionaries_zopfli import _caps, _in_use, _info, _raw, _side_by_side
from test_batch_dictionary import _oracle

HERE = os.path.dirname(os.path.abspath(__file__))
QUICK, Q9, ZS = 4, 4096, 8192  # ..._ROUTE_QUICK_ITEMS, ..._ROUTE_Q9_DICTIONARY_ITEMS, ..._ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS
ZD = 1024  # BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS: the per-item calls' bit, unknown to the shared entry
GUARD = 64
FILL = 0xAA


def _shared(lib, quality, lgwin, routes, dictionary, items, caps=None, with_results=True, mode=0):
    """BrotliMi355xCompressBatchWithDictionaryEx through ctypes: (return value, [bytes], [item result], [size], info)"""
    caps = _caps(lib, items) if caps is None else caps
    n = len(items)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionaryEx(quality, lgwin, mode, c_uint32(routes), c_size_t(len(dictionary)), dictionary, c_size_t(n), inputs,
                                                            in_sizes, outputs, out_sizes, results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n], _info(lib)


def _check(lib, items, dictionary, quality, lgwin, routes=ZS):
    """every stream the oracle's, info = [n, side, n - side, 0, >= 1, in use, 0, 0]; returns (streams, info)"""
    want = [_oracle(x, quality, lgwin, dictionary) for x in items]
    ret, got, results, sizes, info = _shared(lib, quality, lgwin, routes, dictionary, items)
    assert ret == 1 and results == [1] * len(items), (quality, lgwin, results, lib.last_error())
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (quality, lgwin, i, len(items[i]), len(dictionary), len(g), len(w))
    side = sum(1 for x in items if _side_by_side(x, quality, lgwin, dictionary))
    assert info[:4] == [len(items), side, len(items) - side, 0] and info[5:] == [_in_use(quality, lgwin, dictionary), 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got, info


def _items(gpu):
    a = synth.alice()
    items = [b"", b"x", a[30000:35000], a[30000:30000 + 8192], synth.random_bytes(3000)]
    if not gpu:
        items += [a[1000:1000 + 65536], a[1000:1000 + 65537]]
    return items


# ---- 1. taken side by side (fails where 8192 is an unknown route of the call: the call returns 0)

def _taken_side_by_side(lib, gpu):
    a = synth.alice()
    dictionary = a[:16384]
    items = _items(gpu)
    n = len(items)
    side = n - 1 - (0 if gpu else 1)  # all but the empty item and the one of 65 537 bytes
    caps = _caps(lib, items)
    for quality in (10, 11):
        for lgwin in (22, 16):
            in_use = _in_use(quality, lgwin, dictionary)
            got, info = _check(lib, items, dictionary, quality, lgwin)
            assert info[:4] == [n, side, n - side, 0] and info[4] >= 1 and info[5:] == [in_use, 0, 0], (quality, lgwin, info)
            # routes == 0: the same bytes, nothing side by side
            ret, outs, results, _, plain = _shared(lib, quality, lgwin, 0, dictionary, items, caps)
            assert ret == 1 and results == [1] * n and outs == got, (quality, lgwin)
            assert plain == [n, 0, n, 0, 0, in_use, 0, 0], (quality, lgwin, plain)
            # 8192 | 4 | 4096 behaves as 8192 alone
            ret, outs, results, _, both = _shared(lib, quality, lgwin, ZS | QUICK | Q9, dictionary, items, caps)
            assert ret == 1 and results == [1] * n and outs == got and both == info, (quality, lgwin, both, info)
    small, small_caps = items[:5], caps[:5]
    # the bit changes nothing at qualities 2, 5 and 9: the same bytes and the same info as without it
    for quality in (2, 5, 9):
        want = [_oracle(x, quality, 22, dictionary) for x in small]
        ret, outs, _, _, plain = _shared(lib, quality, 22, 0, dictionary, small, small_caps)
        assert ret == 1 and outs == want and plain[:4] == ([5, 4, 1, 0] if quality == 5 else [5, 0, 5, 0]), (quality, plain)
        ret, outs, _, _, info = _shared(lib, quality, 22, ZS, dictionary, small, small_caps)
        assert ret == 1 and outs == want and info == plain, (quality, info, plain)
    # a route this call does not know fails the whole call, and only info[0] is set: also beside the one it knows
    for routes in (ZD, 2048, ZS | 1, 1 << 31):
        ret, outs, results, sizes, info = _shared(lib, 11, 22, routes, dictionary, small, small_caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert info == [5, 0, 0, 0, 0, 0, 0, 0], routes
        assert "routes %d" % routes in lib.last_error()
    # ... and 8192 is an unknown route of the other batch calls
    bufs = [ctypes.create_string_buffer(c) for c in small_caps]
    inputs, in_sizes = (c_char_p * 5)(*small), (c_size_t * 5)(*[len(x) for x in small])
    outputs = (c_void_p * 5)(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * 5)(*small_caps)
    results = (c_int32 * 5)(*([7] * 5))
    ret = lib.lib.BrotliMi355xCompressBatchEx(11, 22, 0, c_uint32(ZS), c_size_t(5), inputs, in_sizes, outputs, out_sizes, results)
    assert ret == 0 and list(results) == [0] * 5 and list(out_sizes) == [0] * 5 and "route" in lib.last_error()
    assert _info(lib) == [5, 0, 0, 0, 0, 0, 0, 0]
    for routes in (ZS, ZS | ZD):
        ret, outs, results, sizes, info = _raw(lib, 11, 22, routes, [dictionary], [0] * 5, small, small_caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5 and "routes %d" % routes in lib.last_error(), routes
        assert info == [5, 0, 0, 0, 0, 0, 0, 0], routes


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"), True)


# ---- 2. equal to the one-index call: the per-item entries with 1024 and item_dicts = [0] * n take the same path -- identical bytes,
# results and info, on host and on device memory (canaries around every output untouched)

def _equal_to_one_index(lib, which):
    Mem = test_batch_device._mem(which)
    a = synth.alice()
    dictionary = a[:16384]
    items = _items(which == "gpu")
    n = len(items)
    caps = _caps(lib, items)
    blocks, at = [], 3
    for blob in [dictionary] + items:
        blocks.append(at)
        at += len(blob) + 5
    src = Mem(at, 0)
    for off, blob in zip(blocks, [dictionary] + items):
        src.write(off, blob)
    out_at, at = [], GUARD
    for c in caps:
        out_at.append(at)
        at += c + GUARD
    for quality, lgwin in ((10, 22), (11, 22), (11, 16)):
        want = [_oracle(x, quality, lgwin, dictionary) for x in items]
        shared = _shared(lib, quality, lgwin, ZS, dictionary, items, caps)
        assert shared[0] == 1 and shared[1] == want, (quality, lgwin)
        # (the other two dictionaries are named by nobody: they count nowhere)
        named = _raw(lib, quality, lgwin, ZD, [dictionary, a[:100], b""], [0] * n, items, caps)
        assert named == shared, (quality, lgwin, named[2:], shared[2:])
        dst = Mem(at, FILL)
        Mem.sync()
        dict_ptrs = (c_void_p * 1)(src.ptr + blocks[0])
        dict_sizes = (c_size_t * 1)(len(dictionary))
        in_ptrs = (c_void_p * n)(*[src.ptr + o for o in blocks[1:]])
        in_sizes = (c_size_t * n)(*[len(x) for x in items])
        out_ptrs = (c_void_p * n)(*[dst.ptr + o for o in out_at])
        out_sizes = (c_size_t * n)(*caps)
        results = (c_int32 * n)(*([7] * n))
        ret = lib.lib.BrotliMi355xCompressBatchWithDictionariesDevice(quality, lgwin, 0, c_uint32(ZD), c_size_t(1), dict_ptrs, dict_sizes, c_size_t(n),
                                                                      (c_size_t * n)(*([0] * n)), in_ptrs, in_sizes, out_ptrs, out_sizes, results)
        info = _info(lib)
        assert (ret, list(results), list(out_sizes), info) == (shared[0], shared[2], shared[3], shared[4]), (quality, lgwin, lib.last_error())
        image = dst.read()
        covered = bytearray(len(image))
        for o, cap, size, w in zip(out_at, caps, shared[3], want):
            assert image[o:o + size] == w, (quality, lgwin)
            covered[o:o + cap] = b"\x01" * cap
        # (a byte outside every [out, out + capacity) still holds the fill)
        assert all(image[i] == FILL for i in range(len(image)) if not covered[i]), (quality, lgwin)


def test_equal_to_one_index_emu():
    _equal_to_one_index(test_cabi._load("emu"), "emu")


@pytest.mark.gpu
def test_equal_to_one_index_gpu():
    _equal_to_one_index(test_cabi._load("gpu"), "gpu")


# ---- 3. image parity (fails where modes 2 and 3 of the debug entry are refused): the image build of several workgroups leaves the
# buckets and the forest of the one-lane loop, bit for bit, and the replay lays them over a used table with the item's slots zeroed

_IMAGE_D = (2, 3, 126, 127, 128, 129, 190, 191, 192, 193, 255, 256, 257, 1000, 4099, 8192)
_IMAGE_ITEMS = (1, 63, 64, 65, 700)


def _slots(n, lgwin):
    return min((n + 63) & ~63, 1 << lgwin)


def _prepend(lib, text, D, lgwin, mode):
    slots = _slots(len(text) if mode == 3 else D, lgwin)
    buckets = (c_uint32 * (1 << 17))()
    forest = (c_uint32 * max(1, 2 * slots))()
    ret = lib.lib.brotli_mi355x_debug_zopfli_prepend(text, c_uint32(len(text)), c_uint32(D), c_uint32(lgwin), c_uint32(mode), buckets, forest)
    assert ret == 0, (ret, D, lgwin, mode)
    return bytes(buckets), bytes(forest)[:8 * slots]


def _has_word(blob, word):
    at = blob.find(word)
    while at >= 0 and at % 4 != 0:
        at = blob.find(word, at + 1)
    return at >= 0


def _image_sources(gpu):
    sources = [("text", synth.alice()[1000:1000 + (8192 if gpu else 65536) + 700]), ("random", synth.random_bytes(8192 + 700)), ("a", b"a" * (8192 + 700))]
    return [(name, src, _IMAGE_D + (() if gpu or name != "text" else (65536,))) for name, src in sources]


def _image_parity(lib, other=None):
    stale = b"\xa5" * 4
    for lgwin in (22, 10):
        invalid = (0x100000000 - ((1 << lgwin) - 1)).to_bytes(4, "little")
        for name, src, sizes in _image_sources(other is not None):
            for D in sizes:
                D = min(D, (1 << lgwin) - 16)
                lane0 = _prepend(lib, src[:D + 1], D, lgwin, 0)
                image = _prepend(lib, src[:D + 1], D, lgwin, 2)
                assert image == lane0, (lgwin, name, D)
                assert (D >= 128) == (lane0[0] != invalid * (1 << 17)), (lgwin, name, D)  # (something was stored)
                if other is not None:
                    assert _prepend(other, src[:D + 1], D, lgwin, 2) == image, (lgwin, name, D)
                for n in _IMAGE_ITEMS:
                    buckets, forest = _prepend(lib, src[:D + n], D, lgwin, 3)
                    assert buckets == lane0[0], (lgwin, name, D, n)
                    assert len(forest) == 8 * _slots(D + n, lgwin) and forest == lane0[1] + bytes(len(forest) - len(lane0[1])), (lgwin, name, D, n)
                    # (nothing of the table's earlier contents is left in the written range)
                    assert not _has_word(buckets, stale) and not _has_word(forest, stale), (lgwin, name, D, n)


def test_image_parity_emu():
    _image_parity(test_cabi._load("emu"))


@pytest.mark.gpu
def test_image_parity_gpu():
    _image_parity(test_cabi._load("gpu"), test_cabi._load("emu"))


# ---- 4. edges through the call: the prepend's first stored position (D = 128), the stitch's threshold (128 dictionary bytes, 3 item
# bytes), partial copy steps, store_end (128 item bytes); the items are the text that follows the dictionary, so matches straddle
# dict_break.  At lgwin 10 a dictionary is cut to its last 1008 bytes and the forest wraps inside the 700-byte item.

_EDGE_D = _IMAGE_D[:-1]  # up to 4099
_EDGE_ITEMS = (1, 2, 3, 4, 6, 7, 8, 127, 128, 129, 700)
_EDGE_CASES = [(10, 22), (11, 22), (10, 10), (11, 10)]


def _edges(lib, quality, lgwin):
    a = synth.alice()
    for k, D in enumerate(_EDGE_D):
        at = 9000 + 531 * k
        items = [a[at + D:at + D + n] for n in _EDGE_ITEMS]
        got, info = _check(lib, items, a[at:at + D], quality, lgwin)
        assert info[:5] == [len(items), len(items), 0, 0, 1] and info[5] == min(D, (1 << lgwin) - 16), (D, info)


@pytest.mark.parametrize("quality,lgwin", _EDGE_CASES)
def test_edges_emu(quality, lgwin):
    _edges(test_cabi._load("emu"), quality, lgwin)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin", _EDGE_CASES)
def test_edges_gpu(quality, lgwin):
    _edges(test_cabi._load("gpu"), quality, lgwin)


# ---- 5. table reuse: one and two tables, groups of ten items (settings are read once per process: a child); 24 items of 1 .. 2048
# bytes in mixed order, all stretches of the dictionary's own text: a stale bucket, or a forest slot left in reach behind a shorter
# item, would change bytes.  With every chain filing the dictionary itself (BROTLI_MI355X_BATCH_DICT_SELF_FILE=1) the same digest.

def _reuse_batch():
    a = synth.alice()
    dictionary = a[2000:2000 + 16384]
    items = [dictionary[500 * k:500 * k + 1 + (89 * k) % 2048] for k in range(24)]
    items[5] = dictionary[9000:9000 + 2048]
    return items, dictionary


_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_dictionary_zopfli as t, test_cabi
lib = test_cabi._load(%r)
items, dictionary = t._reuse_batch()
h = hashlib.sha256()
groups = []
for q in (10, 11):
    ret, outs, results, sizes, info = t._shared(lib, q, 22, t.ZS, dictionary, items)
    assert ret == 1 and info[:4] == [24, 24, 0, 0] and info[5:] == [16384, 0, 0], info
    for out in outs:
        h.update(len(out).to_bytes(8, "little") + out)
    groups.append(info[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which):
    items, dictionary = _reuse_batch()
    assert min(len(x) for x in items) == 1 and max(len(x) for x in items) == 2048
    h = hashlib.sha256()
    for q in (10, 11):
        for x in items:
            out = _oracle(x, q, 22, dictionary)
            h.update(len(out).to_bytes(8, "little") + out)
    want = "digest %s groups %s" % (h.hexdigest(), [3, 3])
    for tables, self_file in (("1", None), ("2", None), ("2", "1")):
        env = dict(os.environ)
        env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
        env.pop("BROTLI_MI355X_BATCH_DICT_SELF_FILE", None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "10"})
        if self_file is not None:
            env["BROTLI_MI355X_BATCH_DICT_SELF_FILE"] = self_file
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and want in r.stdout, (tables, self_file, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 6. capacity: the stream rule -- an item goes out if and only if its stream fits; there is no stored fallback

def _capacity(lib):
    a = synth.alice()
    dictionary = a[10000:30000]
    items = [a[:3000], synth.random_bytes(700), a[12000:13900], b"tail"]
    for quality in (10, 11):
        full = [_oracle(x, quality, 22, dictionary) for x in items]
        for k in range(4):
            c = [len(w) for w in full]
            c[k] -= 1
            ret, got, results, sizes, info = _shared(lib, quality, 22, ZS, dictionary, items, c)
            assert ret == 0 and results == [0 if i == k else 1 for i in range(4)] and sizes[k] == 0, (quality, k, ret, results, sizes)
            assert [g for i, g in enumerate(got) if i != k] == [w for i, w in enumerate(full) if i != k]
            assert info[:5] == [4, 4, 0, 0, 1]
        ret, got, _, _, info = _shared(lib, quality, 22, ZS, dictionary, items, [len(w) for w in full], with_results=False)
        assert ret == 1 and got == full and info[:5] == [4, 4, 0, 0, 1]


def test_capacity_emu():
    _capacity(test_cabi._load("emu"))


@pytest.mark.gpu
def test_capacity_gpu():
    _capacity(test_cabi._load("gpu"))


# ---- 7. threads: four threads, each with a routed call and a dictionary of its own

def _threads(lib):
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(24)] for t in range(4)]
    dictionaries = [synth.markov_text(700 * (t + 1), 30 + t) + a[5000 * t:5000 * t + 9000] for t in range(4)]
    want = [[_oracle(x, 10 + t % 2, 22, dictionaries[t]) for x in batches[t]] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        ret, outs, _, _, info = _shared(lib, 10 + t % 2, 22, ZS, dictionaries[t], batches[t])
        got[t], infos[t] = (ret, outs), info  # (BrotliMi355xLastBatchInfo is per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == [(1, w) for w in want]
    assert [i[:4] + i[5:] for i in infos] == [[24, 24, 0, 0, 700 * (t + 1) + 9000, 0, 0] for t in range(4)], infos


def test_threads_emu():
    _threads(test_cabi._load("emu"))


@pytest.mark.gpu
def test_threads_gpu():
    _threads(test_cabi._load("gpu"))


# ---- 8. the Python binding: compress_batch_with_dictionary(..., zopfli_items=True) sets the bit; compress_batch has no such pairing

def _python_binding(lib):
    a = synth.alice()
    dictionary, items = a[:6000], [a[6000:6700], b"", a[100:1300]]
    assert lib.BATCH_ROUTE_ZOPFLI_SHARED_DICTIONARY_ITEMS == ZS
    for quality in (10, 11):
        want = [_oracle(x, quality, 22, dictionary) for x in items]
        assert lib.compress_batch_with_dictionary(items, dictionary, quality=quality, zopfli_items=True) == want
        assert lib.last_batch_info()[:4] == [3, 2, 1, 0]
        assert lib.compress_batch_with_dictionary(items, dictionary, quality=quality, quick_items=True, q9_items=True) == want
        assert lib.last_batch_info()[:4] == [3, 0, 3, 0]
    with pytest.raises(ValueError):
        lib.compress_batch(items, quality=11, dictionary=dictionary, zopfli_items=True)


def test_python_binding_emu():
    _python_binding(test_cabi._load("emu"))


@pytest.mark.gpu
def test_python_binding_gpu():
    _python_binding(test_cabi._load("gpu"))
