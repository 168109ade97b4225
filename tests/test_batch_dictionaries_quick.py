"""BrotliMi355xCompressBatchWithDictionaries with BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS /
Library.compress_batch_with_dictionaries(..., quick_items=True): the batch call with a custom dictionary per item, at qualities 2 to 4.

Item i is the stream of BrotliEncoderSetCustomDictionary(dictionaries[item_dictionaries[i]]) + one BrotliEncoderCompressStream(FINISH)
on the same bytes: the oracle's stream API with that dictionary.  With the route set, at qualities 2 to 4, lgwin 10 to 24, an item of
at most one input block (16 384 bytes at quality 2 and 3, 65 536 at quality 4) behind a dictionary of at least 2 bytes of which at
most 65 536 are in use runs side by side on the device: its chain zeroes a table of its own and files the item's dictionary into it,
64 positions per step with an atomic maximum (batch_quick.h).  Every other item goes one by one through the stream path in the same
call.  No item is skipped or tolerated: every stream equals the oracle's.  last_batch_info() proves which path was taken, so a
silent fall-back fails a test.  The CPU tests run the emulation library -- the same host plan and the same item code -- the GPU
tests the product library.  The oracle's streams are shared with test_batch_dictionary_quick (one cache)."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import threading
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_void_p

import pytest

import orc
import synth
import test_batch_dictionary_quick
import test_cabi
from test_batch_dictionary_quick import _EDGE_CASES, _FAILS_DICTIONARY, _FAILS_ITEM, _block, _edge_items, _edge_share, _oracle

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 512  # BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _side_by_side(item, quality, lgwin, dictionary):
    return (2 <= quality <= 4 and 10 <= lgwin <= 24 and len(dictionary) >= 2 and _in_use(quality, lgwin, dictionary) <= 65536
            and 1 <= len(item) <= _block(quality))


def _expected_info(items, dictionaries, item_dicts, quality, lgwin):
    """info[0..3] and info[5..7]; info[4], the groups, is the caller's to check"""
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    side = sum(1 for x, k in zip(items, named) if _side_by_side(x, quality, lgwin, dictionaries[k]))
    return [len(items), side, len(items) - side, 0], [sum(_in_use(quality, lgwin, dictionaries[k]) for k in sorted(set(named))), 0, 0]


def _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode=0):
    got = lib.compress_batch_with_dictionaries(items, dictionaries, item_dicts, quality, lgwin, mode, quick_items=True)
    info = lib.last_batch_info()
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    assert len(got) == len(items)
    for i, (g, item, k) in enumerate(zip(got, items, named)):
        assert g == _oracle(item, quality, lgwin, dictionaries[k], mode), (quality, lgwin, mode, i, len(item), k, len(dictionaries[k]))
    head, tail = _expected_info(items, dictionaries, item_dicts, quality, lgwin)
    assert info[:4] == head and info[5:] == tail, (info, head, tail)
    assert (info[4] >= 1) == (head[1] > 0), info
    return got


def _raw(lib, quality, lgwin, routes, dictionaries, item_dicts, items, caps, with_results=True):
    """BrotliMi355xCompressBatchWithDictionaries through ctypes: (return value, [bytes], [item result], [size])"""
    n, nd = len(items), len(dictionaries)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    dicts = (c_char_p * max(1, nd))(*dictionaries)
    dict_sizes = (c_size_t * max(1, nd))(*[len(d) for d in dictionaries])
    named = ctypes.cast(None, POINTER(c_size_t)) if item_dicts is None else (c_size_t * max(1, n))(*item_dicts)
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, 0, routes, nd, dicts, dict_sizes, n, named, inputs, in_sizes, outputs, out_sizes,
                                                            results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


def _caps(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]


# ---- 1. taken side by side (fails where routes 512 is an unknown route of the call)

def _taken_side_by_side(lib):
    a, m = synth.alice(), synth.markov_text(40000, 3)
    dictionaries = [a[:20000], m[:300], a[28000:33000], a[20000:20000 + 65536], m[:9000], synth.random_bytes(5000)]
    assert sum(len(d) for d in dictionaries) == 104836

    def batch(block):
        return [b"", b"x", a[30000:35000], a[30000:30000 + block], a[30000:30000 + block + 1], synth.random_bytes(3000)]

    for quality in (2, 3, 4):
        items = batch(_block(quality))
        caps = _caps(lib, items)
        for lgwin in (22, 17):
            want = [_oracle(x, quality, lgwin, d) for x, d in zip(items, dictionaries)]
            ret, outs, results, _ = _raw(lib, quality, lgwin, Q, dictionaries, None, items, caps)
            info = lib.last_batch_info()
            assert ret == 1 and results == [1] * 6, (quality, lgwin, lib.last_error())
            # the empty item and the one of a block + 1 go one by one, through the stream path: none is "answered without an encoder"
            assert info[:4] == [6, 4, 2, 0] and info[4] >= 1 and info[5:] == [104836, 0, 0], (quality, lgwin, info)
            assert outs == want, (quality, lgwin)
            assert lib.compress_batch_with_dictionaries(items, dictionaries, None, quality, lgwin, quick_items=True) == want
            assert lib.last_batch_info() == info
            # routes == 0 and the Python call without the keyword: the same bytes, nothing side by side
            ret, outs, results, _ = _raw(lib, quality, lgwin, 0, dictionaries, None, items, caps)
            assert ret == 1 and outs == want, (quality, lgwin)
            assert lib.last_batch_info() == [6, 0, 6, 0, 0, 104836, 0, 0], (quality, lgwin)
            assert lib.compress_batch_with_dictionaries(items, dictionaries, None, quality, lgwin) == want
            assert lib.last_batch_info() == [6, 0, 6, 0, 0, 104836, 0, 0]
    # the bit changes nothing at quality 5: the items take the greedy route of the plain call, with the same info
    items = batch(65536)
    caps = _caps(lib, items)
    want = [_oracle(x, 5, 22, d) for x, d in zip(items, dictionaries)]
    ret, outs, _, _ = _raw(lib, 5, 22, 0, dictionaries, None, items, caps)
    plain = lib.last_batch_info()
    assert ret == 1 and outs == want and plain[:4] == [6, 4, 2, 0] and plain[5:] == [104836, 0, 0]
    ret, outs, _, _ = _raw(lib, 5, 22, Q, dictionaries, None, items, caps)
    assert ret == 1 and outs == want and lib.last_batch_info() == plain
    # ... and nothing at qualities 1 and 9
    for quality in (1, 9):
        ret, outs, _, _ = _raw(lib, quality, 22, Q, dictionaries[:3], None, items[:3], caps[:3])
        assert ret == 1 and outs == [_oracle(x, quality, 22, d) for x, d in zip(items[:3], dictionaries[:3])]
        assert lib.last_batch_info() == [3, 0, 3, 0, 0, sum(_in_use(quality, 22, d) for d in dictionaries[:3]), 0, 0], quality
    # a route this call does not know fails the whole call, and only info[0] is set: the bits of the other batch calls included,
    # also beside the one it knows
    for routes in (4, 256, Q | 4, 1 << 31):
        ret, outs, results, sizes = _raw(lib, 2, 22, routes, dictionaries, None, items, caps)
        assert ret == 0 and results == [0] * 6 and sizes == [0] * 6, routes
        assert lib.last_batch_info() == [6, 0, 0, 0, 0, 0, 0, 0], routes
        assert "routes %d" % routes in lib.last_error()
    # ... and 512 is an unknown route of the other batch calls
    ret, outs, results, sizes = test_batch_dictionary_quick._raw(lib, 2, 22, Q, dictionaries[0], items, caps)
    assert ret == 0 and results == [0] * 6 and sizes == [0] * 6 and "route" in lib.last_error()
    assert lib.last_batch_info() == [6, 0, 0, 0, 0, 0, 0, 0]
    n = len(items)
    bufs = [ctypes.create_string_buffer(c) for c in caps]
    out_sizes = (c_size_t * n)(*caps)
    results = (c_int32 * n)(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchEx(2, 22, 0, Q, n, (c_char_p * n)(*items), (c_size_t * n)(*[len(x) for x in items]),
                                              (c_void_p * n)(*[ctypes.addressof(b) for b in bufs]), out_sizes, results)
    assert ret == 0 and list(results) == [0] * 6 and list(out_sizes) == [0] * 6 and "route" in lib.last_error()
    assert lib.last_batch_info() == [6, 0, 0, 0, 0, 0, 0, 0]


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. each item uses its own dictionary: item i is a verbatim stretch of dictionary i, and the dictionaries are disjoint texts

def _own_dictionary_is_used(lib):
    dictionaries = [synth.alice()[:20000], synth.markov_text(20000, 17), synth.random_bytes(20000)]
    items = [d[5000:9000] for d in dictionaries]
    for quality in (2, 3, 4):
        own = _check(lib, items, dictionaries, [0, 1, 2], quality, 22)
        rotated = _check(lib, items, dictionaries, [1, 2, 0], quality, 22)
        for i, (g, r) in enumerate(zip(own, rotated)):
            assert 2 * len(g) < len(r), (quality, i, len(g), len(r))


def test_own_dictionary_is_used_emu():
    _own_dictionary_is_used(test_cabi._load("emu"))


@pytest.mark.gpu
def test_own_dictionary_is_used_gpu():
    _own_dictionary_is_used(test_cabi._load("gpu"))


# ---- 3. edge sizes: the inputs of test_batch_dictionary_quick's edge test, the dictionaries of a case's share side by side in one
# call -- D < 8 files nothing, D = 8 files one position, D % 64 != 0 leaves a partial last step, D % 8 != 0 shifts the sweep offset,
# D % 16 != 0 moves the pool alignment, and a long dictionary follows a 2-byte one on the same table

def _edges(lib, quality, lgwin, mode):
    a = synth.alice()
    at = 1200 + 131 * quality
    dictionaries, items, item_dicts = [], [], []
    for k, n in enumerate(_edge_share(quality, lgwin, mode)):
        dictionaries.append(a[at:at + n])
        mine = _edge_items(quality, at, n)
        items += mine
        item_dicts += [k] * len(mine)
    assert 2 <= len(dictionaries) <= 5  # (more than one index: the call does not forward to the shared-dictionary one)
    _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode)


@pytest.mark.parametrize("quality,lgwin,mode", _EDGE_CASES)
def test_edge_sizes_emu(quality, lgwin, mode):
    _edges(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _EDGE_CASES)
def test_edge_sizes_gpu(quality, lgwin, mode):
    _edges(test_cabi._load("gpu"), quality, lgwin, mode)


# ---- 4. slot collisions inside one filing step: every lane of a step hits the same one to four slots, and the stream changes if
# anything but the largest position wins

def _collision_pairs():
    a = synth.alice()
    return [(bytes(65536), bytes(3000)), (bytes(65536), bytes(9)), ((b"abc" * 30000)[:60001], b"abc" * 1000 + a[:500]),
            (bytes(range(256)) * 64, bytes(range(256)) * 8 + a[100:400]), (b"ab" * 100, b"ab" * 50 + b"xyz"), (bytes(64), bytes(64)),
            (bytes(71), a[:100] + bytes(40)), (bytes(1008), bytes(500))]


def _slot_collisions(lib):
    pairs = _collision_pairs()
    for quality in (2, 3, 4):
        for lgwin, mine in ((22, pairs), (10, pairs[4:])):
            _check(lib, [x for _, x in mine], [d for d, _ in mine], None, quality, lgwin)
            assert lib.last_batch_info()[1] == len(mine)


def test_slot_collisions_emu():
    _slot_collisions(test_cabi._load("emu"))


@pytest.mark.gpu
def test_slot_collisions_gpu():
    _slot_collisions(test_cabi._load("gpu"))


# ---- 5. small window and limits

def _small_window(lib):
    a = synth.alice()
    d = a[2000:7000]
    # lgwin 10: the reference cuts a 5000-byte dictionary to its last 1008 bytes, and the chain gets those
    dictionaries = [d, d[-1008:], a[6500:7000]]
    for quality in (2, 3, 4):
        items = [a[6000:6000 + k] for k in (1, 9, 500, 1008, 16384)] + [a[7000:9000], d]
        _check(lib, items, dictionaries, [i % 3 for i in range(len(items))], quality, 10)
        assert lib.last_batch_info()[1] == len(items) and lib.last_batch_info()[5] == 1008 + 1008 + 500
    # a dictionary of 0 or 1 bytes: no dictionary is taken, its item goes one by one
    _check(lib, [a[:3000], a[50000:50700], a[100:2000]], [b"", b"Z", a[:20000]], None, 2, 22)
    assert lib.last_batch_info() == [3, 1, 2, 0, 1, 20000, 0, 0]
    # more than 65 536 dictionary bytes in use: one by one, beside an item that goes side by side
    m = synth.markov_text(70000, 5)
    _check(lib, [a[:3000], a[50000:50700]], [m, a[:20000]], None, 2, 22)
    assert lib.last_batch_info() == [2, 1, 1, 0, 1, 90000, 0, 0]
    # ... unless the window cuts it down to that: lgwin 16 keeps 65 520 of each
    _check(lib, [a[:3000], a[50000:50700], m[69000:]], [m, m[1000:], m], [0, 1, 2], 3, 16)
    assert lib.last_batch_info()[1] == 3 and lib.last_batch_info()[5] == 3 * 65520


def test_small_window_emu():
    _small_window(test_cabi._load("emu"))


@pytest.mark.gpu
def test_small_window_gpu():
    _small_window(test_cabi._load("gpu"))


# ---- 6. the input the reference fails on, among three healthy items with dictionaries of their own

def _reference_fails(lib):
    a = synth.alice()
    d, bad = _FAILS_DICTIONARY, _FAILS_ITEM
    items = [a[:3000], bad, a[100:2000], b"tail"]
    dictionaries = [a[10000:30000], d, synth.markov_text(4000, 6), a[:50]]
    caps = _caps(lib, items)
    for quality in (2, 3, 4):
        for lgwin in (10, 17, 22):
            with pytest.raises(orc.ReferencePanics):
                _oracle(bad, quality, lgwin, d)
            ret, got, results, sizes = _raw(lib, quality, lgwin, Q, dictionaries, None, items, caps)
            assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0, (quality, lgwin, ret, results, sizes)
            assert "reference encoder fails" in lib.last_error()
            assert lib.last_batch_info()[1] == 4 and lib.last_batch_info()[2] == 0
            for k in (0, 2, 3):
                assert got[k] == _oracle(items[k], quality, lgwin, dictionaries[k]), (quality, lgwin, k)
    # the Python method raises, and the exception carries the streams of the items that did not fail
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    with pytest.raises(exc) as e:
        lib.compress_batch_with_dictionaries(items, dictionaries, None, 2, 22, quick_items=True)
    assert e.value.failed == [1] and "reference encoder fails" in str(e.value)
    want = [_oracle(items[k], 2, 22, dictionaries[k]) for k in (0, 2, 3)]
    assert e.value.streams == [want[0], None, want[1], want[2]]
    # with the dictionary's last byte changed the item goes through, side by side
    healed = [dictionaries[0], d[:-1] + b"d", dictionaries[2], dictionaries[3]]
    _check(lib, items, healed, None, 2, 22)
    assert lib.last_batch_info()[1] == 4
    # a capacity one byte short fails its item alone; one of exactly the stream's size is enough; item_results may be NULL
    full = [_oracle(x, 2, 22, k) for x, k in zip(items, healed)]
    for k in range(4):
        c = [len(w) for w in full]
        c[k] -= 1
        ret, got, results, sizes = _raw(lib, 2, 22, Q, healed, None, items, c)
        assert ret == 0 and results == [0 if i == k else 1 for i in range(4)] and sizes[k] == 0, (k, ret, results, sizes)
        assert [g for i, g in enumerate(got) if i != k] == [w for i, w in enumerate(full) if i != k]
        assert lib.last_batch_info()[:5] == [4, 4, 0, 0, 1]
    ret, got, _, _ = _raw(lib, 2, 22, Q, healed, None, items, [len(w) for w in full], with_results=False)
    assert ret == 1 and got == full


def test_reference_fails_emu():
    _reference_fails(test_cabi._load("emu"))


@pytest.mark.gpu
def test_reference_fails_gpu():
    _reference_fails(test_cabi._load("gpu"))


# ---- 7. table and group reuse: three tables, groups of five items (settings are read once per process: a child), dictionaries
# that alternate between 65 536 and 2 bytes -- a short dictionary follows a long one on the same table, and every item is a stretch
# of the long dictionaries' text, so a slot the item in front left in reach would change bytes

def _reuse_batch():
    a = synth.alice()
    dictionaries = [a[k:k + (65536 if k % 2 == 0 else 2)] for k in range(24)]
    items = [a[3000 + 2000 * k:3000 + 2000 * k + 1500 + 37 * k] for k in range(24)]
    return items, dictionaries


_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_dictionaries_quick, test_cabi
lib = test_cabi._load(%r)
items, dictionaries = test_batch_dictionaries_quick._reuse_batch()
h = hashlib.sha256()
groups = []
for q in (2, 3, 4):
    for out in lib.compress_batch_with_dictionaries(items, dictionaries, None, q, 22, quick_items=True):
        h.update(len(out).to_bytes(8, "little") + out)
    info = lib.last_batch_info()
    assert info[:4] == [24, 24, 0, 0], info
    groups.append(info[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which):
    items, dictionaries = _reuse_batch()
    assert [len(d) for d in dictionaries] == [65536, 2] * 12
    h = hashlib.sha256()
    for q in (2, 3, 4):
        for x, d in zip(items, dictionaries):
            out = _oracle(x, q, 22, d)
            h.update(len(out).to_bytes(8, "little") + out)
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
    env.update({"BROTLI_MI355X_BATCH_TABLES": "3", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "5"})
    r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
    want = "digest %s groups %s" % (h.hexdigest(), [5, 5, 5])
    assert r.returncode == 0 and want in r.stdout, (want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu")


# ---- 8. shared indices

def _shared_indices(lib):
    a = synth.alice()
    dictionaries = [a[:20000], synth.markov_text(9000, 4), a[60000:60777]]
    items = [a[500 * i:500 * i + 200 + 61 * i] for i in range(40)]
    item_dicts = [(i * 7 + i // 5) % 3 for i in range(40)]
    assert sorted(set(item_dicts)) == [0, 1, 2]
    for quality in (2, 3, 4):
        got = _check(lib, items, dictionaries, item_dicts, quality, 22)
        assert lib.last_batch_info() == [40, 40, 0, 0, 1, 20000 + 9000 + 777, 0, 0]
        # self-filed and behind the shared image: the same bytes
        for k in range(3):
            mine = [i for i in range(40) if item_dicts[i] == k]
            shared = lib.compress_batch_with_dictionary([items[i] for i in mine], dictionaries[k], quality, 22, quick_items=True)
            assert shared == [got[i] for i in mine], (quality, k)
        # a single index named: the shared-dictionary call with its quick route, in bytes and in info
        single = lib.compress_batch_with_dictionaries(items, dictionaries, [1] * 40, quality, 22, quick_items=True)
        info = lib.last_batch_info()
        shared = lib.compress_batch_with_dictionary(items, dictionaries[1], quality, 22, quick_items=True)
        assert single == shared and info == lib.last_batch_info() == [40, 40, 0, 0, 1, 9000, 0, 0], (quality, info, lib.last_batch_info())
        assert single == [_oracle(x, quality, 22, dictionaries[1]) for x in items]


def test_shared_indices_emu():
    _shared_indices(test_cabi._load("emu"))


@pytest.mark.gpu
def test_shared_indices_gpu():
    _shared_indices(test_cabi._load("gpu"))


# ---- 9. permutation: the streams depend neither on the order of the items nor on that of the dictionaries

def _permutation(lib):
    a = synth.alice()
    dictionaries = [a[:20000], synth.markov_text(65536, 12), a[70000:70009], synth.random_bytes(3000), a[40000:46000]]
    dict_order = [3, 0, 4, 2, 1]  # the new place k holds the old dictionary dict_order[k]
    new_index = {old: new for new, old in enumerate(dict_order)}
    for quality in (2, 4):
        block = _block(quality)
        items = [a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, block - 1, block)] + [bytes(10000), synth.random_bytes(9000)]
        items += [synth.markov_text(n, n) for n in (200, 900, 5000, block - 7)] + [b"", a[:block + 1]]
        item_dicts = [(3 * i + i // 4) % 5 for i in range(len(items))]
        order = list(range(len(items)))
        random.Random(5).shuffle(order)
        straight = _check(lib, items, dictionaries, item_dicts, quality, 22)
        assert lib.last_batch_info()[1] == len(items) - 2  # (all but the empty and the long item)
        shuffled = lib.compress_batch_with_dictionaries([items[i] for i in order], [dictionaries[k] for k in dict_order],
                                                        [new_index[item_dicts[i]] for i in order], quality, 22, quick_items=True)
        assert lib.last_batch_info()[1] == len(items) - 2
        assert shuffled == [straight[i] for i in order]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# ---- 10. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

def test_failed_call_frees_its_blocks_emu():
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    a = synth.alice()
    block = _block(2)
    dictionaries = [a[100000:120000], synth.markov_text(3000, 2), a[:17]]
    items = [a[:block - 384], b"tiny", synth.markov_text(12000 if block == 16384 else block - 5000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch_with_dictionaries(items, dictionaries, [0, 1, 2, 1], 2, 22, quick_items=True))
        assert lib.last_batch_info() == [4, 4, 0, 0, 1, 23017, 0, 0]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 11. threads: four threads, each with dictionaries, a batch and a quality of its own

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(48)] for t in range(4)]
    dictionaries = [[synth.markov_text(700 * (t + 1), 30 + t), a[5000 * t:5000 * t + 9000], a[1000 * t:1000 * t + 40]] for t in range(4)]
    named = [[(i + t) % 3 for i in range(48)] for t in range(4)]
    want = [[_oracle(x, 2 + t % 3, 22, dictionaries[t][k]) for x, k in zip(batches[t], named[t])] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch_with_dictionaries(batches[t], dictionaries[t], named[t], 2 + t % 3, 22, quick_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert [i[:4] + i[5:] for i in infos] == [[48, 48, 0, 0, 700 * (t + 1) + 9040, 0, 0] for t in range(4)], infos
