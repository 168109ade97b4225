"""BrotliMi355xCompressBatchWithDictionaries / Library.compress_batch_with_dictionaries: the batch call with a custom dictionary per
item.

Item i is the stream of BrotliEncoderSetCustomDictionary(dictionaries[item_dictionaries[i]]) + one BrotliEncoderCompressStream(FINISH)
on the same bytes: the oracle's stream API with that dictionary.  At qualities 5 to 8, lgwin 17 to 24, the items of 1 to 65 536
bytes behind a dictionary of 2 to 65 536 bytes run side by side on the device, each chain filing its own dictionary into a table
of its own (batch_greedy.h); every other item goes one by one through the stream path in the same call.  last_batch_info() proves
which path was taken.  The CPU tests run the emulation library -- the same host plan and the same item code -- the GPU tests the
product library.  The oracle's streams are shared with test_batch_dictionary (one cache)."""
import ctypes
import functools
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
import test_cabi
from test_batch_dictionary import BLOCK, GOLDEN, HERE, _oracle


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _side_by_side(item, quality, lgwin, dictionary):
    return 5 <= quality <= 8 and 17 <= lgwin <= 24 and 2 <= len(dictionary) <= BLOCK and 1 <= len(item) <= BLOCK


def _expected_info(items, dictionaries, item_dicts, quality, lgwin):
    """info[0..3] and info[5..7]; info[4], the groups, is the caller's to check"""
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    side = sum(1 for x, k in zip(items, named) if _side_by_side(x, quality, lgwin, dictionaries[k]))
    return [len(items), side, len(items) - side, 0], [sum(_in_use(quality, lgwin, dictionaries[k]) for k in sorted(set(named))), 0, 0]


def _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode=0):
    got = lib.compress_batch_with_dictionaries(items, dictionaries, item_dicts, quality, lgwin, mode)
    info = lib.last_batch_info()
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    assert len(got) == len(items)
    for i, (g, item, k) in enumerate(zip(got, items, named)):
        assert g == _oracle(item, quality, lgwin, dictionaries[k], mode), (quality, lgwin, mode, i, len(item), k, len(dictionaries[k]))
    head, tail = _expected_info(items, dictionaries, item_dicts, quality, lgwin)
    assert info[:4] == head and info[5:] == tail, (info, head, tail)
    assert (info[4] >= 1) == (head[1] > 0), info
    return got


def _raw(lib, quality, lgwin, dictionaries, item_dicts, items, caps, routes=0, num_dicts=None, with_results=True):
    """BrotliMi355xCompressBatchWithDictionaries through ctypes: (return value, [bytes], [item result], [size])"""
    n, nd = len(items), len(dictionaries)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    dicts = (c_char_p * max(1, nd))(*dictionaries)
    dict_sizes = (c_size_t * max(1, nd))(*[0 if d is None else len(d) for d in dictionaries])
    named = ctypes.cast(None, POINTER(c_size_t)) if item_dicts is None else (c_size_t * max(1, n))(*item_dicts)
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, 0, routes, nd if num_dicts is None else num_dicts, dicts, dict_sizes, n, named,
                                                            inputs, in_sizes, outputs, out_sizes,
                                                            results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


def _caps(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]


# ---- 1. taken side by side (fails where the library has no BrotliMi355xCompressBatchWithDictionaries)

def _taken_side_by_side(lib):
    a, m = synth.alice(), synth.markov_text(40000, 3)
    items = [b"", b"x", a[30000:35000], a[30000:30000 + BLOCK], a[30000:30000 + BLOCK + 1], synth.random_bytes(3000)]
    dictionaries = [a[:20000], m[:300], a[28000:33000], a[20000:20000 + BLOCK], m[:9000], synth.random_bytes(5000)]
    got = lib.compress_batch_with_dictionaries(items, dictionaries, None, 5, 22)
    info = lib.last_batch_info()
    # the empty and the long item go one by one, through the stream path: none is "answered without an encoder"
    assert info[:4] == [6, 4, 2, 0] and info[4] >= 1 and info[5:] == [sum(len(d) for d in dictionaries), 0, 0], info
    assert got == [_oracle(x, 5, 22, d) for x, d in zip(items, dictionaries)]
    _check(lib, items, dictionaries, None, 8, 17)


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. each item uses its own dictionary: item i is a verbatim stretch of dictionary i, and the dictionaries are disjoint texts

def _own_dictionary_is_used(lib):
    dictionaries = [synth.alice()[:20000], synth.markov_text(20000, 17), synth.random_bytes(20000)]
    items = [d[5000:9000] for d in dictionaries]
    for quality in (5, 8):
        own = _check(lib, items, dictionaries, [0, 1, 2], quality, 22)
        rotated = _check(lib, items, dictionaries, [1, 2, 0], quality, 22)
        for i, (g, r) in enumerate(zip(own, rotated)):
            assert 2 * len(g) < len(r), (quality, i, len(g), len(r))


def test_own_dictionary_is_used_emu():
    _own_dictionary_is_used(test_cabi._load("emu"))


@pytest.mark.gpu
def test_own_dictionary_is_used_gpu():
    _own_dictionary_is_used(test_cabi._load("gpu"))


# ---- 3. identity set: the alignment edges of the layout kernel and of the 16-byte shift

_IDENTITY_CASES = [(q, w, 0) for q in (5, 6, 7, 8) for w in (22, 24, 17)] + [(5, 22, 1), (5, 22, 2), (5, 22, 6)]
_DICTIONARY_SIZES = (2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 20000, 65536)
_ITEM_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, BLOCK - 1, BLOCK)


@functools.lru_cache(maxsize=None)
def _dictionaries():
    """every size, by turns from the book and from generated text"""
    a, m = synth.alice(), synth.markov_text(70000, 21)
    return tuple((a[1000:1000 + n] if j % 2 == 0 else m[300:300 + n]) for j, n in enumerate(_DICTIONARY_SIZES))


@functools.lru_cache(maxsize=None)
def _identity_items():
    a = synth.alice()
    return tuple([a[7:7 + n] for n in _ITEM_SIZES] + [bytes(30000), synth.random_bytes(20000)])


def _identity_deal(quality, part):
    """The three calls of a quality (its windows; a mode takes the share of its place among the modes) share the dictionaries out:
    dictionary j goes to the call with (j + quality) % 3 == part.  Every call takes every item, item i behind the
    (i + quality) % len(share)-th dictionary of the share.  -> (indices into _dictionaries(), item_dicts)"""
    share = [j for j in range(len(_DICTIONARY_SIZES)) if (j + quality) % 3 == part]
    return share, [(i + quality) % len(share) for i in range(len(_identity_items()))]


def _identity(lib, quality, lgwin, mode):
    part = (22, 24, 17).index(lgwin) if mode == 0 else (1, 2, 6).index(mode)
    share, item_dicts = _identity_deal(quality, part)
    dictionaries = [_dictionaries()[j] for j in share]
    # ... and every dictionary of the share once in front of the longest item, and once as an item behind itself
    items = list(_identity_items()) + [_identity_items()[len(_ITEM_SIZES) - 1]] * len(share) + dictionaries
    item_dicts = item_dicts + list(range(len(share))) * 2
    _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode)


def test_identity_deal_covers_every_size_per_quality():
    for quality in (5, 6, 7, 8):
        seen = []
        for part in range(3):
            share, item_dicts = _identity_deal(quality, part)
            assert len(item_dicts) == len(_identity_items()) == len(_ITEM_SIZES) + 2  # (every item size in every call)
            assert sorted(set(item_dicts)) == list(range(len(share)))  # (every dictionary of the share is named)
            seen += share
        assert sorted(seen) == list(range(len(_DICTIONARY_SIZES))), (quality, seen)
    assert sorted(len(d) for d in _dictionaries()) == sorted(_DICTIONARY_SIZES)
    assert [len(x) for x in _identity_items()[:len(_ITEM_SIZES)]] == list(_ITEM_SIZES)


@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_emu(quality, lgwin, mode):
    _identity(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_gpu(quality, lgwin, mode):
    _identity(test_cabi._load("gpu"), quality, lgwin, mode)


# ---- 4. table and group reuse: three tables, groups of five items (settings are read once per process: a child), dictionaries
# that alternate between 65 536 and 2 bytes -- a short dictionary follows a long one on the same table, and every item is a stretch
# of the long dictionaries' text, so an entry the item in front left in reach would change bytes

def _reuse_batch():
    a = synth.alice()
    dictionaries = [a[k:k + (BLOCK if k % 2 == 0 else 2)] for k in range(24)]
    items = [a[3000 + 2000 * k:3000 + 2000 * k + 1500 + 37 * k] for k in range(24)]
    return items, dictionaries


_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_dictionaries, test_cabi
lib = test_cabi._load(%r)
items, dictionaries = test_batch_dictionaries._reuse_batch()
h = hashlib.sha256()
groups = []
for q in (5, 8):
    for out in lib.compress_batch_with_dictionaries(items, dictionaries, None, q, 22):
        h.update(len(out).to_bytes(8, "little") + out)
    info = lib.last_batch_info()
    assert info[:4] == [24, 24, 0, 0], info
    groups.append(info[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which):
    items, dictionaries = _reuse_batch()
    assert [len(d) for d in dictionaries] == [BLOCK, 2] * 12
    h = hashlib.sha256()
    for q in (5, 8):
        for x, d in zip(items, dictionaries):
            out = _oracle(x, q, 22, d)
            h.update(len(out).to_bytes(8, "little") + out)
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
    env.update({"BROTLI_MI355X_BATCH_TABLES": "3", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "5"})
    r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
    want = "digest %s groups %s" % (h.hexdigest(), [5, 5])
    assert r.returncode == 0 and want in r.stdout, (want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu")


# ---- 5. shared indices

def _shared_indices(lib):
    a = synth.alice()
    dictionaries = [a[:20000], synth.markov_text(9000, 4), a[60000:60000 + 777]]
    items = [a[500 * i:500 * i + 200 + 61 * i] for i in range(40)]
    item_dicts = [(i * 7 + i // 5) % 3 for i in range(40)]
    assert sorted(set(item_dicts)) == [0, 1, 2]
    got = _check(lib, items, dictionaries, item_dicts, 5, 22)
    assert lib.last_batch_info()[:6] == [40, 40, 0, 0, 1, 20000 + 9000 + 777]
    for k in range(3):
        mine = [i for i in range(40) if item_dicts[i] == k]
        shared = lib.compress_batch([items[i] for i in mine], 5, 22, dictionary=dictionaries[k])
        assert shared == [got[i] for i in mine], k
    # a single index named: the shared-dictionary call, in bytes and in info
    for quality in (5, 2):
        single = lib.compress_batch_with_dictionaries(items, dictionaries, [1] * 40, quality, 22)
        info = lib.last_batch_info()
        shared = lib.compress_batch(items, quality, 22, dictionary=dictionaries[1])
        assert single == shared and info == lib.last_batch_info(), (quality, info, lib.last_batch_info())
        assert info[:6] == ([40, 40, 0, 0, 1, 9000] if quality == 5 else [40, 0, 40, 0, 0, 9000])
    # item i takes dictionaries[i]
    _check(lib, items[:3], dictionaries, None, 7, 22)
    _check(lib, items[:1], dictionaries[:1], None, 7, 22)


def test_shared_indices_emu():
    _shared_indices(test_cabi._load("emu"))


@pytest.mark.gpu
def test_shared_indices_gpu():
    _shared_indices(test_cabi._load("gpu"))


# ---- 6. one by one, same bytes: dictionaries that are too short or too long, other windows and qualities, an item of three
# blocks, the empty item -- among items that go side by side

def _one_by_one(lib, long_item):
    a = synth.alice()
    m = synth.markov_text(70000, 5)
    dictionaries = [b"", m[:1], m, a[:20000]]
    items = [a[:3000], a[50000:50700], a[100:3000], long_item, b"", a[30000:31000], a[31000:31001]]
    item_dicts = [0, 1, 2, 3, 3, 3, 2]
    _check(lib, items, dictionaries, item_dicts, 5, 22)
    assert lib.last_batch_info()[:6] == [7, 1, 6, 0, 1, 90000]
    for quality, lgwin in ((5, 16), (0, 22), (2, 22), (9, 22)):
        _check(lib, [items[0], items[5], b""], [a[:20000], m[:5000], a[40000:40300]], None, quality, lgwin)
        assert lib.last_batch_info()[:6] == [3, 0, 3, 0, 0, 0 if quality == 0 else 25300]


def test_one_by_one_emu():
    _one_by_one(test_cabi._load("emu"), synth.markov_text(3 * BLOCK, 8))


@pytest.mark.gpu
def test_one_by_one_gpu():
    _one_by_one(test_cabi._load("gpu"), synth.markov_text(3 * BLOCK, 8))


# ---- 7. failures

def _failures(lib):
    a = synth.alice()
    x = open(os.path.join(GOLDEN, "copy_of_length_one.bin"), "rb").read()
    d, bad = x[:64], x[64:]
    items = [a[:3000], bad, a[100:2000], b"tail"]
    dictionaries = [a[10000:30000], d, synth.markov_text(4000, 6), a[:50]]
    caps = _caps(lib, items)
    want = [None if k == 1 else _oracle(items[k], 6, 20, dictionaries[k]) for k in range(4)]
    with pytest.raises(orc.ReferencePanics):
        _oracle(bad, 6, 20, d)
    # the item the reference fails on fails alone
    ret, got, results, sizes = _raw(lib, 6, 20, dictionaries, None, items, caps)
    assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0, (ret, results, sizes)
    assert "reference encoder fails" in lib.last_error()
    assert lib.last_batch_info() == [4, 4, 0, 0, 1, 20000 + 64 + 4000 + 50, 0, 0]
    assert [got[k] for k in (0, 2, 3)] == [want[k] for k in (0, 2, 3)]
    # ... also where it goes one by one
    with pytest.raises(orc.ReferencePanics):
        _oracle(bad, 9, 22, d)
    ret, got, results, sizes = _raw(lib, 9, 22, dictionaries, None, items, caps)
    assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0 and "reference encoder fails" in lib.last_error()
    assert [got[k] for k in (0, 2, 3)] == [_oracle(items[k], 9, 22, dictionaries[k]) for k in (0, 2, 3)]
    # a capacity too small fails its item alone; one of exactly the stream's size is enough; item_results may be NULL
    healthy, healthy_dicts = [items[0], items[2], items[3]], [0, 2, 3]
    hw = [want[0], want[2], want[3]]
    for k, cap in ((0, len(hw[0]) - 1), (2, 0), (1, 5)):
        c = [len(w) for w in hw]
        c[k] = cap
        ret, got, results, sizes = _raw(lib, 6, 20, dictionaries, healthy_dicts, healthy, c)
        assert ret == 0 and results == [0 if i == k else 1 for i in range(3)] and sizes[k] == 0, (k, cap, ret, results, sizes)
        assert [g for i, g in enumerate(got) if i != k] == [w for i, w in enumerate(hw) if i != k]
    ret, got, results, sizes = _raw(lib, 6, 20, dictionaries, healthy_dicts, healthy, [len(w) for w in hw], with_results=False)
    assert ret == 1 and got == hw
    assert lib.last_batch_info() == [3, 3, 0, 0, 1, 20000 + 4000 + 50, 0, 0]  # (the dictionary no item names does not count)
    # what fails the whole call before any work is done: only info[0] is set
    hc = _caps(lib, healthy)
    for kwargs, named, message in ((dict(), [0, 4, 3], "names dictionary 4 of 4"), (dict(), None, "num_dicts"), (dict(routes=4), healthy_dicts, "routes 4"),
                                   (dict(routes=256), healthy_dicts, "routes 256"), (dict(num_dicts=3), healthy_dicts, "names dictionary 3 of 3")):
        ret, got, results, sizes = _raw(lib, 6, 20, dictionaries, named, healthy, hc, **kwargs)
        assert ret == 0 and results == [0, 0, 0] and sizes == [0, 0, 0], (kwargs, named, ret, results, sizes)
        assert message in lib.last_error(), (message, lib.last_error())
        assert lib.last_batch_info() == [3, 0, 0, 0, 0, 0, 0, 0]
    # count == 0 (with NULL indices, num_dicts == count == 0; and with dictionaries nobody names); a NULL dictionary of size 0
    assert _raw(lib, 6, 20, [], None, [], [])[0] == 1
    assert _raw(lib, 6, 20, dictionaries, [], [], [])[0] == 1
    assert lib.last_batch_info() == [0] * 8
    ret, got, results, _ = _raw(lib, 6, 20, [None, dictionaries[2]], [0, 1], healthy[:2], hc[:2])
    assert ret == 1 and results == [1, 1] and got == [_oracle(healthy[0], 6, 20, b""), _oracle(healthy[1], 6, 20, dictionaries[2])]
    assert lib.last_batch_info() == [2, 1, 1, 0, 1, 4000, 0, 0]
    # the Python method raises like its neighbours and carries what the call left
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    with pytest.raises(exc) as e:
        lib.compress_batch_with_dictionaries(items, dictionaries, None, 6, 20)
    assert e.value.failed == [1] and [e.value.streams[k] for k in (0, 2, 3)] == [want[k] for k in (0, 2, 3)] and e.value.streams[1] is None
    with pytest.raises(exc):
        lib.compress_batch_with_dictionaries(items, dictionaries[:3], None, 6, 20)


def test_failures_emu():
    _failures(test_cabi._load("emu"))


@pytest.mark.gpu
def test_failures_gpu():
    _failures(test_cabi._load("gpu"))


# ---- 8. permutation: the streams depend neither on the order of the items nor on that of the dictionaries

def _permutation(lib):
    a = synth.alice()
    dictionaries = [a[:20000], synth.markov_text(BLOCK, 12), a[70000:70009], synth.random_bytes(3000), a[40000:40000 + 6000]]
    items = list(_identity_items()) + [synth.markov_text(n, n) for n in (200, 900, 5000, 60000)] + [b"", a[:BLOCK + 1]]
    item_dicts = [(3 * i + i // 4) % 5 for i in range(len(items))]
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    dict_order = [3, 0, 4, 2, 1]  # the new place k holds the old dictionary dict_order[k]
    new_index = {old: new for new, old in enumerate(dict_order)}
    for quality in (5, 7):
        straight = _check(lib, items, dictionaries, item_dicts, quality, 22)
        assert lib.last_batch_info()[1] == len(items) - 2  # (all but the empty and the long item)
        shuffled = lib.compress_batch_with_dictionaries([items[i] for i in order], [dictionaries[k] for k in dict_order],
                                                        [new_index[item_dicts[i]] for i in order], quality, 22)
        assert lib.last_batch_info()[1] == len(items) - 2
        assert shuffled == [straight[i] for i in order]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# ---- 9. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

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
    dictionaries = [a[100000:120000], synth.markov_text(3000, 2), a[:17]]
    items = [a[:20000], b"tiny", synth.markov_text(60000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch_with_dictionaries(items, dictionaries, [0, 1, 2, 1], 5, 22))
        assert lib.last_batch_info()[:6] == [4, 4, 0, 0, 1, 23017]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 10. threads: four threads, each with dictionaries and a batch of its own

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(48)] for t in range(4)]
    dictionaries = [[synth.markov_text(700 * (t + 1), 30 + t), a[5000 * t:5000 * t + 9000], a[1000 * t:1000 * t + 40]] for t in range(4)]
    named = [[(i + t) % 3 for i in range(48)] for t in range(4)]
    want = [[_oracle(x, 5, 22, dictionaries[t][k]) for x, k in zip(batches[t], named[t])] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch_with_dictionaries(batches[t], dictionaries[t], named[t], 5, 22)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert [i[:4] + i[5:] for i in infos] == [[48, 48, 0, 0, 700 * (t + 1) + 9040, 0, 0] for t in range(4)], infos
