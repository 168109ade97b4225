"""The dictionary batch calls with BROTLI_MI355X_BATCH_ROUTE_Q9_DICTIONARY_ITEMS (4096): quality 9 behind a custom dictionary, shared
(BrotliMi355xCompressBatchWithDictionaryEx) and per item (BrotliMi355xCompressBatchWithDictionaries / ...Device), side by side.

Item i is the stream of BrotliEncoderSetCustomDictionary(dicts[item_dicts[i]]) + one BrotliEncoderCompressStream(FINISH) on the same
bytes: the oracle's stream API with that dictionary.  With the route set, at quality 9 and lgwin 17 to 24, an item of 1 to 65 536
bytes behind a dictionary of at least 2 bytes of which at most 65 536 are in use runs side by side on the device: one live H9 chain
that starts at position D of dictionary | item on a private H9 table -- behind a dictionary per item the chain files the
dictionary itself, behind one shared dictionary it replays the image made once per call (batch_q9.h, batch_q9_device.h).  Every
other item goes one by one through the stream path in the same call.  No item is skipped or tolerated: every stream equals the
oracle's, and an oracle failure on one of these inputs is a test error (but for the one input that is there to fail).
BrotliMi355xLastBatchInfo proves which path was taken, so a silent fall-back fails a test.  The calls are bound through ctypes
here.  The CPU tests run the emulation library -- the same host plan and the same item code -- the GPU tests the product library;
there no side-by-side item exceeds 8 KiB (a chain lasts about 1 us per byte) but for the runs of one byte that wrap a counter."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import threading
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_uint32, c_void_p

import pytest

import orc
import synth
import test_batch_device
import test_cabi
from test_batch_dictionaries_zopfli import _caps, _info, _raw
from test_batch_dictionary import _oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUICK, Z, Q9 = 512, 1024, 4096  # BROTLI_MI355X_BATCH_ROUTE_{QUICK,ZOPFLI,Q9}_DICTIONARY_ITEMS
GUARD = 64
FILL = 0xAA


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _side_by_side(item, quality, lgwin, dictionary):
    return (quality == 9 and 17 <= lgwin <= 24 and 2 <= _in_use(quality, lgwin, dictionary) <= 65536 and 1 <= len(item) <= 65536)


def _raw_shared(lib, quality, lgwin, routes, dictionary, items, caps=None, with_results=True, mode=0):
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


def _expected_info(items, dictionaries, item_dicts, quality, lgwin):
    """info[0..3] and info[5..7]; info[4], the groups, is the caller's to check"""
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    side = sum(1 for x, k in zip(items, named) if _side_by_side(x, quality, lgwin, dictionaries[k]))
    return [len(items), side, len(items) - side, 0], [sum(_in_use(quality, lgwin, dictionaries[k]) for k in sorted(set(named))), 0, 0]


def _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode=0, routes=Q9):
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    want = [_oracle(x, quality, lgwin, dictionaries[k], mode) for x, k in zip(items, named)]
    ret, got, results, sizes, info = _raw(lib, quality, lgwin, routes, dictionaries, item_dicts, items, mode=mode)
    assert ret == 1 and results == [1] * len(items), (quality, lgwin, mode, results, lib.last_error())
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (quality, lgwin, mode, i, len(items[i]), named[i], len(dictionaries[named[i]]), len(g), len(w))
    head, tail = _expected_info(items, dictionaries, item_dicts, quality, lgwin)
    assert info[:4] == head and info[5:] == tail, (info, head, tail)
    assert (info[4] >= 1) == (head[1] > 0), info
    return got


# ---- 1. taken side by side (fails where 4096 is an unknown route of the call)

def _taken_side_by_side(lib, gpu):
    a, m = synth.alice(), synth.markov_text(40000, 3)
    dictionaries = [m[:300], a[28000:33000], a[:16384], a[20000:20000 + 65536], synth.random_bytes(5000)]
    items = [b"", b"x", a[30000:35000], a[30000:30000 + 8192], synth.random_bytes(3000)]
    if not gpu:
        items += [a[1000:1000 + 65536], a[1000:1000 + 65537]]
    named = [i % 5 for i in range(len(items))]
    n = len(items)
    side = n - 1 - (0 if gpu else 1)  # all but the empty item and the one of 65 537 bytes
    caps = _caps(lib, items)
    for lgwin in (22, 17):
        in_use = sum(_in_use(9, lgwin, dictionaries[k]) for k in sorted(set(named)))
        got = _check(lib, items, dictionaries, named, 9, lgwin)
        info = _info(lib)
        assert info[:4] == [n, side, n - side, 0] and info[4] >= 1 and info[5] == in_use and info[6:] == [0, 0], (lgwin, info)
        # routes == 0: the same bytes, nothing side by side
        ret, outs, _, _, info = _raw(lib, 9, lgwin, 0, dictionaries, named, items, caps)
        assert ret == 1 and outs == got, lgwin
        assert info == [n, 0, n, 0, 0, in_use, 0, 0], (lgwin, info)
    small, small_named = items[:5], named[:5]
    small_caps = caps[:5]
    # the bit changes nothing at qualities 5, 2 and 11: the same bytes and the same info as without it
    for quality in (5, 2, 11):
        want = [_oracle(x, quality, 22, dictionaries[k]) for x, k in zip(small, small_named)]
        ret, outs, _, _, plain = _raw(lib, quality, 22, 0, dictionaries, small_named, small, small_caps)
        assert ret == 1 and outs == want and plain[:4] == ([5, 4, 1, 0] if quality == 5 else [5, 0, 5, 0]), (quality, plain)
        ret, outs, _, _, info = _raw(lib, quality, 22, Q9, dictionaries, small_named, small, small_caps)
        assert ret == 1 and outs == want and info == plain, (quality, info, plain)
    # lgwin 16 (hasher 42 in the reference) goes one by one
    ret, outs, _, _, info = _raw(lib, 9, 16, Q9, dictionaries, small_named, small, small_caps)
    assert ret == 1 and outs == [_oracle(x, 9, 16, dictionaries[k]) for x, k in zip(small, small_named)]
    assert info == [5, 0, 5, 0, 0, sum(_in_use(9, 16, dictionaries[k]) for k in small_named), 0, 0], info
    # 4096 | 512 | 1024 behaves as 4096 at quality 9
    ret, outs, results, _, info = _raw(lib, 9, 22, Q9, dictionaries, small_named, small, small_caps)
    assert ret == 1 and info[1] == 4, info
    ret2, outs2, results2, _, info2 = _raw(lib, 9, 22, Q9 | QUICK | Z, dictionaries, small_named, small, small_caps)
    assert (ret2, outs2, results2, info2) == (ret, outs, results, info)
    assert outs == [_oracle(x, 9, 22, dictionaries[k]) for x, k in zip(small, small_named)]
    # a route this call does not know fails the whole call, and only info[0] is set: also beside the one it knows
    for routes in (2048, Q9 | 4, 1 << 31):
        ret, outs, results, sizes, info = _raw(lib, 9, 22, routes, dictionaries, small_named, small, small_caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert info == [5, 0, 0, 0, 0, 0, 0, 0], routes
        assert "routes %d" % routes in lib.last_error()
    # ... and 4096 is an unknown route of the plain batch call
    bufs = [ctypes.create_string_buffer(c) for c in small_caps]
    inputs, in_sizes = (c_char_p * 5)(*small), (c_size_t * 5)(*[len(x) for x in small])
    outputs = (c_void_p * 5)(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * 5)(*small_caps)
    results = (c_int32 * 5)(*([7] * 5))
    ret = lib.lib.BrotliMi355xCompressBatchEx(9, 22, 0, c_uint32(Q9), c_size_t(5), inputs, in_sizes, outputs, out_sizes, results)
    assert ret == 0 and list(results) == [0] * 5 and list(out_sizes) == [0] * 5 and "route" in lib.last_error()
    assert _info(lib) == [5, 0, 0, 0, 0, 0, 0, 0]


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"), True)


# ---- 2. each item uses its own dictionary: item i is a verbatim stretch of dictionary i, and the dictionaries are disjoint texts

def _own_dictionary_is_used(lib):
    dictionaries = [synth.alice()[:20000], synth.markov_text(20000, 17), synth.random_bytes(20000)]
    items = [d[5000:9000] for d in dictionaries]
    own = _check(lib, items, dictionaries, [0, 1, 2], 9, 22)
    assert _info(lib)[1] == 3
    rotated = _check(lib, items, dictionaries, [1, 2, 0], 9, 22)
    assert _info(lib)[1] == 3
    for i, (g, r) in enumerate(zip(own, rotated)):
        assert 2 * len(g) < len(r), (i, len(g), len(r))


def test_own_dictionary_is_used_emu():
    _own_dictionary_is_used(test_cabi._load("emu"))


@pytest.mark.gpu
def test_own_dictionary_is_used_gpu():
    _own_dictionary_is_used(test_cabi._load("gpu"))


# ---- 3. edges: the prepend's first stored position (D = 4), the stitch's threshold (3 dictionary bytes, 3 item bytes), partial
# 64-lane filing steps (D - 3 around 64, 128, 256); the items are the text that follows the dictionary, so matches straddle
# dict_break, and one item repeats the dictionary's tail

_EDGE_D = (2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4099)
_EDGE_ITEMS = (1, 2, 3, 4, 6, 7, 8, 127, 128, 129, 700)
_EDGE_AT, _EDGE_STEP = 9000, 531  # (offsets on which the oracle succeeds on every item: checked on the CPU)


def _edge_batch():
    a = synth.alice()
    dictionaries, items, named = [], [], []
    for k, D in enumerate(_EDGE_D):
        at = _EDGE_AT + _EDGE_STEP * k
        dictionaries.append(a[at:at + D])
        mine = [a[at + D:at + D + n] for n in _EDGE_ITEMS] + [a[at + D - min(D, 200):at + D]]
        items += mine
        named += [k] * len(mine)
    return items, dictionaries, named


def _edges(lib, lgwin):
    items, dictionaries, named = _edge_batch()
    _check(lib, items, dictionaries, named, 9, lgwin)
    assert _info(lib)[1] == len(items)
    # ... and each dictionary as the shared one of a call of its own items: the image replayed instead of the chain's filing
    for k in (0, 1, 2, 3, 5, 9, 12, 14):
        mine = [x for x, j in zip(items, named) if j == k]
        ret, got, results, _, info = _raw_shared(lib, 9, lgwin, Q9, dictionaries[k], mine)
        assert ret == 1 and results == [1] * len(mine), (lgwin, k, lib.last_error())
        assert got == [_oracle(x, 9, lgwin, dictionaries[k]) for x in mine], (lgwin, k)
        assert info[:4] == [len(mine), len(mine), 0, 0] and info[5] == len(dictionaries[k]), (lgwin, k, info)


@pytest.mark.parametrize("lgwin", [22, 17])
def test_edges_emu(lgwin):
    _edges(test_cabi._load("emu"), lgwin)


@pytest.mark.gpu
@pytest.mark.parametrize("lgwin", [22, 17])
def test_edges_gpu(lgwin):
    _edges(test_cabi._load("gpu"), lgwin)


# ---- 4. counter wrap and deep rings: a run of one byte files one key more than 65 536 times within dictionary + item (the u16
# counter comes back to 0 inside the item); a text of period 7 files seven keys 5 700 times each, rings 256 deep many times over

def _deep_rings(lib):
    run_d, run_item = b"q" * 65536, b"q" * 4096
    period = bytes(range(65, 72))
    per_d, per_item = (period * 6000)[:40000], (period * 700)[3:3 + 4096]
    for items, dictionaries in (([run_item], [run_d]), ([per_item], [per_d]), ([run_item, per_item, run_item[:100]], [run_d, per_d, run_d])):
        _check(lib, items, dictionaries, None, 9, 22)
        assert _info(lib)[1] == len(items)
    # ... and through the image
    for d, x in ((run_d, run_item), (per_d, per_item)):
        ret, got, results, _, info = _raw_shared(lib, 9, 22, Q9, d, [x, x[:1000]])
        assert ret == 1 and got == [_oracle(x, 9, 22, d), _oracle(x[:1000], 9, 22, d)]
        assert info[:6] == [2, 2, 0, 0, 1, len(d)], info


def test_deep_rings_emu():
    _deep_rings(test_cabi._load("emu"))


@pytest.mark.gpu
def test_deep_rings_gpu():
    _deep_rings(test_cabi._load("gpu"))


# ---- 5. table reuse: one and two tables, groups of ten items (settings are read once per process: a child); a 2-byte and a 129-byte
# dictionary follow a 16 KiB one on the same table, and every item is a stretch of the long dictionaries' text, so a ring slot the
# item in front left in reach would change bytes.  Once per item, once shared (the image replayed over a used table).

def _reuse_batch():
    a = synth.alice()
    sizes = (16384, 2, 129)
    dictionaries = [a[700 * k:700 * k + sizes[k % 3]] for k in range(24)]
    items = [a[4000 + 300 * k:4000 + 300 * k + 1 + (89 * k) % 2048] for k in range(24)]
    items[5] = a[2000:2000 + 2048]
    return items, dictionaries


_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_dictionaries_q9 as t, test_cabi
lib = test_cabi._load(%r)
items, dictionaries = t._reuse_batch()
h = hashlib.sha256()
ret, outs, results, sizes, info = t._raw(lib, 9, 22, t.Q9, dictionaries, None, items)
assert ret == 1 and info[:4] == [24, 24, 0, 0], info
groups = [info[4]]
ret, shared, results, sizes, info = t._raw(lib, 9, 22, t.Q9, dictionaries[:1], [0] * 24, items)
assert ret == 1 and info[:4] == [24, 24, 0, 0] and info[5] == 16384, info
groups.append(info[4])
for out in outs + shared:
    h.update(len(out).to_bytes(8, "little") + out)
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which):
    items, dictionaries = _reuse_batch()
    assert 1 <= min(len(x) for x in items) and max(len(x) for x in items) == 2048
    h = hashlib.sha256()
    for x, d in list(zip(items, dictionaries)) + [(x, dictionaries[0]) for x in items]:
        out = _oracle(x, 9, 22, d)
        h.update(len(out).to_bytes(8, "little") + out)
    want = "digest %s groups %s" % (h.hexdigest(), [3, 3])
    for tables in ("1", "2"):
        env = dict(os.environ)
        env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
        env.pop("BROTLI_MI355X_BATCH_DICT_SELF_FILE", None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "10"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 6. one dictionary, three ways: every item naming index 0 of the per-item call; the same call with a copy of the dictionary per
# item under distinct indices; BrotliMi355xCompressBatchWithDictionaryEx with 4096.  The oracle's bytes from all three; the first
# and the third are one path (equal info, info[5] the dictionary's bytes), the second names n dictionaries.

def _three_ways_batch():
    a = synth.alice()
    d = a[40000:40000 + 12000]
    items = [a[44000:44000 + 3000], b"", a[60000:60000 + 700], synth.random_bytes(900), a[41000:41000 + 5000], b"ab", a[51990:51990 + 400]]
    return items, d


def _three_ways(lib):
    items, d = _three_ways_batch()
    n, caps = len(items), _caps(lib, items)
    want = [_oracle(x, 9, 22, d) for x in items]
    side = n - 1  # (all but the empty item)
    first = _raw(lib, 9, 22, Q9, [d], [0] * n, items, caps)
    second = _raw(lib, 9, 22, Q9, [bytes(bytearray(d)) for _ in range(n)], None, items, caps)
    third = _raw_shared(lib, 9, 22, Q9, d, items, caps)
    for got in (first, second, third):
        assert got[0] == 1 and got[2] == [1] * n and got[1] == want, (got[0], got[2], got[3])
    assert first[4] == third[4], (first[4], third[4])
    assert first[4][:4] == [n, side, 1, 0] and first[4][4] >= 1 and first[4][5:] == [len(d), 0, 0], first[4]
    assert second[4][:4] == [n, side, 1, 0] and second[4][4] >= 1 and second[4][5:] == [n * len(d), 0, 0], second[4]
    # without the bit the shared call runs quality 9 one by one
    plain = _raw_shared(lib, 9, 22, 0, d, items, caps)
    assert plain[0] == 1 and plain[1] == want and plain[4] == [n, 0, n, 0, 0, len(d), 0, 0], plain[4]


def test_three_ways_behind_one_dictionary_emu():
    _three_ways(test_cabi._load("emu"))


@pytest.mark.gpu
def test_three_ways_behind_one_dictionary_gpu():
    _three_ways(test_cabi._load("gpu"))


# ---- 7. an input the reference fails on (a match cut to one byte at the dictionary's end): it fails alone, shared and per item

def _reference_fails(lib):
    a = synth.alice()
    x = open(os.path.join(GOLDEN, "copy_of_length_one.bin"), "rb").read()
    d, bad = x[:64], x[64:]
    items = [a[:3000], bad, a[100:2000], b"tail"]
    with pytest.raises(orc.ReferencePanics):
        _oracle(bad, 9, 22, d)
    want = [_oracle(items[k], 9, 22, d) for k in (0, 2, 3)]
    for shared in (True, False):
        if shared:
            ret, got, results, sizes, info = _raw_shared(lib, 9, 22, Q9, d, items)
        else:
            ret, got, results, sizes, info = _raw(lib, 9, 22, Q9, [d, bytes(bytearray(d))], [0, 1, 0, 1], items)
        assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0, (shared, ret, results, sizes)
        assert "reference encoder fails" in lib.last_error()
        assert info[:6] == [4, 4, 0, 0, 1, 64 if shared else 128], (shared, info)
        assert [got[k] for k in (0, 2, 3)] == want, shared
    # (the per-item call with one index named: the shared path, the same info)
    ret, got, results, sizes, info = _raw(lib, 9, 22, Q9, [d], [0] * 4, items)
    assert ret == 0 and results == [1, 0, 1, 1] and info[:6] == [4, 4, 0, 0, 1, 64], (results, info)


def test_reference_fails_emu():
    _reference_fails(test_cabi._load("emu"))


@pytest.mark.gpu
def test_reference_fails_gpu():
    _reference_fails(test_cabi._load("gpu"))


# ---- 8. capacity: the stream rule -- an item goes out if and only if its stream fits; there is no stored fallback

def _capacity(lib):
    a = synth.alice()
    items = [a[:3000], synth.random_bytes(700), a[100:2000], b"tail"]
    dictionaries = [a[10000:30000], a[:900], synth.markov_text(4000, 6), a[:50]]
    full = [_oracle(x, 9, 22, d) for x, d in zip(items, dictionaries)]
    for k in range(4):
        c = [len(w) for w in full]
        c[k] -= 1
        ret, got, results, sizes, info = _raw(lib, 9, 22, Q9, dictionaries, None, items, c)
        assert ret == 0 and results == [0 if i == k else 1 for i in range(4)] and sizes[k] == 0, (k, ret, results, sizes)
        assert [g for i, g in enumerate(got) if i != k] == [w for i, w in enumerate(full) if i != k]
        assert info[:5] == [4, 4, 0, 0, 1]
    ret, got, _, _, info = _raw(lib, 9, 22, Q9, dictionaries, None, items, [len(w) for w in full], with_results=False)
    assert ret == 1 and got == full and info[:5] == [4, 4, 0, 0, 1]


def test_capacity_emu():
    _capacity(test_cabi._load("emu"))


@pytest.mark.gpu
def test_capacity_gpu():
    _capacity(test_cabi._load("gpu"))


# ---- 9. the device entry: the same bytes and info as the host call, canaries around every output untouched

def _device_entry(lib, which):
    Mem = test_batch_device._mem(which)
    a, m = synth.alice(), synth.markov_text(40000, 3)
    dictionaries = [a[:16384], m[:300], a[28000:33000], a[20000:40000], m[:9000], synth.random_bytes(5000)]
    # (the last item runs one by one: 65 537 bytes)
    items = [b"", b"x", a[30000:35000], a[30000:30000 + 8192], synth.random_bytes(3000), a[1000:1000 + 65537]]
    blocks, at = [], 3
    for blob in dictionaries + items:
        blocks.append(at)
        at += len(blob) + 5
    src = Mem(at, 0)
    for off, blob in zip(blocks, dictionaries + items):
        src.write(off, blob)
    caps = _caps(lib, items)
    out_at, at = [], GUARD
    for c in caps:
        out_at.append(at)
        at += c + GUARD
    n, nd = len(items), len(dictionaries)
    # a dictionary per item, then every item behind dictionary 0 (the shared image, reached by a copy on the device)
    for named, head in (([0, 1, 2, 3, 4, 5], [6, 4, 2, 0]), ([0] * 6, [6, 4, 2, 0])):
        ret, want, want_results, want_sizes, want_info = _raw(lib, 9, 22, Q9, dictionaries, named, items, caps)
        assert ret == 1 and want == [_oracle(x, 9, 22, dictionaries[k]) for x, k in zip(items, named)]
        assert want_info[:4] == head and want_info[4] >= 1, want_info
        dst = Mem(at, FILL)
        Mem.sync()
        dict_ptrs = (c_void_p * nd)(*[src.ptr + o for o in blocks[:nd]])
        dict_sizes = (c_size_t * nd)(*[len(d) for d in dictionaries])
        in_ptrs = (c_void_p * n)(*[src.ptr + o for o in blocks[nd:]])
        in_sizes = (c_size_t * n)(*[len(x) for x in items])
        out_ptrs = (c_void_p * n)(*[dst.ptr + o for o in out_at])
        out_sizes = (c_size_t * n)(*caps)
        results = (c_int32 * n)(*([7] * n))
        ret = lib.lib.BrotliMi355xCompressBatchWithDictionariesDevice(9, 22, 0, c_uint32(Q9), c_size_t(nd), dict_ptrs, dict_sizes, c_size_t(n),
                                                                      (c_size_t * n)(*named), in_ptrs, in_sizes, out_ptrs, out_sizes, results)
        info = _info(lib)
        assert ret == 1 and list(results) == want_results and list(out_sizes) == want_sizes, (named, lib.last_error())
        assert info == want_info, (info, want_info)
        image = dst.read()
        covered = bytearray(len(image))
        for o, cap, size, w in zip(out_at, caps, want_sizes, want):
            assert image[o:o + size] == w, named
            covered[o:o + cap] = b"\x01" * cap
        # (a byte outside every [out, out + capacity) still holds the fill)
        assert all(image[i] == FILL for i in range(len(image)) if not covered[i]), named


def test_device_entry_emu():
    _device_entry(test_cabi._load("emu"), "emu")


@pytest.mark.gpu
def test_device_entry_gpu():
    _device_entry(test_cabi._load("gpu"), "gpu")


# ---- 10. isolation: twenty copies of one item behind different dictionaries, and a shorter one: no chain sees its neighbour's
# text; four threads, each with a routed batch of its own and its own info

def _isolation(lib):
    a = synth.alice()
    item = a[50000:53000]
    dictionaries = [a[49000 - 150 * k:49000 - 150 * k + 600 + 171 * k] for k in range(20)] + [a[51000:52500]]
    items = [item] * 20 + [item[:2999]]
    got = _check(lib, items, dictionaries, None, 9, 22)
    assert _info(lib)[1] == 21
    assert len(set(got[:20])) > 1  # (the dictionaries matter)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"))


def _threads(lib):
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(24)] for t in range(4)]
    dictionaries = [[synth.markov_text(700 * (t + 1), 30 + t), a[5000 * t:5000 * t + 9000], a[1000 * t:1000 * t + 40]] for t in range(4)]
    named = [[(i + t) % 3 for i in range(24)] for t in range(4)]
    want = [[_oracle(x, 9, 22 - t, dictionaries[t][k]) for x, k in zip(batches[t], named[t])] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        ret, outs, _, _, info = _raw(lib, 9, 22 - t, Q9, dictionaries[t], named[t], batches[t])
        got[t], infos[t] = (ret, outs), info  # (BrotliMi355xLastBatchInfo is per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == [(1, w) for w in want]
    assert [i[:4] + i[5:] for i in infos] == [[24, 24, 0, 0, 700 * (t + 1) + 9040, 0, 0] for t in range(4)], infos


def test_threads_emu():
    _threads(test_cabi._load("emu"))


@pytest.mark.gpu
def test_threads_gpu():
    _threads(test_cabi._load("gpu"))


# ---- 11. seeded: items and dictionaries drawn from text, mixed and random sources

_SEEDED_CASES = [(22, 0), (17, 0), (18, 1), (24, 2)]
_SEEDS = {(22, 0): 9220, (17, 0): 9170, (18, 1): 9180, (24, 2): 9240}  # (seeds on which the oracle succeeds on every item: checked on the CPU)


def _seeded_batch(seed):
    rng = random.Random(seed)
    a, m, r = synth.alice(), synth.markov_text(60000, 9), synth.random_bytes(30000)

    def draw(n):
        kind = rng.randrange(3)
        if kind == 0:
            src = a if rng.randrange(2) else m
            at = rng.randrange(len(src) - n)
            return src[at:at + n]
        if kind == 1:  # mixed: stretches of text and of random bytes
            out = b""
            while len(out) < n:
                src = (a, m, r)[rng.randrange(3)]
                k = rng.randrange(1, 400)
                at = rng.randrange(len(src) - k)
                out += src[at:at + k]
            return out[:n]
        at = rng.randrange(len(r) - min(n, len(r) - 1))
        return (r * 2)[at:at + n]

    dictionaries = [draw(rng.choice((2, 3, 129, rng.randrange(2, 16385), rng.randrange(2, 16385)))) for _ in range(12)]
    items = [draw(rng.choice((rng.randrange(1, 300), rng.randrange(1, 4097)))) for _ in range(40)]
    named = [rng.randrange(12) for _ in range(40)]
    return items, dictionaries, named


def _seeded(lib, lgwin, mode):
    items, dictionaries, named = _seeded_batch(_SEEDS[(lgwin, mode)])
    _check(lib, items, dictionaries, named, 9, lgwin, mode)
    assert _info(lib)[1] == 40


@pytest.mark.parametrize("lgwin,mode", _SEEDED_CASES)
def test_seeded_emu(lgwin, mode):
    _seeded(test_cabi._load("emu"), lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("lgwin,mode", _SEEDED_CASES)
def test_seeded_gpu(lgwin, mode):
    _seeded(test_cabi._load("gpu"), lgwin, mode)


# ---- 12. the image against self-filing: BROTLI_MI355X_BATCH_DICT_SELF_FILE=1 (read once per process: a child) gives the shared call
# of case 6 the same streams, every chain filing the dictionary itself

_SELF_FILE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_dictionaries_q9 as t, test_cabi
lib = test_cabi._load(%r)
items, d = t._three_ways_batch()
ret, outs, results, sizes, info = t._raw_shared(lib, 9, 22, t.Q9, d, items)
assert ret == 1 and info[:4] == [len(items), len(items) - 1, 1, 0] and info[5] == len(d), info
h = hashlib.sha256()
for out in outs:
    h.update(len(out).to_bytes(8, "little") + out)
print("digest", h.hexdigest())
"""


def _image_against_self_filing(which):
    items, d = _three_ways_batch()
    h = hashlib.sha256()
    for x in items:
        out = _oracle(x, 9, 22, d)
        h.update(len(out).to_bytes(8, "little") + out)
    want = "digest %s" % h.hexdigest()
    for self_file in (None, "1"):
        env = dict(os.environ)
        env.pop("BROTLI_MI355X_BATCH_DICT_SELF_FILE", None)
        if self_file:
            env["BROTLI_MI355X_BATCH_DICT_SELF_FILE"] = self_file
        r = subprocess.run([sys.executable, "-c", _SELF_FILE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and want in r.stdout, (self_file, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_image_against_self_filing_emu():
    _image_against_self_filing("emu")


@pytest.mark.gpu
def test_image_against_self_filing_gpu():
    _image_against_self_filing("gpu")
