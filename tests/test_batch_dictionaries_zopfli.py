"""BrotliMi355xCompressBatchWithDictionaries / ...Device with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS (1024): the batch
call with a custom dictionary per item, at qualities 10 and 11.

Item i is the stream of BrotliEncoderSetCustomDictionary(dicts[item_dicts[i]]) + one BrotliEncoderCompressStream(FINISH) on the same
bytes: the oracle's stream API with that dictionary -- at quality 10 as well as 11, because through the stream API both are Zopfli.
With the route set, at lgwin 10 to 24, an item of 1 to 65 536 bytes behind a dictionary of at least 2 bytes of which at most 65 536
are in use runs side by side on the device: one wavefront that empties H10 trees of its own, files the item's dictionary into them
wave-wide (a lane per class of hash keys), stitches and walks the item the reference's way (batch_zopfli.h).  Every other item goes
one by one through the stream path in the same call.  No item is skipped or tolerated: every stream equals the oracle's, and an
oracle failure on one of these inputs is a test error.  BrotliMi355xLastBatchInfo proves which path was taken, so a silent
fall-back fails a test.  The calls are bound through ctypes here.  The CPU tests run the emulation library -- the same host plan and
the same item code, the wave-wide partition lane by lane -- the GPU tests the product library; there no side-by-side item exceeds
8 KiB (a walk lasts about 37 us per byte), the 64 KiB caps run on the emulation only."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import threading
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

import synth
import test_batch_device
import test_cabi
from test_batch_dictionary import _oracle

HERE = os.path.dirname(os.path.abspath(__file__))
QUICK, Z = 512, 1024  # BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS, BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_DICTIONARY_ITEMS
GUARD = 64
FILL = 0xAA


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _side_by_side(item, quality, lgwin, dictionary):
    return (quality in (10, 11) and 10 <= lgwin <= 24 and len(dictionary) >= 2 and _in_use(quality, lgwin, dictionary) <= 65536
            and 1 <= len(item) <= 65536)


def _info(lib):
    info = (c_uint64 * 8)()
    lib.lib.BrotliMi355xLastBatchInfo.restype = None
    lib.lib.BrotliMi355xLastBatchInfo.argtypes = [POINTER(c_uint64)]
    lib.lib.BrotliMi355xLastBatchInfo(info)
    return list(info)


def _caps(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]


def _raw(lib, quality, lgwin, routes, dictionaries, item_dicts, items, caps=None, with_results=True, mode=0):
    """BrotliMi355xCompressBatchWithDictionaries through ctypes: (return value, [bytes], [item result], [size], info)"""
    caps = _caps(lib, items) if caps is None else caps
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
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionaries(quality, lgwin, mode, c_uint32(routes), nd, dicts, dict_sizes, n, named, inputs, in_sizes,
                                                            outputs, out_sizes, results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n], _info(lib)


def _expected_info(items, dictionaries, item_dicts, quality, lgwin):
    """info[0..3] and info[5..7]; info[4], the groups, is the caller's to check"""
    named = item_dicts if item_dicts is not None else list(range(len(items)))
    side = sum(1 for x, k in zip(items, named) if _side_by_side(x, quality, lgwin, dictionaries[k]))
    return [len(items), side, len(items) - side, 0], [sum(_in_use(quality, lgwin, dictionaries[k]) for k in sorted(set(named))), 0, 0]


def _check(lib, items, dictionaries, item_dicts, quality, lgwin, mode=0, routes=Z):
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


# ---- 1. taken side by side (fails where 1024 is an unknown route of the call)

def _taken_side_by_side(lib, gpu):
    a, m = synth.alice(), synth.markov_text(40000, 3)
    long_d = a[20000:20000 + 65536]
    dictionaries = [a[:16384], m[:300], a[28000:33000], long_d[:20000] if gpu else long_d, m[:9000], synth.random_bytes(5000)]
    items = [b"", b"x", a[30000:35000], a[30000:30000 + 8192], synth.random_bytes(3000)]
    if not gpu:
        items += [a[1000:1000 + 65536], a[1000:1000 + 65537]]
    named = [i % 6 for i in range(len(items))]
    n = len(items)
    side = n - 1 - (0 if gpu else 1)  # all but the empty item and the one of 65 537 bytes
    caps = _caps(lib, items)
    for quality in (10, 11):
        for lgwin in (22, 16):
            in_use = sum(_in_use(quality, lgwin, dictionaries[k]) for k in sorted(set(named)))
            _check(lib, items, dictionaries, named, quality, lgwin)
            info = _info(lib)
            assert info[:4] == [n, side, n - side, 0] and info[4] >= 1 and info[5] == in_use and info[6:] == [0, 0], (quality, lgwin, info)
            # routes == 0: the same bytes, nothing side by side
            if not gpu or (quality, lgwin) == (11, 22):
                want = [_oracle(x, quality, lgwin, dictionaries[k]) for x, k in zip(items, named)]
                ret, outs, _, _, info = _raw(lib, quality, lgwin, 0, dictionaries, named, items, caps)
                assert ret == 1 and outs == want, (quality, lgwin)
                assert info == [n, 0, n, 0, 0, in_use, 0, 0], (quality, lgwin, info)
    small, small_named = items[:5], named[:5]
    small_caps = caps[:5]
    # the bit changes nothing at quality 5: the items take the greedy route, with the same info as without it
    want = [_oracle(x, 5, 22, dictionaries[k]) for x, k in zip(small, small_named)]
    ret, outs, _, _, plain = _raw(lib, 5, 22, 0, dictionaries, small_named, small, small_caps)
    assert ret == 1 and outs == want and plain[:4] == [5, 4, 1, 0], plain
    ret, outs, _, _, info = _raw(lib, 5, 22, Z, dictionaries, small_named, small, small_caps)
    assert ret == 1 and outs == want and info == plain
    # ... and at qualities 2 and 9 everything goes one by one
    for quality in (2, 9):
        ret, outs, _, _, info = _raw(lib, quality, 22, Z, dictionaries, small_named, small, small_caps)
        assert ret == 1 and outs == [_oracle(x, quality, 22, dictionaries[k]) for x, k in zip(small, small_named)], quality
        assert info == [5, 0, 5, 0, 0, sum(_in_use(quality, 22, dictionaries[k]) for k in small_named), 0, 0], (quality, info)
    # 512 | 1024 behaves as each single bit does: at quality 2 as 512, at quality 11 as 1024
    for quality, single in ((2, QUICK), (11, Z)):
        ret, outs, results, _, info = _raw(lib, quality, 22, single, dictionaries, small_named, small, small_caps)
        assert ret == 1 and info[1] == 4, (quality, info)
        ret2, outs2, results2, _, info2 = _raw(lib, quality, 22, QUICK | Z, dictionaries, small_named, small, small_caps)
        assert (ret2, outs2, results2, info2) == (ret, outs, results, info), quality
        assert outs == [_oracle(x, quality, 22, dictionaries[k]) for x, k in zip(small, small_named)], quality
    # a route this call does not know fails the whole call, and only info[0] is set: also beside the one it knows
    for routes in (4, 256, Z | 4, 2048, 1 << 31):
        ret, outs, results, sizes, info = _raw(lib, 11, 22, routes, dictionaries, small_named, small, small_caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert info == [5, 0, 0, 0, 0, 0, 0, 0], routes
        assert "routes %d" % routes in lib.last_error()
    # ... and 1024 is an unknown route of the other batch calls
    bufs = [ctypes.create_string_buffer(c) for c in small_caps]
    inputs, in_sizes = (c_char_p * 5)(*small), (c_size_t * 5)(*[len(x) for x in small])
    outputs = (c_void_p * 5)(*[ctypes.addressof(b) for b in bufs])
    for shared in (False, True):
        out_sizes = (c_size_t * 5)(*small_caps)
        results = (c_int32 * 5)(*([7] * 5))
        if shared:
            ret = lib.lib.BrotliMi355xCompressBatchWithDictionaryEx(11, 22, 0, c_uint32(Z), c_size_t(len(dictionaries[0])), dictionaries[0], c_size_t(5), inputs,
                                                                    in_sizes, outputs, out_sizes, results)
        else:
            ret = lib.lib.BrotliMi355xCompressBatchEx(11, 22, 0, c_uint32(Z), c_size_t(5), inputs, in_sizes, outputs, out_sizes, results)
        assert ret == 0 and list(results) == [0] * 5 and list(out_sizes) == [0] * 5 and "route" in lib.last_error(), shared
        assert _info(lib) == [5, 0, 0, 0, 0, 0, 0, 0]
    # every item naming index 0: there is no shared tree image, the items still go side by side, each chain with its own copy
    _check(lib, small, dictionaries, [0] * 5, 11, 22)
    info = _info(lib)
    assert info[:4] == [5, 4, 1, 0] and info[4] >= 1 and info[5:] == [16384, 0, 0], info


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"), True)


# ---- 2. each item uses its own dictionary: item i is a verbatim stretch of dictionary i, and the dictionaries are disjoint texts

def _own_dictionary_is_used(lib):
    dictionaries = [synth.alice()[:20000], synth.markov_text(20000, 17), synth.random_bytes(20000)]
    items = [d[5000:9000] for d in dictionaries]
    for quality in (10, 11):
        own = _check(lib, items, dictionaries, [0, 1, 2], quality, 22)
        assert _info(lib)[1] == 3
        rotated = _check(lib, items, dictionaries, [1, 2, 0], quality, 22)
        assert _info(lib)[1] == 3
        for i, (g, r) in enumerate(zip(own, rotated)):
            assert 2 * len(g) < len(r), (quality, i, len(g), len(r))


def test_own_dictionary_is_used_emu():
    _own_dictionary_is_used(test_cabi._load("emu"))


@pytest.mark.gpu
def test_own_dictionary_is_used_gpu():
    _own_dictionary_is_used(test_cabi._load("gpu"))


# ---- 3. edges: the prepend's first stored position (D = 128), the stitch's threshold (128 dictionary bytes, 3 item bytes), partial
# 64-lane steps, store_end (128 item bytes); the items are the text that follows the dictionary, so matches straddle dict_break

_EDGE_D = (2, 3, 126, 127, 128, 129, 190, 191, 192, 193, 255, 256, 257, 1000, 4099)
# (6 .. 8 bytes: ChooseContextMode's UTF-8 census reads the ring buffer two bytes in front of the stream -- the dictionary's end -- and
# with zeros there instead, two of at most eight bytes are enough to tip an ASCII item below the 75 % that select the UTF-8 mode)
_EDGE_ITEMS = (1, 2, 3, 4, 6, 7, 8, 127, 128, 129, 700)


def _edge_batch():
    a = synth.alice()
    dictionaries, items, named = [], [], []
    for k, D in enumerate(_EDGE_D):
        at = 9000 + 531 * k
        dictionaries.append(a[at:at + D])
        mine = [a[at + D:at + D + n] for n in _EDGE_ITEMS] + [a[at + D - min(D, 200):at + D]]
        items += mine
        named += [k] * len(mine)
    return items, dictionaries, named


def _edges(lib, quality, lgwin):
    items, dictionaries, named = _edge_batch()
    _check(lib, items, dictionaries, named, quality, lgwin)
    assert _info(lib)[1] == len(items)


_EDGE_CASES = [(10, 22), (11, 22), (10, 10), (11, 10)]


@pytest.mark.parametrize("quality,lgwin", _EDGE_CASES)
def test_edges_emu(quality, lgwin):
    _edges(test_cabi._load("emu"), quality, lgwin)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin", _EDGE_CASES)
def test_edges_gpu(quality, lgwin):
    _edges(test_cabi._load("gpu"), quality, lgwin)


# ---- 4. a window smaller than dictionary + item: forest slots are reused inside the item, and distances end at the window

def _small_window(lib, gpu):
    a, m = synth.alice(), synth.markov_text(70000, 5)
    for quality in (10, 11):
        if gpu:
            _check(lib, [a[5000:5000 + 8192]], [a[:5000]], None, quality, 12)
            assert _info(lib)[:6] == [1, 1, 0, 0, 1, 4080]
        else:
            _check(lib, [m[4464:70000]], [m], None, quality, 16)
            assert _info(lib)[:6] == [1, 1, 0, 0, 1, 65520]
        _check(lib, [a[5000:5000 + 4096], a[3000:3700]], [a[:5000]], [0, 0], quality, 10)
        assert _info(lib)[:6] == [2, 2, 0, 0, 1, 1008]


def test_small_window_emu():
    _small_window(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_small_window_gpu():
    _small_window(test_cabi._load("gpu"), True)


# ---- 5. table reuse: one and two tables, groups of ten items (settings are read once per process: a child); a 2-byte and a 129-byte
# dictionary follow a 16 KiB one on the same table, and every item is a stretch of the long dictionaries' text, so a bucket or a
# forest slot the item in front left in reach would change bytes

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
import test_batch_dictionaries_zopfli as t, test_cabi
lib = test_cabi._load(%r)
items, dictionaries = t._reuse_batch()
h = hashlib.sha256()
groups = []
for q in (10, 11):
    ret, outs, results, sizes, info = t._raw(lib, q, 22, t.Z, dictionaries, None, items)
    assert ret == 1 and info[:4] == [24, 24, 0, 0], info
    for out in outs:
        h.update(len(out).to_bytes(8, "little") + out)
    groups.append(info[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which):
    items, dictionaries = _reuse_batch()
    assert 1 <= min(len(x) for x in items) and max(len(x) for x in items) == 2048
    h = hashlib.sha256()
    for q in (10, 11):
        for x, d in zip(items, dictionaries):
            out = _oracle(x, q, 22, d)
            h.update(len(out).to_bytes(8, "little") + out)
    want = "digest %s groups %s" % (h.hexdigest(), [3, 3])
    for tables in ("1", "2"):
        env = dict(os.environ)
        env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "10"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 6. isolation: twenty copies of one item behind different dictionaries, and a shorter one: no chain sees its neighbour's text

def _isolation(lib):
    a = synth.alice()
    item = a[50000:53000]
    dictionaries = [a[49000 - 150 * k:49000 - 150 * k + 600 + 171 * k] for k in range(20)] + [a[51000:52500]]
    items = [item] * 20 + [item[:2999]]
    for quality in (10, 11):
        got = _check(lib, items, dictionaries, None, quality, 22)
        assert _info(lib)[1] == 21
        assert len(set(got[:20])) > 1  # (the dictionaries matter)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"))


# ---- 7. capacity: the stream rule -- an item goes out if and only if its stream fits; there is no stored fallback

def _capacity(lib):
    a = synth.alice()
    items = [a[:3000], synth.random_bytes(700), a[100:2000], b"tail"]
    dictionaries = [a[10000:30000], a[:900], synth.markov_text(4000, 6), a[:50]]
    for quality in (10, 11):
        full = [_oracle(x, quality, 22, d) for x, d in zip(items, dictionaries)]
        for k in range(4):
            c = [len(w) for w in full]
            c[k] -= 1
            ret, got, results, sizes, info = _raw(lib, quality, 22, Z, dictionaries, None, items, c)
            assert ret == 0 and results == [0 if i == k else 1 for i in range(4)] and sizes[k] == 0, (quality, k, ret, results, sizes)
            assert [g for i, g in enumerate(got) if i != k] == [w for i, w in enumerate(full) if i != k]
            assert info[:5] == [4, 4, 0, 0, 1]
        ret, got, _, _, info = _raw(lib, quality, 22, Z, dictionaries, None, items, [len(w) for w in full], with_results=False)
        assert ret == 1 and got == full and info[:5] == [4, 4, 0, 0, 1]


def test_capacity_emu():
    _capacity(test_cabi._load("emu"))


@pytest.mark.gpu
def test_capacity_gpu():
    _capacity(test_cabi._load("gpu"))


# ---- 8. the device entry: the same bytes and info as the host call, canaries around every output untouched

def _device_entry(lib, which):
    Mem = test_batch_device._mem(which)
    a, m = synth.alice(), synth.markov_text(40000, 3)
    dictionaries = [a[:16384], m[:300], a[28000:33000], a[20000:40000], m[:9000], synth.random_bytes(5000)]
    # (the last item runs one by one: 65 537 bytes)
    items = [b"", b"x", a[30000:35000], a[30000:30000 + 8192], synth.random_bytes(3000), a[1000:1000 + 65537]]
    named = [0, 1, 2, 3, 4, 5]
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
    for quality in (10, 11):
        ret, want, want_results, want_sizes, want_info = _raw(lib, quality, 22, Z, dictionaries, named, items, caps)
        assert ret == 1 and want == [_oracle(x, quality, 22, dictionaries[k]) for x, k in zip(items, named)]
        assert want_info[:4] == [6, 4, 2, 0]
        dst = Mem(at, FILL)
        Mem.sync()
        dict_ptrs = (c_void_p * nd)(*[src.ptr + o for o in blocks[:nd]])
        dict_sizes = (c_size_t * nd)(*[len(d) for d in dictionaries])
        in_ptrs = (c_void_p * n)(*[src.ptr + o for o in blocks[nd:]])
        in_sizes = (c_size_t * n)(*[len(x) for x in items])
        out_ptrs = (c_void_p * n)(*[dst.ptr + o for o in out_at])
        out_sizes = (c_size_t * n)(*caps)
        results = (c_int32 * n)(*([7] * n))
        ret = lib.lib.BrotliMi355xCompressBatchWithDictionariesDevice(quality, 22, 0, c_uint32(Z), c_size_t(nd), dict_ptrs, dict_sizes, c_size_t(n),
                                                                      (c_size_t * n)(*named), in_ptrs, in_sizes, out_ptrs, out_sizes, results)
        info = _info(lib)
        assert ret == 1 and list(results) == want_results and list(out_sizes) == want_sizes, (quality, lib.last_error())
        assert info == want_info, (info, want_info)
        image = dst.read()
        covered = bytearray(len(image))
        for o, cap, size, w in zip(out_at, caps, want_sizes, want):
            assert image[o:o + size] == w, quality
            covered[o:o + cap] = b"\x01" * cap
        # (a byte outside every [out, out + capacity) still holds the fill)
        assert all(image[i] == FILL for i in range(len(image)) if not covered[i]), quality


def test_device_entry_emu():
    _device_entry(test_cabi._load("emu"), "emu")


@pytest.mark.gpu
def test_device_entry_gpu():
    _device_entry(test_cabi._load("gpu"), "gpu")


# ---- 9. seeded: items and dictionaries drawn from text, mixed and random sources

_SEEDED_CASES = [(10, 22, 0), (11, 22, 0), (11, 10, 0), (10, 18, 1), (11, 17, 2)]


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


def _seeded(lib, quality, lgwin, mode):
    items, dictionaries, named = _seeded_batch(1000 * quality + lgwin + mode)
    _check(lib, items, dictionaries, named, quality, lgwin, mode)
    assert _info(lib)[1] == 40


@pytest.mark.parametrize("quality,lgwin,mode", _SEEDED_CASES)
def test_seeded_emu(quality, lgwin, mode):
    _seeded(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _SEEDED_CASES)
def test_seeded_gpu(quality, lgwin, mode):
    _seeded(test_cabi._load("gpu"), quality, lgwin, mode)


# ---- 10. the prepend by itself (brotli_mi355x_debug_zopfli_prepend): the wave-wide partition leaves the buckets and the forest of
# the one-lane loop, bit for bit

def _prepend(lib, text, D, lgwin, mode):
    slots = min((D + 63) & ~63, 1 << lgwin)
    buckets = (c_uint32 * (1 << 17))()
    forest = (c_uint32 * max(1, 2 * slots))()
    ret = lib.lib.brotli_mi355x_debug_zopfli_prepend(text, c_uint32(len(text)), c_uint32(D), c_uint32(lgwin), c_uint32(mode), buckets, forest)
    assert ret == 0, (ret, D, lgwin, mode)
    return bytes(buckets), bytes(forest)[:8 * slots]


def _prepend_cases():
    a = synth.alice()
    cases = [(a[1000:1000 + D + 300], D) for D in _EDGE_D] + [(a[:8192 + 100], 8192), (a[:65536 + 100], 65536)]
    cases += [(synth.random_bytes(8192), 8192), (b"a" * 8192, 8192)]
    return cases


def _prepend_parity(lib, other=None):
    for lgwin in (22, 10):
        for text, D in _prepend_cases():
            D = min(D, (1 << lgwin) - 16)
            lane0 = _prepend(lib, text, D, lgwin, 0)
            wide = _prepend(lib, text, D, lgwin, 1)
            assert wide == lane0, (lgwin, D)
            invalid = (0x100000000 - ((1 << lgwin) - 1)).to_bytes(4, "little")
            assert (D >= 128) == (lane0[0] != invalid * (1 << 17)), (lgwin, D)  # (something was stored)
            if other is not None:
                assert _prepend(other, text, D, lgwin, 1) == wide, (lgwin, D)


def test_prepend_parity_emu():
    _prepend_parity(test_cabi._load("emu"))


@pytest.mark.gpu
def test_prepend_parity_gpu():
    _prepend_parity(test_cabi._load("gpu"), test_cabi._load("emu"))


# ---- 11. threads: four threads, each with a routed batch of its own

def _threads(lib):
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(24)] for t in range(4)]
    dictionaries = [[synth.markov_text(700 * (t + 1), 30 + t), a[5000 * t:5000 * t + 9000], a[1000 * t:1000 * t + 40]] for t in range(4)]
    named = [[(i + t) % 3 for i in range(24)] for t in range(4)]
    want = [[_oracle(x, 10 + t % 2, 22, dictionaries[t][k]) for x, k in zip(batches[t], named[t])] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        ret, outs, _, _, info = _raw(lib, 10 + t % 2, 22, Z, dictionaries[t], named[t], batches[t])
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
