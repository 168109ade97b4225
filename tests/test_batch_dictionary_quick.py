"""BrotliMi355xCompressBatchWithDictionaryEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS / Library.compress_batch_with_dictionary(...,
quick_items=True): the batch call with one custom dictionary shared by every item, at qualities 2 to 4.

Item i is the stream of BrotliEncoderSetCustomDictionary + one BrotliEncoderCompressStream(FINISH) on the same bytes: the oracle's
stream API with the dictionary.  With the route set, at qualities 2 to 4, lgwin 10 to 24, behind a dictionary of at least 2 bytes of
which at most 65 536 are in use, the items of at most one input block (16 384 bytes at quality 2 and 3, 65 536 at quality 4) run
side by side on the device, each chain on a table that starts as the dictionary's (batch_quick.h); every other item goes one by one
through the stream path in the same call.  No item is skipped or tolerated: every stream equals the oracle's.  last_batch_info()
proves which path was taken, so a silent fall-back fails a test.  The CPU tests run the emulation library -- the same host plan and
the same item code -- the GPU tests the product library."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_void_p

import pytest

import orc
import synth
import test_batch
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
QUICK = 4  # BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS
INFO_ENV = ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES")


def _block(quality):
    return 16384 if quality < 4 else 65536  # one input block: lgblock 14 at quality 2 / 3, 16 at quality 4


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, dictionary, mode=0):
    return b"".join(orc.stream_with_flushes(item, [(0, mode), (1, quality), (2, lgwin)], [], dictionary=dictionary))


@functools.lru_cache(maxsize=None)
def _seeded(block):
    return tuple(test_batch._seeded_items(1024, 100, block, 11))


@functools.lru_cache(maxsize=None)
def _seeded_dictionary(seed=7):
    return synth.markov_text(20000, seed)


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _side_by_side(items, quality, lgwin, dictionary):
    if not (2 <= quality <= 4 and 10 <= lgwin <= 24 and len(dictionary) >= 2 and _in_use(quality, lgwin, dictionary) <= 65536):
        return 0
    return sum(1 for x in items if 1 <= len(x) <= _block(quality))


def _raw(lib, quality, lgwin, routes, dictionary, items, caps, mode=0, with_results=True, old_entry=False):
    """BrotliMi355xCompressBatchWithDictionaryEx (old_entry: BrotliMi355xCompressBatchWithDictionary, which has no routes) through
    ctypes: (return value, [bytes], [item result], [size])"""
    n = len(items)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    res = results if with_results else ctypes.cast(None, POINTER(c_int32))
    dict_size = 0 if dictionary is None else len(dictionary)
    if old_entry:
        ret = lib.lib.BrotliMi355xCompressBatchWithDictionary(quality, lgwin, mode, dict_size, dictionary, n, inputs, in_sizes, outputs, out_sizes, res)
    else:
        ret = lib.lib.BrotliMi355xCompressBatchWithDictionaryEx(quality, lgwin, mode, routes, dict_size, dictionary, n, inputs, in_sizes, outputs,
                                                                out_sizes, res)
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


def _check(lib, items, quality, lgwin, dictionary, mode=0):
    got = lib.compress_batch_with_dictionary(items, dictionary, quality, lgwin, mode, quick_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, dictionary, mode), (quality, lgwin, mode, len(dictionary), i, len(item))
    side = _side_by_side(items, quality, lgwin, dictionary)
    assert info[:4] == [len(items), side, len(items) - side, 0] and info[5:] == [_in_use(quality, lgwin, dictionary), 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side (fails where the library has no BrotliMi355xCompressBatchWithDictionaryEx)

def _taken_side_by_side(lib):
    a = synth.alice()
    d = a[:20000]
    for quality in (2, 3, 4):
        block = _block(quality)
        items = [b"", b"x", a[:5000], a[30000:30000 + block], a[30000:30000 + block + 1], synth.random_bytes(3000)]
        caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]
        want = [_oracle(x, quality, 22, d) for x in items]
        ret, outs, results, _ = _raw(lib, quality, 22, QUICK, d, items, caps)
        info = lib.last_batch_info()
        assert ret == 1 and results == [1] * 6, (quality, lib.last_error())
        # the empty item and the one of a block + 1 go one by one, through the stream path: none is "answered without an encoder"
        assert info[:4] == [6, 4, 2, 0] and info[4] >= 1 and info[5:] == [20000, 0, 0], (quality, info)
        assert outs == want, quality
        assert lib.compress_batch_with_dictionary(items, d, quality, 22, quick_items=True) == want
        assert lib.last_batch_info() == info
        # routes == 0, the old entry, and the Python calls without the route: the same bytes, nothing side by side
        for old_entry in (False, True):
            ret, outs, results, _ = _raw(lib, quality, 22, 0, d, items, caps, old_entry=old_entry)
            assert ret == 1 and outs == want, (quality, old_entry)
            assert lib.last_batch_info() == [6, 0, 6, 0, 0, 20000, 0, 0], (quality, old_entry)
        assert lib.compress_batch_with_dictionary(items, d, quality, 22) == want
        assert lib.last_batch_info() == [6, 0, 6, 0, 0, 20000, 0, 0]
        assert lib.compress_batch(items, quality, 22, dictionary=d) == want
        assert lib.last_batch_info() == [6, 0, 6, 0, 0, 20000, 0, 0]
    # the bit changes nothing at quality 5: the items take the dictionary route of the plain call
    items = [b"", b"x", a[:5000], a[30000:30000 + 65536], a[30000:30000 + 65537], synth.random_bytes(3000)]
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]
    want = [_oracle(x, 5, 22, d) for x in items]
    ret, outs, _, _ = _raw(lib, 5, 22, 0, d, items, caps, old_entry=True)
    plain = lib.last_batch_info()
    assert ret == 1 and outs == want and plain[:4] == [6, 4, 2, 0] and plain[5:] == [20000, 0, 0]
    ret, outs, _, _ = _raw(lib, 5, 22, QUICK, d, items, caps)
    assert ret == 1 and outs == want and lib.last_batch_info() == plain
    # ... and nothing at qualities 1 and 9
    for quality in (1, 9):
        ret, outs, _, _ = _raw(lib, quality, 22, QUICK, d, items[:3], caps[:3])
        assert ret == 1 and outs == [_oracle(x, quality, 22, d) for x in items[:3]]
        assert lib.last_batch_info() == [3, 0, 3, 0, 0, _in_use(quality, 22, d), 0, 0], quality
    # a route this call does not know fails the whole call, and only info[0] is set: those of the plain Ex call and the
    # reserved values included
    for routes in (1, 2, 8, 16, 5, 1 << 31):
        ret, outs, results, sizes = _raw(lib, 2, 22, routes, d, items, caps)
        assert ret == 0 and results == [0] * 6 and sizes == [0] * 6, routes
        assert lib.last_batch_info() == [6, 0, 0, 0, 0, 0, 0, 0], routes
        assert "route" in lib.last_error()
    with pytest.raises(ValueError):
        lib.compress_batch(items, 2, 22, dictionary=d, quick_items=True)


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. edge sizes, the smallest at which the chain can go wrong
# dictionaries: 2 and 7 file nothing, 8 files one position; 9 .. 17 and 63 .. 65 move the 16-byte shift of the upload and make
# D % 8 != 0, where the sweep offset (p >> 3) & (sweep - 1) of H3 / H4 differs from the item-local one; 1008 is what lgwin 10 keeps

_DICTIONARY_SIZES = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1008, 16384, 65535, 65536)
_EDGE_WINDOWS = (10, 16, 17, 24)
_EDGE_CASES = [(q, w, 0) for q in (2, 3, 4) for w in _EDGE_WINDOWS] + [(2, 22, 1), (3, 22, 1), (4, 22, 1)]


def _edge_share(quality, lgwin, mode):
    """The windows of a quality share the dictionary sizes out among themselves: every size once per quality, at a window that
    keeps all of it -- (1 << lgwin) - 16 bytes at least, so the two largest meet lgwin 17 and 24 only -- the choice among those
    windows rotated by the quality.  (What a window cuts off is _small_window's.)  A mode takes three sizes of its own, at
    lgwin 22, which keeps every one."""
    n = len(_DICTIONARY_SIZES)
    if mode != 0:
        return [_DICTIONARY_SIZES[(3 * quality + k) % n] for k in (0, 5, 10)]
    mine = []
    for i, size in enumerate(_DICTIONARY_SIZES):
        keeps = [w for w in _EDGE_WINDOWS if size <= (1 << w) - 16]
        if keeps[(i + quality) % len(keeps)] == lgwin:
            mine.append(size)
    return mine


def test_edge_shares_cover_every_size_per_quality():
    for quality in (2, 3, 4):
        seen = []
        for w in _EDGE_WINDOWS:
            share = _edge_share(quality, w, 0)
            assert share and all(s <= (1 << w) - 16 for s in share), (quality, w, share)  # (all of it in use)
            seen += share
        assert sorted(seen) == sorted(_DICTIONARY_SIZES), (quality, seen)
        assert any(s % 8 for s in seen if s > 8)
        # the largest dictionaries the route takes are in use in full under every hasher
        assert {65535, 65536} <= set(_edge_share(quality, 17, 0) + _edge_share(quality, 24, 0))


def _edge_items(quality, at, n):
    """a: the dictionary is a[at:at + n].  Items of every length at which the chain takes another path (7: the stitch threshold,
    9: the first search), cut from the dictionary's own text -- inside it, across its end (a match that starts in the dictionary's
    last bytes is cut at its end) and behind it -- and the dictionary itself"""
    a = synth.alice()
    block = _block(quality)
    lengths = (1, 6, 7, 8, 9, 16, 17, block - 1, block)
    items = [a[at + 3:at + 3 + k] for k in lengths]  # inside the dictionary (a long one), or across its end (a short one)
    items += [a[at + max(0, n - 5):at + max(0, n - 5) + k] for k in (7, 9, 17, 300, block)]  # starts on the dictionary's last bytes
    items += [a[at + n:at + n + k] for k in (8, 9, 40, 2000)]  # goes on where the dictionary stops
    items += [a[at:at + n], a[at:at + n] * 3, bytes(20), synth.random_bytes(600)]
    return items


def _edges(lib, quality, lgwin, mode):
    for n in _edge_share(quality, lgwin, mode):
        at = 1200 + 131 * quality  # (the reference fails on none of these inputs; where it did, _oracle would raise)
        _check(lib, _edge_items(quality, at, n), quality, lgwin, synth.alice()[at:at + n], mode)


@pytest.mark.parametrize("quality,lgwin,mode", _EDGE_CASES)
def test_edge_sizes_emu(quality, lgwin, mode):
    _edges(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _EDGE_CASES)
def test_edge_sizes_gpu(quality, lgwin, mode):
    _edges(test_cabi._load("gpu"), quality, lgwin, mode)


def _small_window(lib):
    """lgwin 10: the reference cuts a 5000-byte dictionary to its last 1008 bytes, still side by side; an item of a whole block
    at quality 2 runs with max_backward_limit far below the position"""
    a = synth.alice()
    d = a[2000:7000]
    for quality in (2, 3, 4):
        items = [a[6000:6000 + k] for k in (1, 9, 500, 1008, 16384)] + [a[7000:9000], d]
        _check(lib, items, quality, 10, d)
        assert lib.last_batch_info()[5] == 1008
        assert _oracle(items[2], quality, 10, d) == _oracle(items[2], quality, 10, d[-1008:])  # (the reference's truncation)
    # dict_size <= 1: no dictionary is taken and nothing goes side by side
    for d in (b"", b"Z"):
        got = lib.compress_batch_with_dictionary([a[:3000], b"", a[50000:50700]], d, 2, 22, quick_items=True)
        assert lib.last_batch_info() == [3, 0, 3, 0, 0, 0, 0, 0], len(d)
        assert got == [_oracle(x, 2, 22, d) for x in (a[:3000], b"", a[50000:50700])]
    # more than 65 536 dictionary bytes in use: one by one
    m = synth.markov_text(70000, 5)
    got = lib.compress_batch_with_dictionary([a[:3000], a[50000:50700]], m, 2, 22, quick_items=True)
    assert lib.last_batch_info() == [2, 0, 2, 0, 0, 70000, 0, 0]
    assert got == [_oracle(x, 2, 22, m) for x in (a[:3000], a[50000:50700])]
    # ... unless the window cuts it down to that: lgwin 16 keeps 65 520
    _check(lib, [a[:3000], a[50000:50700], m[69000:]], 3, 16, m)
    assert lib.last_batch_info()[1] == 3 and lib.last_batch_info()[5] == 65520


def test_small_window_emu():
    _small_window(test_cabi._load("emu"))


@pytest.mark.gpu
def test_small_window_gpu():
    _small_window(test_cabi._load("gpu"))


# ---- 3. the input the reference fails on: the copy at distance 16 leaves the last-distance candidate on the dictionary's last
# byte, and the match is cut to one byte

_FAILS_DICTIONARY = b"ZYXWVUTS01234c"
_FAILS_ITEM = b"abZYXWVUTS56789cabZqrstuvwxyzQRSTUVWXYZ"


def _reference_fails(lib):
    a = synth.alice()
    d, bad = _FAILS_DICTIONARY, _FAILS_ITEM
    items = [a[:3000], bad, a[100:2000], b"tail"]
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(i)) + 1024 for i in items]
    for quality in (2, 3, 4):
        for lgwin in (10, 17, 22):
            with pytest.raises(orc.ReferencePanics):
                _oracle(bad, quality, lgwin, d)
            assert len(_oracle(bad, quality, lgwin, d[:-1] + b"d")) > 0  # (the dictionary's last byte decides)
            ret, got, results, sizes = _raw(lib, quality, lgwin, QUICK, d, items, caps)
            assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0, (quality, lgwin, ret, results, sizes)
            assert "reference encoder fails" in lib.last_error()
            assert lib.last_batch_info()[:6] == [4, 4, 0, 0, 1, 14]
            for k in (0, 2, 3):
                assert got[k] == _oracle(items[k], quality, lgwin, d), (quality, lgwin, k)
        # one by one: the same verdict from the stream path
        ret, got, results, sizes = _raw(lib, quality, 22, 0, d, items, caps)
        assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0 and "reference encoder fails" in lib.last_error()
        assert lib.last_batch_info()[:6] == [4, 0, 4, 0, 0, 14]
        assert [got[k] for k in (0, 2, 3)] == [_oracle(items[k], quality, 22, d) for k in (0, 2, 3)]
    # the Python method raises, and the exception carries the streams of the items that did not fail
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    with pytest.raises(exc) as e:
        lib.compress_batch_with_dictionary(items, d, 2, 22, quick_items=True)
    assert e.value.failed == [1] and "reference encoder fails" in str(e.value)
    assert e.value.streams == [_oracle(items[0], 2, 22, d), None, _oracle(items[2], 2, 22, d), _oracle(items[3], 2, 22, d)]
    # with the dictionary's last byte changed the item goes through, side by side
    _check(lib, items, 2, 22, d[:-1] + b"d")


def test_reference_fails_emu():
    _reference_fails(test_cabi._load("emu"))


@pytest.mark.gpu
def test_reference_fails_gpu():
    _reference_fails(test_cabi._load("gpu"))


# ---- 4. table and group reuse: one table, then two, groups of 50 items (settings are read once per process: one child per
# setting); a table that kept a predecessor's slots, an image copy that skipped the books, or a chain that saw its neighbour,
# changes bytes

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import synth, test_batch, test_cabi
lib = test_cabi._load(%r)
d = synth.markov_text(20000, 7)
a = synth.alice()
isolation = [a[30000:38000]] * 64 + [a[30000:37999]]
h = hashlib.sha256()
groups = []
for q in (2, 3, 4):
    items = test_batch._seeded_items(1024, 100, 16384 if q < 4 else 65536, 11)[:%d]
    for batch, dictionary in ((items, d), (isolation, a[:20000])):
        for out in lib.compress_batch_with_dictionary(batch, dictionary, q, 22, quick_items=True):
            h.update(len(out).to_bytes(8, "little") + out)
        info = lib.last_batch_info()
        assert info[:4] == [len(batch), len(batch), 0, 0] and info[5:] == [20000, 0, 0], info
        groups.append(info[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which, count):
    a = synth.alice()
    isolation = [a[30000:38000]] * 64 + [a[30000:37999]]
    h = hashlib.sha256()
    for q in (2, 3, 4):
        for batch, dictionary in ((_seeded(_block(q))[:count], _seeded_dictionary()), (isolation, a[:20000])):
            for x in batch:
                out = _oracle(x, q, 22, dictionary)
                h.update(len(out).to_bytes(8, "little") + out)
    want = "digest %s groups %s" % (h.hexdigest(), [(count + 49) // 50, 2] * 3)
    for tables in ("1", "2"):
        env = dict(os.environ)
        for name in INFO_ENV:
            env.pop(name, None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which, count)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu", 120)


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu", 300)


def _group_bytes_child(which):
    """the byte limit of a group counts one dictionary copy per item: 10 items of 1000 bytes behind 20000 bytes of dictionary
    under a limit of 100000 bytes are three groups (4 + 4 + 2), the same bytes"""
    code = ("import sys; sys.path.insert(0, %r); import synth, test_cabi; lib = test_cabi._load(%r); a = synth.alice();\n"
            "got = lib.compress_batch_with_dictionary([a[i * 1000:(i + 1) * 1000] for i in range(30, 40)], a[:20000], 2, 22, quick_items=True);\n"
            "info = lib.last_batch_info(); assert info[:4] == [10, 10, 0, 0], info;\n"
            "import hashlib; print('groups', info[4], hashlib.sha256(b''.join(got)).hexdigest())") % (HERE, which)
    a = synth.alice()
    want = hashlib.sha256(b"".join(_oracle(a[i * 1000:(i + 1) * 1000], 2, 22, a[:20000]) for i in range(30, 40))).hexdigest()
    env = dict(os.environ, BROTLI_MI355X_BATCH_GROUP_BYTES="100000")
    env.pop("BROTLI_MI355X_BATCH_GROUP_ITEMS", None)
    env.pop("BROTLI_MI355X_BATCH_TABLES", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "groups 3 " + want in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_group_bytes_count_the_dictionary_emu():
    _group_bytes_child("emu")


@pytest.mark.gpu
def test_group_bytes_count_the_dictionary_gpu():
    _group_bytes_child("gpu")


# ---- 5. seeded sweep: stored meta-blocks (should_compress and the size fallback) behind a dictionary; no item is skipped: every
# one gets the verdict of the oracle

_SEEDED_CASES = [(2, 22), (3, 18), (4, 22), (2, 12)]


def _seeded_sweep(lib, quality, lgwin):
    """Every item gets the oracle's verdict: its stream, or -- where the reference itself fails on it, as on one item of the
    sweep at (2, 12) -- a failure of that item alone.  All of them run side by side."""
    d = _seeded_dictionary()
    items = list(_seeded(_block(quality))[:300])
    want = []
    for x in items:
        try:
            want.append(_oracle(x, quality, lgwin, d))
        except orc.ReferencePanics:
            want.append(None)
    fails = [i for i, w in enumerate(want) if w is None]
    assert len(fails) == (1 if (quality, lgwin) == (2, 12) else 0), (quality, lgwin, fails)
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]
    ret, got, results, sizes = _raw(lib, quality, lgwin, QUICK, d, items, caps)
    assert lib.last_batch_info() == [300, 300, 0, 0, 1, _in_use(quality, lgwin, d), 0, 0]
    assert ret == (0 if fails else 1)
    if fails:
        assert "reference encoder fails" in lib.last_error()
    for i, w in enumerate(want):
        if w is None:
            assert results[i] == 0 and sizes[i] == 0, (quality, lgwin, i)
        else:
            assert results[i] == 1 and got[i] == w, (quality, lgwin, i, len(items[i]))


@pytest.mark.parametrize("quality,lgwin", _SEEDED_CASES)
def test_seeded_emu(quality, lgwin):
    _seeded_sweep(test_cabi._load("emu"), quality, lgwin)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin", _SEEDED_CASES)
def test_seeded_gpu(quality, lgwin):
    _seeded_sweep(test_cabi._load("gpu"), quality, lgwin)


# ---- 6. ABI semantics: the body of test_batch_dictionary._abi_semantics against the new entry, at quality 2

def _abi_semantics(lib, quality=2):
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    d = synth.alice()[20000:40000]
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    want = [_oracle(x, quality, 22, d) for x in items]
    roomy = [max_size(len(x)) + 1024 for x in items]
    ret, outs, results, sizes = _raw(lib, quality, 22, QUICK, d, items, roomy)
    assert ret == 1 and results == [1] * len(items) and outs == want
    assert lib.last_batch_info() == [5, 4, 1, 0, 1, 20000, 0, 0]
    # a buffer too small for item k fails k alone (capacity 0 included; the empty item, which goes one by one, as well), and the
    # call returns 0; a buffer of exactly the stream's size is enough
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000), (4, 0), (0, len(want[0]) - 1)):
        caps = list(roomy)
        caps[k] = cap
        ret, got, results, sizes = _raw(lib, quality, 22, QUICK, d, items, caps)
        assert ret == 0, (k, cap)
        assert results == [0 if i == k else 1 for i in range(len(items))], (k, cap, results)
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(want) if i != k]
        assert lib.last_batch_info() == [5, 4, 1, 0, 1, 20000, 0, 0]
    ret, got, results, sizes = _raw(lib, quality, 22, QUICK, d, items, [len(w) for w in want])
    assert ret == 1 and got == want
    # count == 0; item_results == NULL; a NULL dictionary of size 0
    assert _raw(lib, quality, 22, QUICK, d, [], [])[0] == 1
    assert lib.last_batch_info() == [0, 0, 0, 0, 0, 0, 0, 0]
    assert lib.compress_batch_with_dictionary([], d, quality, 22, quick_items=True) == []
    ret, got, _, _ = _raw(lib, quality, 22, QUICK, d, items, roomy, with_results=False)
    assert ret == 1 and got == want
    assert lib.last_batch_info() == [5, 4, 1, 0, 1, 20000, 0, 0]
    ret, got, results, _ = _raw(lib, quality, 22, QUICK, None, items, roomy)
    assert ret == 1 and results == [1] * len(items) and got == [_oracle(x, quality, 22, b"") for x in items]
    assert lib.last_batch_info() == [5, 0, 5, 0, 0, 0, 0, 0]
    # no fallback to a stored stream: the oracle's stream is the judge of what fits
    noise = synth.random_bytes(16000)
    stream = _oracle(noise, quality, 22, d)
    ret, got, results, _ = _raw(lib, quality, 22, QUICK, d, [b"abc", noise], [64, len(stream)])
    assert ret == 1 and results == [1, 1] and got[1] == stream
    ret, got, results, sizes = _raw(lib, quality, 22, QUICK, d, [b"abc", noise], [64, len(stream) - 1])
    assert ret == 0 and results == [1, 0] and sizes[1] == 0
    assert lib.last_batch_info() == [2, 2, 0, 0, 1, 20000, 0, 0]


def test_abi_semantics_emu():
    _abi_semantics(test_cabi._load("emu"))


@pytest.mark.gpu
def test_abi_semantics_gpu():
    _abi_semantics(test_cabi._load("gpu"))


# ---- 7. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

def test_failed_call_frees_its_blocks_emu():
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    d = synth.alice()[100000:120000]
    items = [synth.alice()[:16000], b"tiny", synth.markov_text(9000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch_with_dictionary(items, d, 3, 22, quick_items=True))
        assert lib.last_batch_info() == [4, 4, 0, 0, 1, 20000, 0, 0]
        return out

    test_device_memory.sweep(L, call, exc)

