"""BrotliMi355xCompressBatchWithDictionary / Library.compress_batch(..., dictionary=d): the batch call with one custom dictionary
shared by every item.

Item i is the stream of BrotliEncoderSetCustomDictionary + one BrotliEncoderCompressStream(FINISH) on the same bytes: the oracle's
stream API with the dictionary.  At qualities 5 to 8, lgwin 17 to 24, behind a dictionary of 2 to 65 536 bytes the items of 1 to
65 536 bytes run side by side on the device, each chain on a table that already holds the dictionary (batch_greedy.h); every other
item goes one by one through the stream path in the same call.  last_batch_info() proves which path was taken.  The CPU tests run
the emulation library -- the same host plan and the same item code -- the GPU tests the product library."""
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
import test_batch
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BLOCK = 65536  # one input block at qualities 5 to 8; also the longest dictionary that goes side by side


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, dictionary, mode=0):
    return b"".join(orc.stream_with_flushes(item, [(0, mode), (1, quality), (2, lgwin)], [], dictionary=dictionary))


@functools.lru_cache(maxsize=None)
def _seeded():
    return tuple(test_batch._seeded_items(1024, 100, 65536, 11))


@functools.lru_cache(maxsize=None)
def _seeded_dictionary(seed=7):
    return synth.markov_text(20000, seed)


def _side_by_side(items, quality, lgwin, dictionary):
    if not (5 <= quality <= 8 and 17 <= lgwin <= 24 and 2 <= len(dictionary) <= BLOCK):
        return 0
    return sum(1 for x in items if 1 <= len(x) <= BLOCK)


def _in_use(quality, lgwin, dictionary):
    return 0 if len(dictionary) <= 1 or quality <= 1 else min(len(dictionary), (1 << lgwin) - 16)


def _check(lib, items, quality, lgwin, dictionary, mode=0):
    got = lib.compress_batch(items, quality, lgwin, mode, dictionary=dictionary)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, dictionary, mode), (quality, lgwin, mode, len(dictionary), i, len(item))
    side = _side_by_side(items, quality, lgwin, dictionary)
    assert info[:4] == [len(items), side, len(items) - side, 0] and info[5:] == [_in_use(quality, lgwin, dictionary), 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side (fails where the library has no BrotliMi355xCompressBatchWithDictionary)

def _taken_side_by_side(lib):
    a = synth.alice()
    d = a[:20000]
    items = [b"", b"x", a[30000:35000], a[30000:30000 + BLOCK], a[30000:30000 + BLOCK + 1], synth.random_bytes(3000)]
    got = lib.compress_batch(items, 5, 22, dictionary=d)
    info = lib.last_batch_info()
    # the empty and the long item go one by one, through the stream path: none is "answered without an encoder"
    assert info[:4] == [6, 4, 2, 0] and info[4] >= 1 and info[5:] == [20000, 0, 0], info
    assert got == [_oracle(x, 5, 22, d) for x in items]
    for quality, lgwin, in_use in ((9, 22, 20000), (2, 22, 20000), (0, 22, 0), (5, 16, 20000)):
        got = lib.compress_batch(items, quality, lgwin, dictionary=d)
        info = lib.last_batch_info()
        assert info[:6] == [6, 0, 6, 0, 0, in_use], (quality, lgwin, info)
        assert got == [_oracle(x, quality, lgwin, d) for x in items], (quality, lgwin)


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. the dictionary is used: an item that is a verbatim stretch of it shrinks to a fraction of its plain stream

def _dictionary_is_used(lib):
    a = synth.alice()
    d = a[:20000]
    items = [a[5000:5000 + n] for n in (500, 4000)]
    for quality in (5, 8):
        got = _check(lib, items, quality, 22, d)
        plain = lib.compress_batch(items, quality, 22)
        for g, p, x in zip(got, plain, items):
            assert 2 * len(g) < len(p), (quality, len(x), len(g), len(p))


def test_dictionary_is_used_emu():
    _dictionary_is_used(test_cabi._load("emu"))


@pytest.mark.gpu
def test_dictionary_is_used_gpu():
    _dictionary_is_used(test_cabi._load("gpu"))


# ---- 3. identity set

_IDENTITY_CASES = [(q, w, 0) for q in (5, 6, 7, 8) for w in (22, 24, 17)] + [(5, 22, 1), (5, 22, 2), (5, 22, 6)]
_DICTIONARY_SIZES = (2, 3, 7, 8, 9, 64, 1000, 20000, 65536)


@functools.lru_cache(maxsize=None)
def _dictionaries():
    """every size once from the book and once from generated text: 18 dictionaries"""
    a, m = synth.alice(), synth.markov_text(70000, 21)
    return tuple([a[1000:1000 + n] for n in _DICTIONARY_SIZES] + [m[300:300 + n] for n in _DICTIONARY_SIZES])


def _golden_small():
    return [x for x in test_batch._golden_small() if len(x) <= BLOCK]


@functools.lru_cache(maxsize=None)
def _identity_items():
    a = synth.alice()
    return tuple([a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, BLOCK - 1, BLOCK)] + _golden_small() +
                 [bytes(30000), synth.random_bytes(20000)])


def _identity(lib, quality, lgwin, mode):
    """The windows of a quality share the dictionaries out among themselves: every size once per quality, from the book or from
    generated text, the share rotated by one for the second source -- so the 64 KiB dictionary meets lgwin 17 (from the book) and
    lgwin 22 (generated).  A mode takes two.  Every call adds the dictionary itself as an item.  Then one dictionary that stops in
    the middle of the text the item goes on with: matches straddle the dictionary end, and the dict_break rule (mod.rs:42-54)
    decides."""
    a = synth.alice()
    dictionaries = _dictionaries()
    if mode == 0:
        part = (22, 24, 17).index(lgwin)
        mine = [d for i, d in enumerate(dictionaries) if (i + i // len(_DICTIONARY_SIZES)) % 3 == part][(quality & 1)::2]
    else:
        part = (1, 2, 6).index(mode)
        mine = [dictionaries[7 + part], dictionaries[9 + 3 * part]]
    for d in mine:
        _check(lib, list(_identity_items()) + [d], quality, lgwin, d, mode)
    c = (12000, 47000, 101000)[part]
    _check(lib, [a[c:c + 5000], a[c - 2:c + 40], a[c - 9000:c - 8000]], quality, lgwin, a[c - 9000:c], mode)


def test_identity_shares_cover_every_size_per_quality():
    n = len(_DICTIONARY_SIZES)
    for quality in (5, 6, 7, 8):
        seen = []
        for part in range(3):
            seen += [i % n for i in range(2 * n) if (i + i // n) % 3 == part][(quality & 1)::2]
        assert sorted(seen) == list(range(n)), (quality, seen)


@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_emu(quality, lgwin, mode):
    _identity(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_gpu(quality, lgwin, mode):
    _identity(test_cabi._load("gpu"), quality, lgwin, mode)


# ---- 4. seeded set: stored meta-blocks (should_compress and the size fallback) behind a dictionary; no item is skipped

_SEEDED_CASES = [(5, 22), (6, 22), (7, 22), (8, 22), (8, 17)]


@pytest.mark.parametrize("quality,lgwin", _SEEDED_CASES)
def test_seeded_emu(quality, lgwin):
    _check(test_cabi._load("emu"), list(_seeded()[:300]), quality, lgwin, _seeded_dictionary())


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin", _SEEDED_CASES)
def test_seeded_gpu(quality, lgwin):
    _check(test_cabi._load("gpu"), list(_seeded()[:300]), quality, lgwin, _seeded_dictionary())


# ---- 5. the input the reference fails on: a match cut to one byte at the dictionary end

def _raw_batch(lib, quality, lgwin, dictionary, items, caps, with_results=True):
    """BrotliMi355xCompressBatchWithDictionary through ctypes: (return value, [bytes], [item result], [size])"""
    n = len(items)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionary(quality, lgwin, 0, 0 if dictionary is None else len(dictionary), dictionary, n, inputs,
                                                          in_sizes, outputs, out_sizes,
                                                          results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


def _reference_fails(lib):
    a = synth.alice()
    x = open(os.path.join(GOLDEN, "copy_of_length_one.bin"), "rb").read()
    d, bad = x[:64], x[64:]
    items = [a[:3000], bad, a[100:2000], b"tail"]
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(i)) + 1024 for i in items]
    for quality, lgwin in ((6, 20), (5, 22), (8, 17)):
        with pytest.raises(orc.ReferencePanics):
            _oracle(bad, quality, lgwin, d)
        ret, got, results, sizes = _raw_batch(lib, quality, lgwin, d, items, caps)
        assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0, (quality, lgwin, ret, results, sizes)
        assert "reference encoder fails" in lib.last_error()
        assert lib.last_batch_info()[:6] == [4, 4, 0, 0, 1, 64]
        for k in (0, 2, 3):
            assert got[k] == _oracle(items[k], quality, lgwin, d), (quality, lgwin, k)
    # one by one (a quality that does not go side by side): the same verdict from the stream path
    with pytest.raises(orc.ReferencePanics):
        _oracle(bad, 9, 22, d)
    ret, got, results, sizes = _raw_batch(lib, 9, 22, d, items, caps)
    assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0 and "reference encoder fails" in lib.last_error()
    assert lib.last_batch_info()[:6] == [4, 0, 4, 0, 0, 64]
    assert [got[k] for k in (0, 2, 3)] == [_oracle(items[k], 9, 22, d) for k in (0, 2, 3)]


def test_reference_fails_emu():
    _reference_fails(test_cabi._load("emu"))


@pytest.mark.gpu
def test_reference_fails_gpu():
    _reference_fails(test_cabi._load("gpu"))


# ---- 6. one by one, same bytes: dictionaries that are too short or too long, an item of three blocks

def _one_by_one(lib, long_item):
    a = synth.alice()
    m = synth.markov_text(140000, 5)
    items = [a[:3000], b"", a[50000:50700]]
    for d in (b"", m[:1], m[:70000], m):
        got = lib.compress_batch(items, 5, 17, dictionary=d)
        info = lib.last_batch_info()
        assert info[:6] == [3, 0, 3, 0, 0, _in_use(5, 17, d)], (len(d), info)
        assert got == [_oracle(x, 5, 17, d) for x in items], len(d)
    assert _in_use(5, 17, m) == (1 << 17) - 16
    assert _oracle(items[0], 5, 17, m) == _oracle(items[0], 5, 17, m[-((1 << 17) - 16):])  # (the reference's truncation)
    # an item of three input blocks among short ones
    d = a[:20000]
    items = [a[30000:31000], long_item, a[40000:40100]]
    got = lib.compress_batch(items, 5, 22, dictionary=d)
    assert lib.last_batch_info()[:6] == [3, 2, 1, 0, 1, 20000]
    assert got == [_oracle(x, 5, 22, d) for x in items]
    got = lib.compress_batch([long_item], 5, 22, dictionary=d)
    assert lib.last_batch_info()[:6] == [1, 0, 1, 0, 0, 20000]
    assert got == [_oracle(long_item, 5, 22, d)]


def test_one_by_one_emu():
    _one_by_one(test_cabi._load("emu"), synth.markov_text(3 * BLOCK, 8))


@pytest.mark.gpu
def test_one_by_one_gpu():
    _one_by_one(test_cabi._load("gpu"), synth.markov_text(3 * BLOCK, 8))


# ---- 7. table and group reuse: two tables, groups of 50 items (settings are read once per process: one child per setting); a
# table that kept a predecessor's entries, or a chain that saw its neighbour, changes bytes

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import synth, test_batch, test_cabi
lib = test_cabi._load(%r)
items = test_batch._seeded_items(1024, 100, 65536, 11)[:%d]
d = synth.markov_text(20000, 7)
a = synth.alice()
isolation = [a[30000:50000]] * 64 + [a[30000:49999]]
h = hashlib.sha256()
groups = []
for q in (5, 8):
    for batch, dictionary in ((items, d), (isolation, a[:20000])):
        for out in lib.compress_batch(batch, q, 22, dictionary=dictionary):
            h.update(len(out).to_bytes(8, "little") + out)
        groups.append(lib.last_batch_info()[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which, count):
    a = synth.alice()
    isolation = [a[30000:50000]] * 64 + [a[30000:49999]]
    h = hashlib.sha256()
    for q in (5, 8):
        for batch, dictionary in ((_seeded()[:count], _seeded_dictionary()), (isolation, a[:20000])):
            for x in batch:
                out = _oracle(x, q, 22, dictionary)
                h.update(len(out).to_bytes(8, "little") + out)
    for settings, groups in (({"BROTLI_MI355X_BATCH_TABLES": "2", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"}, [(count + 49) // 50, 2] * 2),
                             ({}, [1, 1] * 2)):
        env = dict(os.environ)
        for name in ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES"):
            env.pop(name, None)
        env.update(settings)
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which, count)], env=env, capture_output=True, text=True, timeout=600)
        want = "digest %s groups %s" % (h.hexdigest(), groups)
        assert r.returncode == 0 and want in r.stdout, (settings, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu", 120)


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu", 300)


def _group_bytes_child(which):
    """the byte limit of a group counts one dictionary copy per item: 10 items of 1000 bytes behind 20000 bytes of dictionary
    under a limit of 100000 bytes are three groups (4 + 4 + 2), the same bytes"""
    code = ("import sys; sys.path.insert(0, %r); import synth, test_cabi; lib = test_cabi._load(%r); a = synth.alice();\n"
            "got = lib.compress_batch([a[i * 1000:(i + 1) * 1000] for i in range(30, 40)], 5, 22, dictionary=a[:20000]);\n"
            "import hashlib; print('groups', lib.last_batch_info()[4], hashlib.sha256(b''.join(got)).hexdigest())") % (HERE, which)
    a = synth.alice()
    want = hashlib.sha256(b"".join(_oracle(a[i * 1000:(i + 1) * 1000], 5, 22, a[:20000]) for i in range(30, 40))).hexdigest()
    env = dict(os.environ, BROTLI_MI355X_BATCH_GROUP_BYTES="100000")
    env.pop("BROTLI_MI355X_BATCH_GROUP_ITEMS", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "groups 3 " + want in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_group_bytes_count_the_dictionary_emu():
    _group_bytes_child("emu")


# ---- 8. permutation

def _permutation(lib):
    a = synth.alice()
    d = a[:20000]
    items = list(_identity_items()) + [synth.markov_text(n, n) for n in (200, 900, 5000, 60000)] + [b"", a[:BLOCK + 1]]
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    for quality in (5, 7):
        straight = lib.compress_batch(items, quality, 22, dictionary=d)
        shuffled = lib.compress_batch([items[i] for i in order], quality, 22, dictionary=d)
        assert lib.last_batch_info()[1] == len(items) - 2  # (all but the empty and the long item)
        assert shuffled == [straight[i] for i in order]
        assert straight == [_oracle(x, quality, 22, d) for x in items]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# ---- 9. ABI semantics: the body of test_batch_greedy._abi_semantics against the new entry

def _abi_semantics(lib, quality=5):
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    d = synth.alice()[20000:40000]
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    want = [_oracle(x, quality, 22, d) for x in items]
    roomy = [max_size(len(x)) + 1024 for x in items]
    ret, outs, results, sizes = _raw_batch(lib, quality, 22, d, items, roomy)
    assert ret == 1 and results == [1] * len(items) and outs == want
    assert lib.last_batch_info()[:6] == [5, 4, 1, 0, 1, 20000]
    # a buffer too small for item k fails k alone (capacity 0 included; the empty item, which goes one by one, as well), and the
    # call returns 0; a buffer of exactly the stream's size is enough
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000), (4, 0), (0, len(want[0]) - 1)):
        caps = list(roomy)
        caps[k] = cap
        ret, got, results, sizes = _raw_batch(lib, quality, 22, d, items, caps)
        assert ret == 0, (k, cap)
        assert results == [0 if i == k else 1 for i in range(len(items))], (k, cap, results)
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(want) if i != k]
    ret, got, results, sizes = _raw_batch(lib, quality, 22, d, items, [len(w) for w in want])
    assert ret == 1 and got == want
    # count == 0; item_results == NULL; a NULL dictionary of size 0
    assert _raw_batch(lib, quality, 22, d, [], [])[0] == 1
    assert lib.last_batch_info()[:6] == [0, 0, 0, 0, 0, 0]
    ret, got, _, _ = _raw_batch(lib, quality, 22, d, items, roomy, with_results=False)
    assert ret == 1 and got == want
    ret, got, results, _ = _raw_batch(lib, quality, 22, None, items, roomy)
    assert ret == 1 and results == [1] * len(items) and got == [_oracle(x, quality, 22, b"") for x in items]
    assert lib.last_batch_info()[:6] == [5, 0, 5, 0, 0, 0]
    # no fallback to a stored stream: an incompressible item of one input block may outgrow BrotliEncoderMaxCompressedSize -- the
    # oracle's stream is the judge of what fits
    noise = synth.random_bytes(60000)
    stream = _oracle(noise, quality, 22, d)
    ret, got, results, _ = _raw_batch(lib, quality, 22, d, [b"abc", noise], [64, len(stream)])
    assert ret == 1 and results == [1, 1] and got[1] == stream
    ret, got, results, sizes = _raw_batch(lib, quality, 22, d, [b"abc", noise], [64, len(stream) - 1])
    assert ret == 0 and results == [1, 0] and sizes[1] == 0


def test_abi_semantics_emu():
    _abi_semantics(test_cabi._load("emu"))


@pytest.mark.gpu
def test_abi_semantics_gpu():
    _abi_semantics(test_cabi._load("gpu"))


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
    d = synth.alice()[100000:120000]
    items = [synth.alice()[:20000], b"tiny", synth.markov_text(60000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch(items, 5, 22, dictionary=d))
        assert lib.last_batch_info()[:6] == [4, 4, 0, 0, 1, 20000]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 11. threads: four threads, each with a dictionary and a batch of its own

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    batches = [list(_seeded()[256 * t:256 * (t + 1)]) for t in range(4)]
    dictionaries = [synth.markov_text(5000 * (t + 1), 30 + t) for t in range(4)]
    want = [[_oracle(x, 5, 22, dictionaries[t]) for x in batches[t]] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 5, 22, dictionary=dictionaries[t])
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert [i[:4] + [i[5]] for i in infos] == [[256, 256, 0, 0, 5000 * (t + 1)] for t in range(4)], infos


# ---- 12. every chain filing the dictionary itself (BROTLI_MI355X_BATCH_DICT_SELF_FILE, the other arm of the A/B in DESIGN.md
# section 10; read once per process): the same bytes as the image replay, on tables that are reused

_SELF_FILE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import synth, test_batch, test_cabi
lib = test_cabi._load(%r)
items = test_batch._seeded_items(1024, 100, 65536, 11)[:60]
h = hashlib.sha256()
for q, d in ((5, synth.markov_text(20000, 7)), (8, synth.alice()[:65536]), (6, b"ab")):
    for out in lib.compress_batch(items, q, 22, dictionary=d):
        h.update(len(out).to_bytes(8, "little") + out)
    assert lib.last_batch_info()[1] == 60
print("digest", h.hexdigest())
"""


def _self_file(which):
    h = hashlib.sha256()
    for q, d in ((5, _seeded_dictionary()), (8, synth.alice()[:65536]), (6, b"ab")):
        for x in _seeded()[:60]:
            out = _oracle(x, q, 22, d)
            h.update(len(out).to_bytes(8, "little") + out)
    for value in ("1", "0"):
        env = dict(os.environ, BROTLI_MI355X_BATCH_DICT_SELF_FILE=value, BROTLI_MI355X_BATCH_TABLES="3")
        r = subprocess.run([sys.executable, "-c", _SELF_FILE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "digest " + h.hexdigest() in r.stdout, (value, r.stdout[-2000:] + r.stderr[-3000:])


def test_self_filing_arm_emu():
    _self_file("emu")


@pytest.mark.gpu
def test_self_filing_arm_gpu():
    _self_file("gpu")


# ---- 13. the stream API itself with a dictionary too short to prime (0 or 1 bytes): catable and appendable are turned on behind
# the encoder's initialisation (encode.rs:1237-1241), so the stream is written as a catable one but starts from the usual last
# distances.  What the batch call's one-by-one path rests on, checked directly against the oracle -- one FINISH, and with a flush

def _short_dictionary_stream(lib):
    a = synth.alice()
    for quality, lgwin in ((2, 22), (5, 22), (5, 17), (9, 22), (10, 18)):
        for d in (b"", b"Z"):
            for item, cuts in ((a[:9000], []), (a[3000:3100], []), (a[:40000], [15000])):
                params = [(0, 0), (1, quality), (2, lgwin)]
                want = orc.stream_with_flushes(item, params, cuts, dictionary=d)
                e = lib.encoder(params=params, dictionary=d)
                try:
                    got, at = [], 0
                    for cut in cuts:
                        got.append(e.flush(item[at:cut]))
                        at = cut
                    e._stream(2, item[at:])
                    got.append(bytes(e._out))
                finally:
                    e.close()
                assert got == want, (quality, lgwin, len(d), len(item), cuts)


def test_short_dictionary_stream_emu():
    _short_dictionary_stream(test_cabi._load("emu"))


@pytest.mark.gpu
def test_short_dictionary_stream_gpu():
    _short_dictionary_stream(test_cabi._load("gpu"))
