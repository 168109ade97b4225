"""BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS: at qualities 5 to 8 the items of more than one and at most
four input blocks (65 537 to 262 144 bytes) run side by side as well, one live chain each that walks from block to block and leaves
up to four meta-blocks (batch_greedy.h).  routes == 0 is BrotliMi355xCompressBatch.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken: [7] counts the long items taken side by side, [6] those that began side by side and were redone one by
one (a meta-block that is not the item's last took the size fallback).  Every case but the demotion case asserts [6] == 0, so that
none passes through the one-shot path unnoticed.  The CPU tests run the emulation library -- the same host plan and the same item
code -- the GPU tests the product library."""
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

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 65536    # one input block at qualities 5 to 8
CAP = 4 * BLOCK  # the longest item that goes side by side
LONG = 1         # BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


def _short(items, lgwin):
    return sum(1 for x in items if 0 < len(x) <= BLOCK) if 17 <= lgwin <= 24 else 0


def _long(items, lgwin):
    return sum(1 for x in items if BLOCK < len(x) <= CAP) if 17 <= lgwin <= 24 else 0


def _check(lib, items, quality, lgwin, mode=0, demoted=0):
    """the items with the flag set: the oracle's bytes, and the info of a call that took every eligible item side by side"""
    got = lib.compress_batch(items, quality, lgwin, mode, long_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    short, long_ = _short(items, lgwin), _long(items, lgwin)
    assert info[6] == demoted, info
    assert info[:4] == [len(items), short + long_ - demoted, len(items) - short - long_ - empty + demoted, empty], info
    assert info[5] == 0 and info[7] == long_ - demoted, info
    return got, info


def _raw_ex(lib, quality, lgwin, routes, items, caps, with_results=True):
    """BrotliMi355xCompressBatchEx through ctypes: (return value, [bytes], [item result], [size])"""
    n = len(items)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchEx(quality, lgwin, 0, routes, n, inputs, in_sizes, outputs, out_sizes,
                                              results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


# ---- 1. taken side by side

def _taken_side_by_side(lib):
    a = synth.alice()
    items = [b"", a[:5000], a[:BLOCK], a[:BLOCK + 1], a[:2 * BLOCK], a[:2 * BLOCK + 1], a, synth.markov_text(CAP, 3), synth.markov_text(CAP + 1, 3)]
    want = [_oracle(x, 5, 22) for x in items]
    got = lib.compress_batch(items, 5, 22, long_items=True)
    info = lib.last_batch_info()
    assert info[:4] == [9, 7, 1, 1] and info[4] >= 2 and info[5:] == [0, 0, 5], info
    assert got == want
    # routes == 0 and the plain call: today's routing, the same bytes
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    ret, outs, results, _ = _raw_ex(lib, 5, 22, 0, items, caps)
    info = lib.last_batch_info()
    assert ret == 1 and results == [1] * 9 and outs == want
    assert info[:4] == [9, 2, 6, 1] and info[4] == 1 and info[5:] == [0, 0, 0], info
    assert lib.compress_batch(items, 5, 22) == want
    assert lib.last_batch_info() == info
    # qualities and windows the chains do not take: every item one by one, flag or not
    few = items[:5]
    for quality, lgwin in ((9, 22), (2, 22), (5, 16)):
        got = lib.compress_batch(few, quality, lgwin, long_items=True)
        info = lib.last_batch_info()
        assert info[:4] == [5, 0, 4, 1] and info[5:] == [0, 0, 0], (quality, lgwin, info)
        assert got == [_oracle(x, quality, lgwin) for x in few]
    # a route this build does not know fails the whole call, and only info[0] is set
    for routes in (2, LONG | 2, 1 << 31):
        ret, outs, results, sizes = _raw_ex(lib, 5, 22, routes, few, caps[:5])
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert lib.last_batch_info() == [5, 0, 0, 0, 0, 0, 0, 0]
        assert "route" in lib.last_error()


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. block seams and several meta-blocks

@functools.lru_cache(maxsize=None)
def _seam_items():
    a = synth.alice()
    rnd = synth.random_bytes
    # byte 65 533 onward repeats the start: matches begin in the last three positions of the first block (the tail stitch)
    stitched = (a[:65533] + a[:BLOCK] * 2)[:2 * BLOCK]
    assert len(stitched) == 2 * BLOCK and stitched[65533:65533 + 2000] == stitched[:2000]
    return (
        (a[:30000] * 9)[:CAP],                            # a copy runs across every block end: extend_last_command
        synth.mixed(200000, 3),                           # two meta-blocks at lgwin 17, one elsewhere
        a[:70000] + rnd(70000, 9) + a[70000:140000],      # two meta-blocks at lgwin 17 and 18
        rnd(140000, 5) + a[:60000],                       # three meta-blocks at lgwin 17, one stored by should_compress
        a[:60000] + rnd(140000, 5),                       # the final meta-block stored at lgwin 17 to 19: the empty last meta-block
        rnd(200000, 7),                                   # the whole-stream stored fallback of OneShotDeliver
        stitched,
    )


_SEAM_CASES = [(q, w, 0) for q in (5, 6, 7, 8) for w in (17, 18, 22)] + [(5, 22, 1), (5, 22, 6)]


def _seams(lib, quality, lgwin, mode):
    _, info = _check(lib, list(_seam_items()), quality, lgwin, mode)
    assert info[7] == len(_seam_items())


@pytest.mark.parametrize("quality,lgwin,mode", _SEAM_CASES)
def test_seams_emu(quality, lgwin, mode):
    _seams(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _SEAM_CASES)
def test_seams_gpu(quality, lgwin, mode):
    _seams(test_cabi._load("gpu"), quality, lgwin, mode)


# ---- 3. demotion: a meta-block that is not the item's last takes the size fallback
#
# The first block is noise that codes to no less than it takes stored, yet should_compress lets it through: its verdict rests on a
# histogram of every 13th byte, and here exactly those bytes have their top bit cleared (seven bits of entropy where the test wants
# 7.92).  A few four-byte repeats give the block commands, so that the flush rule closes it as a meta-block of its own at lgwin 17
# and the distance cache behind it differs from the one at its start.  The reference stores the meta-block (encode.rs:2141-2163)
# and parses the text behind it from the saved cache.  (The family first proposed for this case -- xorshift noise with a four-byte
# repeat every 80 .. 200 bytes at distance 3000 / 30000, seeds 1 .. 8 -- never gets there: DESIGN.md section 10.)

def noise(n, seed):
    """bytes no entropy coder gains on (synth.random_bytes codes to 97 %)"""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += hashlib.sha256(b"%d:%d" % (seed, k)).digest()
        k += 1
    return out[:n]


def fooling_block(seed, every, dist):
    b = noise(BLOCK, seed)
    for q in range(0, BLOCK, 13):
        b[q] &= 0x7f
    for p in range(dist + 1000, BLOCK - 4, every):
        b[p:p + 4] = b[p - dist:p - dist + 4]
    return bytes(b)


DEMOTION = dict(seed=2, every=3000, dist=20000, lgwin=17)


def _demotion(lib):
    a = synth.alice()
    d = DEMOTION
    bad = fooling_block(d["seed"], d["every"], d["dist"]) + a[:60000]
    items = [a[:140000], bad, a[:9000], synth.mixed(200000, 3)]
    for quality in (5, 8):
        got, info = _check(lib, items, quality, d["lgwin"], demoted=1)
        assert info[6] >= 1 and info[:4] == [4, 3, 1, 0] and info[7] == 2, info


def test_demotion_emu():
    _demotion(test_cabi._load("emu"))


@pytest.mark.gpu
def test_demotion_gpu():
    _demotion(test_cabi._load("gpu"))


# ---- 4. isolation and reuse

def _isolation(lib):
    a = synth.alice()
    items = [a[:140000]] * 32 + [a[:139999]]  # a chain that saw its neighbour would emit one long copy
    for quality in (5, 8):
        _check(lib, items, quality, 22)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"))


def _permutation_items():
    a = synth.alice()
    return list(_seam_items()) + [b"", b"x", a[:700], synth.markov_text(5000, 4), synth.random_bytes(3000), a[:BLOCK]]


def _permutation(lib):
    items = _permutation_items()
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    for quality, lgwin in ((5, 17), (7, 22)):
        straight, _ = _check(lib, items, quality, lgwin)
        shuffled, _ = _check(lib, [items[i] for i in order], quality, lgwin)
        assert shuffled == [straight[i] for i in order]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# two tables, groups of five items (settings are read once per process: one child per setting)
_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_long, test_cabi
lib = test_cabi._load(%r)
items = test_batch_long._permutation_items()
h = hashlib.sha256()
infos = []
for q in (5, 8):
    for out in lib.compress_batch(items, q, 17, long_items=True):
        h.update(len(out).to_bytes(8, "little") + out)
    infos.append(lib.last_batch_info())
print("digest", h.hexdigest(), "infos", infos)
"""


def _reuse(which):
    items = _permutation_items()
    h = hashlib.sha256()
    for q in (5, 8):
        for x in items:
            out = _oracle(x, q, 17)
            h.update(len(out).to_bytes(8, "little") + out)
    short, long_ = _short(items, 17), _long(items, 17)
    groups = (short + 4) // 5 + (long_ + 4) // 5  # short and long items form groups of their own
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
    env.update({"BROTLI_MI355X_BATCH_TABLES": "2", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "5"})
    r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
    info = [len(items), short + long_, 0, 1, groups, 0, 0, long_]
    want = "digest %s infos %s" % (h.hexdigest(), [info, info])
    assert r.returncode == 0 and want in r.stdout, (want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu")


# ---- 5. ABI semantics with a long item: the body of test_batch_greedy._abi_semantics

def _abi_semantics(lib, quality=5):
    import test_batch
    _raw_one = test_batch._raw_one
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q", synth.alice()[:150000]]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes = _raw_ex(lib, quality, 22, LONG, items, roomy)
    assert ret == 1 and results == [1] * len(items)
    assert lib.last_batch_info() == [6, 5, 0, 1, 2, 0, 0, 1]
    for x, cap, out in zip(items, roomy, outs):
        assert (1, out) == _raw_one(lib, quality, 22, x, cap)
    # a buffer too small for item k fails k alone (capacity 0 included), and the call returns 0
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000), (5, 100), (5, 0)):
        caps = list(roomy)
        caps[k] = cap
        assert _raw_one(lib, quality, 22, items[k], cap)[0] == 0
        ret, got, results, sizes = _raw_ex(lib, quality, 22, LONG, items, caps)
        assert ret == 0
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
        assert lib.last_batch_info()[6] == 0
    assert _raw_ex(lib, quality, 22, LONG, [], [])[0] == 1
    ret, got, _, _ = _raw_ex(lib, quality, 22, LONG, items, roomy, with_results=False)
    assert ret == 1 and got == outs
    # an incompressible long item in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    noise = synth.random_bytes(150000)
    cap = max_size(len(noise))
    ok, want = _raw_one(lib, quality, 22, noise, cap)
    ret, got, results, _ = _raw_ex(lib, quality, 22, LONG, [b"abc", noise], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want
    assert lib.last_batch_info()[1] == 2 and lib.last_batch_info()[6:] == [0, 1]
    assert orc.decompress(want, len(noise)) == noise
    # the python wrapper refuses the flag together with a dictionary
    with pytest.raises(ValueError):
        lib.compress_batch(items, quality, 22, dictionary=b"some dictionary", long_items=True)


def test_abi_semantics_emu():
    _abi_semantics(test_cabi._load("emu"))


@pytest.mark.gpu
def test_abi_semantics_gpu():
    _abi_semantics(test_cabi._load("gpu"))


# ---- 6. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

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
    items = [a[:70000], b"tiny", synth.random_bytes(40000, 5) + a[:40000], synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch(items, 5, 17, long_items=True))
        assert lib.last_batch_info() == [4, 4, 0, 0, 2, 0, 0, 2]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 7. threads: four threads, each with a batch of 16 long items

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[t * 300 + i * 50:t * 300 + i * 50 + 66000 + 4000 * i] for i in range(16)] for t in range(4)]
    want = [[_oracle(x, 5, 22) for x in b] for b in batches]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 5, 22, long_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i == [16, 16, 0, 0, 1, 0, 0, 16] for i in infos), infos
