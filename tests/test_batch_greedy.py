"""BrotliMi355xCompressBatch at qualities 5 to 8: the items of at most one input block run side by side on the device, one live
chain and one meta-block each (batch_greedy.h); every other item goes one by one in the same call.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken.  The CPU tests run the emulation library -- the same host plan and the same item code -- the GPU tests
the product library."""
import functools
import hashlib
import os
import random
import subprocess
import sys
import threading

import pytest

import orc
import synth
import test_batch
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 65536  # one input block at qualities 5 to 8


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


@functools.lru_cache(maxsize=None)
def _seeded():
    return tuple(test_batch._seeded_items(1024, 100, 65536, 11))


def _eligible(items, lgwin=22):
    return sum(1 for x in items if 0 < len(x) <= BLOCK) if 17 <= lgwin <= 24 else 0


def _check(lib, items, quality, lgwin, mode=0):
    got = lib.compress_batch(items, quality, lgwin, mode)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    side = _eligible(items, lgwin)
    assert info[:4] == [len(items), side, len(items) - side - empty, empty] and info[5:] == [0, 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side (fails where the library has no BrotliMi355xLastBatchInfo)

def _taken_side_by_side(lib):
    a = synth.alice()
    items = [b"", b"x", a[:5000], a[:BLOCK], a[:BLOCK + 1], synth.random_bytes(3000)]
    got = lib.compress_batch(items, 5, 22)
    info = lib.last_batch_info()
    assert info[:4] == [6, 4, 1, 1] and info[4] >= 1 and info[5:] == [0, 0, 0], info
    assert got == [_oracle(x, 5, 22) for x in items]
    got = lib.compress_batch(items, 9, 22)
    info = lib.last_batch_info()
    assert info[1] == 0 and info[2] == 5, info
    assert got == [_oracle(x, 9, 22) for x in items]
    got = lib.compress_batch(items, 0, 22)
    info = lib.last_batch_info()
    assert info[1] == 5 and info[2] == 0 and info[3] == 1, info
    assert got == [_oracle(x, 0, 22) for x in items]
    # lgwin 16 selects another hasher family: one by one
    lib.compress_batch(items[:3], 5, 16)
    assert lib.last_batch_info()[:4] == [3, 0, 2, 1]


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. isolation: a chain that could see its neighbour would emit one long copy

def _isolation(lib, copies):
    a = synth.alice()
    items = [a[:20000]] * copies + [a[:19999]]
    for quality in (5, 8):
        _check(lib, items, quality, 22)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"), 8)


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"), 64)


# ---- 3. identity set

_IDENTITY_CASES = [(q, w, 0) for q in (5, 6, 7, 8) for w in (22, 24, 17)] + [(5, 22, 1), (5, 22, 2), (5, 22, 6)]


@functools.lru_cache(maxsize=None)
def _identity_items(with_long_items):
    a = synth.alice()
    items = test_batch._identity_items(reduced=True) + [a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, BLOCK - 1, BLOCK)]
    if not with_long_items:  # (the emulation runs a long item through the whole speculative one-shot path: one of them will do)
        items = [x for x in items if len(x) <= BLOCK] + [a[:BLOCK + 1]]
    return tuple(items)


@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_emu(quality, lgwin, mode):
    _check(test_cabi._load("emu"), list(_identity_items(False)), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_gpu(quality, lgwin, mode):
    _check(test_cabi._load("gpu"), list(_identity_items(True)), quality, lgwin, mode)


# ---- 4. seeded set: stored meta-blocks (should_compress and the size fallback), static-dictionary matches, the throttle

@pytest.mark.parametrize("quality", [5, 6, 7, 8])
def test_seeded_emu(quality):
    _check(test_cabi._load("emu"), list(_seeded()[:200]), quality, 22)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [5, 6, 7, 8])
def test_seeded_gpu(quality):
    _check(test_cabi._load("gpu"), list(_seeded()), quality, 22)


# ---- 5. table and group reuse: two tables, groups of 50 items (settings are read once per process: one child per setting)

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch, test_cabi
lib = test_cabi._load(%r)
items = test_batch._seeded_items(1024, 100, 65536, 11)[:%d]
h = hashlib.sha256()
groups = []
for q in (5, 8):
    for out in lib.compress_batch(items, q, 22):
        h.update(len(out).to_bytes(8, "little") + out)
    groups.append(lib.last_batch_info()[4])
print("digest", h.hexdigest(), "groups", groups)
"""


def _reuse(which, count):
    h = hashlib.sha256()
    for q in (5, 8):
        for x in _seeded()[:count]:
            out = _oracle(x, q, 22)
            h.update(len(out).to_bytes(8, "little") + out)
    for settings, groups in (({"BROTLI_MI355X_BATCH_TABLES": "2", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"}, (count + 49) // 50), ({}, 1)):
        env = dict(os.environ)
        for name in ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES"):
            env.pop(name, None)
        env.update(settings)
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which, count)], env=env, capture_output=True, text=True, timeout=600)
        want = "digest %s groups %s" % (h.hexdigest(), [groups, groups])
        assert r.returncode == 0 and want in r.stdout, (settings, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu", 120)


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu", 300)


# ---- 6. permutation

def _permutation(lib):
    a = synth.alice()
    items = [x for x in test_batch._identity_items(reduced=True) if len(x) <= BLOCK] + [synth.markov_text(n, n) for n in (200, 900, 5000, 60000)] + [a[:BLOCK + 1]]
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    for quality in (5, 7):
        straight = lib.compress_batch(items, quality, 22)
        shuffled = lib.compress_batch([items[i] for i in order], quality, 22)
        assert lib.last_batch_info()[1] == len(items) - 2  # (all but the empty and the long item)
        assert shuffled == [straight[i] for i in order]
        assert straight == [_oracle(x, quality, 22) for x in items]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# ---- 7. ABI semantics on the new path: the body of test_batch.test_abi_semantics_emu at quality 5

def _abi_semantics(lib, quality=5):
    _raw_batch, _raw_one = test_batch._raw_batch, test_batch._raw_one
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes = _raw_batch(lib, quality, 22, items, roomy)
    assert ret == 1 and results == [1] * len(items)
    assert lib.last_batch_info()[:4] == [5, 4, 0, 1]
    for x, cap, out in zip(items, roomy, outs):
        assert (1, out) == _raw_one(lib, quality, 22, x, cap)
    # a buffer too small for item k fails k alone (capacity 0 included), and the call returns 0
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000)):
        caps = list(roomy)
        caps[k] = cap
        assert _raw_one(lib, quality, 22, items[k], cap)[0] == 0
        ret, got, results, sizes = _raw_batch(lib, quality, 22, items, caps)
        assert ret == 0
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
    assert _raw_batch(lib, quality, 22, [], [])[0] == 1
    ret, got, _, _ = _raw_batch(lib, quality, 22, items, roomy, with_results=False)
    assert ret == 1 and got == outs
    # an incompressible item of one input block in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    noise = synth.random_bytes(60000)
    cap = max_size(len(noise))
    ok, want = _raw_one(lib, quality, 22, noise, cap)
    ret, got, results, _ = _raw_batch(lib, quality, 22, [b"abc", noise], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want
    assert lib.last_batch_info()[1] == 2
    assert orc.decompress(want, len(noise)) == noise


def test_abi_semantics_emu():
    _abi_semantics(test_cabi._load("emu"))


@pytest.mark.gpu
def test_abi_semantics_gpu():
    _abi_semantics(test_cabi._load("gpu"))


# ---- 8. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

def test_failed_call_frees_its_blocks_emu():
    import ctypes
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    items = [synth.alice()[:20000], b"tiny", synth.markov_text(60000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch(items, 5, 22))
        assert lib.last_batch_info()[:5] == [4, 4, 0, 0, 1]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 9. threads: four threads, each with a batch of its own

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    batches = [list(_seeded()[256 * t:256 * (t + 1)]) for t in range(4)]
    want = [[_oracle(x, 5, 22) for x in b] for b in batches]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 5, 22)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i[:4] == [256, 256, 0, 0] for i in infos), infos
