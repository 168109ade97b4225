"""BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS: at qualities 2 to 4 the items of at most one input block
(16 384 bytes at quality 2 and 3, 65 536 at quality 4) run side by side on the device, one chain on a private BasicHasher table and
one meta-block each (batch_quick.h); every other item goes one by one in the same call.  routes == 0 and 1 take these qualities one
by one, as before.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken, so a silent fall-back to the one-by-one path fails a test.  The CPU tests run the emulation library --
the same host plan and the same item code -- the GPU tests the product library."""
import ctypes
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
import test_batch_long
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LONG, QUICK = 1, 4  # BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS, BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS


def _block(quality):
    return 16384 if quality < 4 else 65536  # one input block: lgblock 14 at quality 2 / 3, 16 at quality 4


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


@functools.lru_cache(maxsize=None)
def _seeded(block):
    return tuple(test_batch._seeded_items(1024, 100, block, 11))


def _check(lib, items, quality, lgwin, mode=0):
    got = lib.compress_batch(items, quality, lgwin, mode, quick_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    side = sum(1 for x in items if 0 < len(x) <= _block(quality))
    assert info[:4] == [len(items), side, len(items) - side - empty, empty] and info[5:] == [0, 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side (fails where the library does not know the route: the call returns 0)

def _taken_side_by_side(lib):
    a = synth.alice()
    items = [b"", b"x", a[:5000], a[:16384], a[:16385], a[:65536], a[:65537], synth.random_bytes(3000)]
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    for quality in (2, 3, 4):
        want = [_oracle(x, quality, 22) for x in items]
        ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, QUICK, items, caps)
        info = lib.last_batch_info()
        assert ret == 1 and results == [1] * 8, (quality, lib.last_error())
        assert info[:4] == ([8, 4, 3, 1] if quality < 4 else [8, 6, 1, 1]) and info[4] >= 1 and info[5:] == [0, 0, 0], (quality, info)
        assert outs == want
        assert lib.compress_batch(items, quality, 22, quick_items=True) == want
        assert lib.last_batch_info() == info
        # the two routes together: the long-items route takes nothing at these qualities
        assert lib.compress_batch(items, quality, 22, long_items=True, quick_items=True) == want
        assert lib.last_batch_info() == info
        # routes 0 and 1, and the plain call: nothing side by side, the same bytes
        for routes in (0, LONG):
            ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, routes, items, caps)
            assert ret == 1 and outs == want
            assert lib.last_batch_info() == [8, 0, 7, 1, 0, 0, 0, 0], (quality, routes)
        assert lib.compress_batch(items, quality, 22) == want
        assert lib.last_batch_info() == [8, 0, 7, 1, 0, 0, 0, 0]
    # the bit changes nothing at quality 5 ...
    want = [_oracle(x, 5, 22) for x in items]
    assert lib.compress_batch(items, 5, 22) == want
    plain = lib.last_batch_info()
    assert lib.compress_batch(items, 5, 22, quick_items=True) == want
    assert lib.last_batch_info() == plain
    # ... with the long-items route either
    assert lib.compress_batch(items, 5, 22, long_items=True) == want
    long_info = lib.last_batch_info()
    ret, outs, _, _ = test_batch_long._raw_ex(lib, 5, 22, LONG | QUICK, items, caps)
    assert ret == 1 and outs == want and lib.last_batch_info() == long_info
    # a route this build does not know fails the whole call, and only info[0] is set
    for routes in (2, 6, 8, 1 << 31):
        ret, outs, results, sizes = test_batch_long._raw_ex(lib, 2, 22, routes, items, caps)
        assert ret == 0 and results == [0] * 8 and sizes == [0] * 8, routes
        assert lib.last_batch_info() == [8, 0, 0, 0, 0, 0, 0, 0]
        assert "route" in lib.last_error()
    with pytest.raises(ValueError):
        lib.compress_batch(items, 2, 22, dictionary=b"some dictionary", quick_items=True)


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. isolation: a chain that could see its neighbour would emit one long copy

def _isolation(lib, copies):
    a = synth.alice()
    items = [a[:8000]] * copies + [a[:7999]]
    for quality in (2, 3, 4):
        _check(lib, items, quality, 22)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"), 8)


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"), 64)


# ---- 3. table reuse: one table, then two, groups of 50 items (settings are read once per process: one child per setting).  The
# items share content, so that a slot left by the item in front points at plausible text of the next one; a random item drives the
# static-dictionary throttle, and the text behind it must start with the books at 0 again.

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_quick, test_cabi
lib = test_cabi._load(%r)
items = test_batch_quick._reuse_items()
h = hashlib.sha256()
infos = []
for q in (2, 3, 4):
    for out in lib.compress_batch(items, q, 22, quick_items=True):
        h.update(len(out).to_bytes(8, "little") + out)
    infos.append(lib.last_batch_info())
print("digest", h.hexdigest(), "infos", infos)
"""


def _reuse_items():
    a = synth.alice()
    items = [a[37 * i:37 * i + 1500 + 13 * (i % 11)] for i in range(116)]
    # (largest first within a group: the random items run in front of shorter text)
    items[10:10] = [synth.random_bytes(3000), a[500:2900]]
    items[70:70] = [synth.random_bytes(3000), a[40000:42000]]
    assert len(items) == 120
    return items


def _reuse(which):
    items = _reuse_items()
    h = hashlib.sha256()
    for q in (2, 3, 4):
        for x in items:
            out = _oracle(x, q, 22)
            h.update(len(out).to_bytes(8, "little") + out)
    for tables in ("1", "2"):
        env = dict(os.environ)
        for name in ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES"):
            env.pop(name, None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        want = "digest %s infos %s" % (h.hexdigest(), [[120, 120, 0, 0, 3, 0, 0, 0]] * 3)
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 4. identity set

_IDENTITY_CASES = [(q, w, 0) for q in (2, 3, 4) for w in (10, 14, 16, 17, 22, 24)] + [(4, 22, 1), (4, 22, 2), (4, 22, 6), (2, 22, 2), (3, 22, 6)]


@functools.lru_cache(maxsize=None)
def _identity_items(block, with_long_item):
    a = synth.alice()
    items = [x[:block] for x in test_batch._identity_items(reduced=True)]
    # 1 .. 8: no search at all; 9: the first search; 33 and above: both sweep offsets at H3, all four at H4
    items += [a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, block - 1, block)]
    # copies of 16 and more go through the quad branch of StoreRange; both literal-spree step sizes and a stored meta-block
    items += [b"ab" * 40, bytes(300), synth.random_bytes(3000)]
    if with_long_item:
        items.append(a[:block + 1])  # one by one
    return tuple(items)


@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_emu(quality, lgwin, mode):
    _check(test_cabi._load("emu"), list(_identity_items(_block(quality), False)), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _IDENTITY_CASES)
def test_identity_gpu(quality, lgwin, mode):
    _check(test_cabi._load("gpu"), list(_identity_items(_block(quality), True)), quality, lgwin, mode)


# ---- 5. seeded set: stored meta-blocks (should_compress and the size fallback), static-dictionary matches, zero runs

@pytest.mark.parametrize("quality", [2, 3, 4])
def test_seeded_emu(quality):
    _check(test_cabi._load("emu"), list(_seeded(_block(quality))[:200]), quality, 22)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [2, 3, 4])
def test_seeded_gpu(quality):
    _check(test_cabi._load("gpu"), list(_seeded(_block(quality))), quality, 22)


# ---- 6. permutation

def _permutation(lib):
    a = synth.alice()
    for quality in (2, 3, 4):
        block = _block(quality)
        items = [x[:block] for x in test_batch._identity_items(reduced=True)] + [synth.markov_text(n, n) for n in (200, 900, 5000, block - 3)] + [a[:block + 1]]
        order = list(range(len(items)))
        random.Random(5).shuffle(order)
        straight = lib.compress_batch(items, quality, 22, quick_items=True)
        info = lib.last_batch_info()
        shuffled = lib.compress_batch([items[i] for i in order], quality, 22, quick_items=True)
        assert lib.last_batch_info() == info and info[:4] == [len(items), len(items) - 2, 1, 1] and info[5:] == [0, 0, 0], info
        assert shuffled == [straight[i] for i in order]
        assert straight == [_oracle(x, quality, 22) for x in items]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# ---- 7. ABI semantics on the new route

def _abi_semantics(lib, quality):
    _raw_ex, _raw_one = test_batch_long._raw_ex, test_batch._raw_one
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes = _raw_ex(lib, quality, 22, QUICK, items, roomy)
    assert ret == 1 and results == [1] * len(items)
    assert lib.last_batch_info() == [5, 4, 0, 1, 1, 0, 0, 0]
    for x, cap, out in zip(items, roomy, outs):
        assert (1, out) == _raw_one(lib, quality, 22, x, cap)
        assert out == _oracle(x, quality, 22)
    # a buffer too small for item k fails k alone (capacity 0 included), and the call returns 0
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000)):
        caps = list(roomy)
        caps[k] = cap
        assert _raw_one(lib, quality, 22, items[k], cap)[0] == 0
        ret, got, results, sizes = _raw_ex(lib, quality, 22, QUICK, items, caps)
        assert ret == 0
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
    assert _raw_ex(lib, quality, 22, QUICK, [], [])[0] == 1
    ret, got, _, _ = _raw_ex(lib, quality, 22, QUICK, items, roomy, with_results=False)
    assert ret == 1 and got == outs
    # an incompressible item of one input block in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    noise = synth.random_bytes(_block(quality))
    cap = max_size(len(noise))
    ok, want = _raw_one(lib, quality, 22, noise, cap)
    ret, got, results, _ = _raw_ex(lib, quality, 22, QUICK, [b"abc", noise], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want
    assert lib.last_batch_info()[1] == 2
    assert orc.decompress(want, len(noise)) == noise


@pytest.mark.parametrize("quality", [2, 4])
def test_abi_semantics_emu(quality):
    _abi_semantics(test_cabi._load("emu"), quality)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [2, 4])
def test_abi_semantics_gpu(quality):
    _abi_semantics(test_cabi._load("gpu"), quality)


# ---- 8. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

def test_failed_call_frees_its_blocks_emu():
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    items = [synth.alice()[:12000], b"tiny", synth.markov_text(16000, 3), synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch(items, 3, 22, quick_items=True))
        assert lib.last_batch_info()[:5] == [4, 4, 0, 0, 1]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 9. threads: four threads, each with a routed batch of its own

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    quality = [2, 4, 2, 4]
    batches = [list(_seeded(_block(quality[t]))[256 * t:256 * (t + 1)]) for t in range(4)]
    want = [[_oracle(x, quality[t], 22) for x in batches[t]] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], quality[t], 22, quick_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i[:4] == [256, 256, 0, 0] and i[5:] == [0, 0, 0] for i in infos), infos
