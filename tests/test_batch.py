"""BrotliMi355xCompressBatch / Library.compress_batch: many inputs in one call, each a complete stream of its own.

Item i of a batch is exactly what BrotliEncoderCompress gives on the same bytes (the oracle's stream), whatever the other items are,
however the plan cuts the batch into groups, and wherever a small fragment keeps its hash table (device memory or workgroup memory,
BROTLI_MI355X_BATCH_LDS_BITS).  The CPU tests run the emulation library -- the same host plan and the same item code -- the GPU tests
the product library."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
from ctypes import POINTER, byref, c_char_p, c_int32, c_size_t, c_void_p

import pytest

import orc
import synth
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(HERE, "golden", "small")


def _golden_small():
    return [open(os.path.join(SMALL, name), "rb").read() for name in sorted(os.listdir(SMALL))]


def _identity_items(reduced):
    zeros, rnd = (30000, 20000) if reduced else (300000, 200000)
    return ([b"", b"a", b"abc", bytes(range(15)), bytes(range(16))] + _golden_small() +
            [synth.alice(), bytes(zeros), synth.random_bytes(rnd)])


def _check(lib, items, quality, lgwin):
    got = lib.compress_batch(items, quality, lgwin)
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == orc.compress(item, quality, lgwin), (quality, lgwin, i, len(item))
        assert orc.decompress(g, len(item)) == item, (quality, lgwin, i, len(item))
    return got


def _identity(lib, reduced):
    items = _identity_items(reduced)
    for quality in (0, 1):
        for lgwin in (22, 18, 16, 10):
            _check(lib, items, quality, lgwin)
        # two fragments of one stream among single-fragment streams
        two = synth.markov_text((3 << 18) if reduced else (3 << 19), 4)
        _check(lib, [b"xyz", two, synth.alice()[:3000]], quality, 19 if reduced else 20)


def test_identity_emu():
    _identity(test_cabi._load("emu"), reduced=False)


# what _SIDE_BY_SIDE_CHILD of test_quality_0_1.py feeds one call at a time, as the items of one batch: text, random bytes and zeros
# in pieces of all sizes, so that stored and compressed meta-blocks alternate and fragments start at every bit phase
_SWEEP_CHILD = """
import random, sys
sys.path.insert(0, %r)
import orc, synth, test_cabi
lib = test_cabi._load(%r)
rng = random.Random(%d)
text, rnd = synth.markov_text(1 << 20, 3), synth.random_bytes(1 << 20)
items = []
for it in range(%d):
    parts, total = [], rng.choice([0, 40, 700, 3000, 20000, 100000, 200000])
    while sum(map(len, parts)) < total:
        k, ln = rng.choice([0, 0, 1, 1, 2]), rng.choice([1, 7, 100, 900, 1024, 1500, 5000, 40000, 140000])
        off = rng.randrange(0, (1 << 20) - ln)
        parts.append(text[off:off + ln] if k == 0 else (rnd[off:off + ln] if k == 1 else bytes(ln)))
    items.append(b"".join(parts)[:total + (rng.randrange(0, 50) if total else 0)])
for w in %r:
    for q in (0, 1):
        got = lib.compress_batch(items, q, w)
        assert len(got) == len(items)
        for i, (g, d) in enumerate(zip(got, items)):
            assert g == orc.compress(d, q, w), (i, q, w, len(d))
print("ok")
"""


def _sweep(which, seed, count, lgwins, **env):
    env = dict(os.environ, BROTLI_MI355X_SELFTEST="1", **env)
    r = subprocess.run([sys.executable, "-c", _SWEEP_CHILD % (HERE, which, seed, count, tuple(lgwins))], env=env, capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_seeded_sweep_emu():
    _sweep("emu", 21, 300, (10, 16, 18))


def test_groups_emu():
    # groups of at most 200 000 bytes of input and 300 000 bytes of scratch: several groups, items that span groups (a 200 KB item
    # at lgwin 16 is four fragments, a group holds three), groups that end one stream and begin the next
    _sweep("emu", 21, 300, (16, 18), BROTLI_MI355X_FRAGMENT_BATCH="200000", BROTLI_MI355X_FRAGMENT_SCRATCH="300000")


def test_again_path_emu():
    # every fragment off phase 0 is compressed again by itself, where it sat in the batch (its slabs or its workgroup table)
    _sweep("emu", 22, 80, (16, 18), BROTLI_MI355X_TEST_FRAGMENT_AGAIN="1")


def test_permutation_emu():
    lib = test_cabi._load("emu")
    items = _identity_items(reduced=True) + [synth.markov_text(n, n) for n in (200, 900, 5000, 70000)]
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    for quality in (0, 1):
        straight = lib.compress_batch(items, quality, 16)
        shuffled = lib.compress_batch([items[i] for i in order], quality, 16)
        assert shuffled == [straight[i] for i in order]


def _raw_batch(lib, quality, lgwin, items, caps, with_results=True):
    """BrotliMi355xCompressBatch through ctypes: (return value, [bytes or None], [item result])"""
    n = len(items)
    bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
    inputs = (c_char_p * max(1, n))(*items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatch(quality, lgwin, 0, n, inputs, in_sizes, outputs, out_sizes,
                                            results if with_results else ctypes.cast(None, POINTER(c_int32)))
    return ret, [bufs[i].raw[:out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n]


def _raw_one(lib, quality, lgwin, item, cap):
    buf = ctypes.create_string_buffer(max(1, cap))
    n = c_size_t(cap)
    ok = lib.lib.BrotliEncoderCompress(quality, lgwin, 0, len(item), item, byref(n), buf)
    return ok, (buf.raw[:n.value] if ok else b"")


@pytest.mark.parametrize("quality", [0, 1, 5])
def test_abi_semantics_emu(quality):
    lib = test_cabi._load("emu")
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    roomy = [max_size(len(x)) + 16 for x in items]
    # every item as the one-shot call gives it
    ret, outs, results, sizes = _raw_batch(lib, quality, 22, items, roomy)
    assert ret == 1 and results == [1] * len(items)
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
    # count == 0
    assert _raw_batch(lib, quality, 22, [], [])[0] == 1
    # item_results == NULL
    ret, got, _, _ = _raw_batch(lib, quality, 22, items, roomy, with_results=False)
    assert ret == 1 and got == outs
    # an incompressible item in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    noise = synth.random_bytes(70000)
    cap = max_size(len(noise))
    ok, want = _raw_one(lib, quality, 22, noise, cap)
    ret, got, results, _ = _raw_batch(lib, quality, 22, [b"abc", noise], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want
    assert orc.decompress(want, len(noise)) == noise


def test_another_quality_emu():
    lib = test_cabi._load("emu")
    items = [synth.alice()[:20000], b"", synth.markov_text(3000, 2)]
    assert lib.compress_batch(items, 5, 22) == [lib.compress(x, 5, 22) for x in items]


@pytest.mark.parametrize("quality", [0, 1, 5])
def test_failed_batch_call_frees_its_blocks(quality):
    # (quality 5: the items run one by one through the one-shot path, and a device error in one of them fails the call as a whole)
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib  # (the same shared object as every other binding of the emulation library: one set of counters)
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    items = [synth.alice()[:20000], b"tiny", synth.markov_text(70000, 3), synth.random_bytes(3000)]  # (lgwin 16: the third is two fragments)
    test_device_memory.sweep(L, lambda: b"|".join(lib.compress_batch(items, quality, 16)), exc)


# ---- GPU: the product library

def _seeded_items(count, lo, hi, seed):
    rng = random.Random(seed)
    text, rnd = synth.markov_text(1 << 20, 3), synth.random_bytes(1 << 20)
    items = []
    for _ in range(count):
        n = int(lo * (hi / lo) ** rng.random())
        kind = rng.choice([0, 0, 0, 1, 2, 3])
        off = rng.randrange(0, (1 << 20) - n)
        if kind == 0:
            items.append(text[off:off + n])
        elif kind == 1:
            items.append(rnd[off:off + n])
        elif kind == 2:
            items.append(text[off:off + n // 2] + rnd[off:off + n - n // 2])
        else:
            items.append(bytes(n // 3) + text[off:off + n - n // 3])
    return items


@pytest.mark.gpu
def test_identity_gpu():
    _identity(test_cabi._load("gpu"), reduced=True)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [0, 1])
def test_4096_items_gpu(quality):
    lib = test_cabi._load("gpu")
    items = _seeded_items(4096, 200, 64 << 10, 7)
    got = lib.compress_batch(items, quality, 22)
    for i, (g, x) in enumerate(zip(got, items)):
        assert g == orc.compress(x, quality, 22), (quality, i, len(x))


@pytest.mark.gpu
def test_64_alice_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    for quality in (0, 1):
        assert lib.compress_batch([a] * 64, quality, 22) == [orc.compress(a, quality, 22)] * 64


_LDS_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch, test_cabi
lib = test_cabi._load(%r)
items = test_batch._seeded_items(1500, 100, 40000, 3)
h = hashlib.sha256()
for q in (0, 1):
    for out in lib.compress_batch(items, q, 22):
        h.update(len(out).to_bytes(8, "little") + out)
print("digest", h.hexdigest())
"""


def _lds_switch(which):
    """the table's home is one setting per process, read once: one child per value, the same bytes from both (and the oracle's)"""
    items = _seeded_items(1500, 100, 40000, 3)
    h = hashlib.sha256()
    for q in (0, 1):
        for x in items:
            out = orc.compress(x, q, 22)
            h.update(len(out).to_bytes(8, "little") + out)
    for value in ("0", None, "9"):
        env = dict(os.environ)
        env.pop("BROTLI_MI355X_BATCH_LDS_BITS", None)
        if value is not None:
            env["BROTLI_MI355X_BATCH_LDS_BITS"] = value
        r = subprocess.run([sys.executable, "-c", _LDS_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "digest " + h.hexdigest() in r.stdout, (value, r.stdout[-2000:] + r.stderr[-3000:])


def test_lds_switch_emu():
    _lds_switch("emu")


@pytest.mark.gpu
def test_lds_switch_gpu():
    _lds_switch("gpu")


@pytest.mark.parametrize("quality", [0, 5])
def test_device_error_fails_the_whole_call_emu(quality):
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    items = [synth.alice()[:5000], synth.markov_text(3000, 2), synth.alice()[:7000]]
    caps = [L.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    assert _raw_batch(lib, quality, 22, items, caps)[0] == 1  # warm: what a process allocates once is there afterwards
    before = L.brotli_emu_alloc_count()
    assert _raw_batch(lib, quality, 22, items, caps)[0] == 1
    n = L.brotli_emu_alloc_count() - before
    try:
        L.brotli_emu_fail_alloc(n)  # the last allocation of the call: at quality 5 the first items are done by then
        ret, _, results, sizes = _raw_batch(lib, quality, 22, items, caps)
    finally:
        L.brotli_emu_fail_alloc(0)
    assert ret == 0 and results == [0, 0, 0] and sizes == [0, 0, 0]
    assert "BrotliMi355xCompressBatch" in lib.last_error()
