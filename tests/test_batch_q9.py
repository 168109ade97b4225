"""BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_Q9_ITEMS (128): at qualities 9 and 10 and lgwin 17 .. 24 the items of
at most one input block run side by side on the device, one live chain each on a private H9 table (32 768 keys, rings 256 deep),
and leave one meta-block (batch_greedy.h: BatchQ9Compress, k_parse_batch_h9); every other item goes one by one in the same call.
Quality 10 goes as quality 9, as BrotliEncoderCompress runs it.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken, so a silent fall-back to the one-by-one path fails a test.  The CPU tests run the emulation library --
the same host plan and the same item code -- the GPU tests the product library.  Where the library does not know the route every
call with the bit returns 0, and every test here fails.

GPU shapes.  A chain is one wavefront and takes a lone chain's time for its item -- measured on an MI355X: about 1.07 us per byte
of text, 0.14 s for the 131 072 bytes of the edge at lgwin 17 -- so the GPU variants keep to items of a few kilobytes except for
that edge, which runs there as on the emulation; the 262 144-byte edge at lgwin 18 is emulation only."""
import functools
import hashlib
import os
import subprocess
import sys
import threading

import pytest

import orc
import synth
import test_batch
import test_batch_dictionary_quick
import test_batch_long
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LONG, QUICK, QUICK_LONG, ZOPFLI, Q9 = 1, 4, 16, 32, 128  # BROTLI_MI355X_BATCH_ROUTE_*_ITEMS
ALL = LONG | QUICK | QUICK_LONG | ZOPFLI | Q9


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


def _cap(lgwin):
    """the largest item the route takes: one input block"""
    return 0 if lgwin < 17 or lgwin > 24 else 1 << min(18, lgwin)


def _side(items, quality, lgwin):
    """how many of the items the route takes side by side"""
    return sum(1 for x in items if 0 < len(x) <= _cap(lgwin)) if quality in (9, 10) else 0


def _check(lib, items, quality, lgwin, mode=0):
    got = lib.compress_batch(items, quality, lgwin, mode, q9_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    side = _side(items, quality, lgwin)
    assert info[:4] == [len(items), side, len(items) - side - empty, empty] and info[5:] == [0, 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side

def _taken_side_by_side(lib):
    a = synth.alice()
    rnd = synth.random_bytes(3000)
    items = [b"", b"x", a[:5000], a[:16384], rnd]
    n = len(items)
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    assert len(_oracle(rnd, 9, 22)) == 3004  # (the random item closes as a stored meta-block)
    for quality in (9, 10):
        want = [_oracle(x, quality, 22) for x in items]
        assert want == [_oracle(x, 9, 22) for x in items]
        ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, Q9, items, caps)
        info = lib.last_batch_info()
        assert ret == 1 and results == [1] * n, (quality, lib.last_error())
        assert outs == want
        assert info[:4] == [5, 4, 0, 1] and info[4] >= 1 and info[5:] == [0, 0, 0], (quality, info)
        assert lib.compress_batch(items, quality, 22, q9_items=True) == want
        assert lib.last_batch_info() == info
        # every bit together: the other routes take nothing at these qualities
        ret, outs, _, _ = test_batch_long._raw_ex(lib, quality, 22, ALL, items, caps)
        assert ret == 1 and outs == want and lib.last_batch_info() == info
        assert lib.compress_batch(items, quality, 22, long_items=True, quick_items=True, quick_long_items=True, zopfli_items=True, q9_items=True) == want
        assert lib.last_batch_info() == info
        # routes 0, 1, 4, 16, 32 and the plain call: nothing side by side, the same bytes
        for routes in (0, LONG, QUICK, QUICK_LONG, ZOPFLI):
            ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, routes, items, caps)
            assert ret == 1 and outs == want
            assert lib.last_batch_info() == [n, 0, n - 1, 1, 0, 0, 0, 0], (quality, routes)
        assert lib.compress_batch(items, quality, 22) == want
        assert lib.last_batch_info() == [n, 0, n - 1, 1, 0, 0, 0, 0]
    # the bit changes nothing at qualities 5, 8 and 11
    small = [b"", b"x", a[:5000], a[:8192], rnd]
    for quality in (5, 8, 11):
        want = [_oracle(x, quality, 22) for x in small]
        assert lib.compress_batch(small, quality, 22) == want
        plain = lib.last_batch_info()
        assert lib.compress_batch(small, quality, 22, q9_items=True) == want
        assert lib.last_batch_info() == plain
    # ... and with it quality 11 + ZOPFLI still goes the Zopfli way
    want = [_oracle(x, 11, 22) for x in small]
    assert lib.compress_batch(small, 11, 22, zopfli_items=True) == want
    zopfli = lib.last_batch_info()
    assert zopfli[:4] == [5, 4, 0, 1] and zopfli[4] >= 1
    assert lib.compress_batch(small, 11, 22, zopfli_items=True, q9_items=True) == want
    assert lib.last_batch_info() == zopfli
    # a route this build does not know fails the whole call, and only info[0] is set
    for routes in (2, 8, 64, Q9 | 2, 256, 1 << 31):
        ret, outs, results, sizes = test_batch_long._raw_ex(lib, 9, 22, routes, items, caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert lib.last_batch_info() == [5, 0, 0, 0, 0, 0, 0, 0]
        assert "route" in lib.last_error()
    assert type(lib).BATCH_ROUTE_Q9_ITEMS == 128
    with pytest.raises(ValueError):
        lib.compress_batch(items, 9, 22, dictionary=b"some dictionary", q9_items=True)
    # not combined with a dictionary: the dictionary call does not know the bit
    dcaps = [c + 1024 for c in caps]
    ret, outs, results, sizes = test_batch_dictionary_quick._raw(lib, 9, 22, Q9, b"some dictionary", items, dcaps)
    assert ret == 0 and results == [0] * 5 and sizes == [0] * 5
    assert lib.last_batch_info() == [5, 0, 0, 0, 0, 0, 0, 0]
    assert "route" in lib.last_error()


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"))


# ---- 2. eligibility edges: one input block is 1 << 17 bytes at lgwin 17 and 1 << 18 from lgwin 18 on; lgwin <= 16 is another hasher

def _repeated(n):
    a = synth.alice()
    return (a * (n // len(a) + 1))[:n]


def _eligibility_edges(lib, gpu):
    a = synth.alice()
    items = [_repeated((1 << 17) - 1), _repeated(1 << 17), _repeated((1 << 17) + 1)]
    for quality in (9, 10):
        _check(lib, items, quality, 17)
        assert lib.last_batch_info()[:4] == [3, 2, 1, 0]
    if not gpu:
        _check(lib, [_repeated(1 << 18), _repeated((1 << 18) + 1)], 9, 18)
        assert lib.last_batch_info()[:4] == [2, 1, 1, 0]
    small = [a[:3000], b"x", a[100:1700]]
    for lgwin in (16, 10):
        _check(lib, small, 9, lgwin)
        assert lib.last_batch_info() == [3, 0, 3, 0, 0, 0, 0, 0]
    for mode in (1, 2):  # BROTLI_MODE_TEXT, BROTLI_MODE_FONT
        for quality in (9, 10):
            _check(lib, small, quality, 22, mode)
            assert lib.last_batch_info()[:4] == [3, 3, 0, 0]


def test_eligibility_edges_emu():
    _eligibility_edges(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_eligibility_edges_gpu():
    _eligibility_edges(test_cabi._load("gpu"), True)


# ---- 3. ring depth and counter wrap: the smallest shapes at which an H9 ring can go wrong

def _ring_depth(lib):
    a = synth.alice()
    zeros = bytes(70000)  # one key filed more than 65 536 times: the u16 counter wraps, the 256-slot ring hundreds of times
    assert len(_oracle(zeros, 9, 17)) == 13 and len(_oracle(zeros, 9, 22)) == 13
    assert _oracle(zeros, 10, 22) == _oracle(zeros, 9, 22)
    assert len(_oracle(b"ab" * 4000, 9, 22)) == 14
    items = [zeros, b"ab" * 4000, a[:300] * 40]  # (the last: many keys past depth 256 with real matches)
    for quality, lgwin in ((9, 17), (9, 22), (10, 22)):
        _check(lib, items, quality, lgwin)
        assert lib.last_batch_info()[:4] == [3, 3, 0, 0]
    # the htl edges of the tail
    short = [a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)]
    _check(lib, short, 9, 22)
    assert lib.last_batch_info()[:4] == [11, 11, 0, 0]


def test_ring_depth_emu():
    _ring_depth(test_cabi._load("emu"))


@pytest.mark.gpu
def test_ring_depth_gpu():
    _ring_depth(test_cabi._load("gpu"))


# ---- 4. isolation: a chain that saw its neighbour's text or ring would emit one long copy

def _isolation(lib, copies):
    a = synth.alice()
    items = [a[:3000]] * copies + [a[:2999]]
    for quality in (9, 10):
        _check(lib, items, quality, 22)
        assert lib.last_batch_info()[1] == copies + 1


def test_isolation_emu():
    _isolation(test_cabi._load("emu"), 8)


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"), 64)


# ---- 5. table and group reuse: one table, then two, groups of 50 items (settings are read once per process: one child per
# setting).  A run of zeros leaves one key's counter far past the ring depth and 256 stale slots; the item that comes next on that
# table must see its own filings only.

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_q9, test_cabi
lib = test_cabi._load(%r)
items = test_batch_q9._reuse_items()
h = hashlib.sha256()
for out in lib.compress_batch(items, 9, 22, q9_items=True):
    h.update(len(out).to_bytes(8, "little") + out)
print("digest", h.hexdigest(), "info", lib.last_batch_info())
"""


def _reuse_items():
    a = synth.alice()
    rnd = synth.random_bytes(2000 + 40)
    items = []
    for i in range(40):
        items += [bytes(5000), a[i * 37:i * 37 + 4000], rnd[i:i + 2000]]
    assert len(items) == 120
    return items


def _reuse(which):
    h = hashlib.sha256()
    for x in _reuse_items():
        out = _oracle(x, 9, 22)
        h.update(len(out).to_bytes(8, "little") + out)
    for tables in ("1", "2"):
        env = dict(os.environ)
        for name in ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES"):
            env.pop(name, None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        want = "digest %s info %s" % (h.hexdigest(), [120, 120, 0, 0, 3, 0, 0, 0])
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 6. an item that fails alone: capacities too small for item 1 of 4

def _fails_alone(lib):
    a = synth.alice()
    items = [a[:3000], a[500:4500], synth.random_bytes(2000), b"q" * 700]
    roomy = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    for quality in (9, 10):
        want = [_oracle(x, quality, 22) for x in items]
        caps = list(roomy)
        caps[1] = len(want[1]) - 1
        assert test_batch._raw_one(lib, quality, 22, items[1], caps[1])[0] == 0
        ret, got, results, sizes = test_batch_long._raw_ex(lib, quality, 22, Q9, items, caps)
        assert ret == 0 and results == [1, 0, 1, 1] and sizes[1] == 0
        assert [g for i, g in enumerate(got) if i != 1] == [w for i, w in enumerate(want) if i != 1]
        assert lib.last_batch_info() == [4, 4, 0, 0, 1, 0, 0, 0]  # (it ran side by side and has its answer)


def test_fails_alone_emu():
    _fails_alone(test_cabi._load("emu"))


@pytest.mark.gpu
def test_fails_alone_gpu():
    _fails_alone(test_cabi._load("gpu"))


# ---- 7. threads: four threads, each with one call of 64 slices of 2 KiB

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[997 * t + 131 * i:997 * t + 131 * i + 2048] for i in range(64)] for t in range(4)]
    want = [[_oracle(x, 9, 22) for x in batches[t]] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 9, 22, q9_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i == [64, 64, 0, 0, 1, 0, 0, 0] for i in infos), infos
