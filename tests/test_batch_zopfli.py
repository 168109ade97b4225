"""BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_ZOPFLI_ITEMS (32): at quality 11 the items of at most 65 536 bytes run
side by side on the device, one wavefront each that walks the item the reference's way on H10 trees of its own, and leave one
meta-block (batch_zopfli.h); every other item goes one by one in the same call.  Routes 0, 1, 4 and 16 take this quality one by
one, as before.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken, so a silent fall-back to the one-by-one path fails a test.  The CPU tests run the emulation library --
the same host plan and the same item code -- the GPU tests the product library.

Quality 10.  Every check runs at quality 10 as well, against orc.compress(item, 10, ...) like everywhere.  BrotliEncoderCompress
runs quality 10 at quality 9 (encode.rs:1468-1481; test_cabi pins compress(a, 10, 22) == orc.compress(a, 9, 22): the stream is
byte for byte that of plain quality 9) -- so the stream the call owes an item of quality 10 is not the one a Zopfli walk
gives, and the route cannot take such items without changing their bytes.  They go one by one with the bit set; the tests assert
exactly that (`_side`), together with the bytes."""
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
import test_batch_long
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LONG, QUICK, QUICK_LONG, ZOPFLI = 1, 4, 16, 32  # BROTLI_MI355X_BATCH_ROUTE_*_ITEMS
CAP = 65536  # the largest item the route takes


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


def _side(items, quality):
    """how many of the items the route takes side by side"""
    return sum(1 for x in items if 0 < len(x) <= CAP) if quality == 11 else 0


def _check(lib, items, quality, lgwin, mode=0):
    got = lib.compress_batch(items, quality, lgwin, mode, zopfli_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    side = _side(items, quality)
    assert info[:4] == [len(items), side, len(items) - side - empty, empty] and info[5:] == [0, 0, 0], info
    assert (info[4] >= 1) == (side > 0), info
    return got


# ---- 1. taken side by side (fails where the library does not know the route: the call returns 0)

def _taken_side_by_side(lib, gpu):
    a = synth.alice()
    cases = {10: [b"", b"x", a[:5000], a[:65536], a[:65537], synth.random_bytes(3000)],
             11: [b"", b"x", a[:5000], a[:65536], a[:65537], synth.random_bytes(3000)]}
    if gpu:  # (one chain of 64 KiB at quality 11 lasts seconds: the cap itself is covered by the emulation)
        cases[11] = [b"", b"x", a[:5000], a[:8192], synth.random_bytes(3000)]
    for quality, items in cases.items():
        n = len(items)
        caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
        want = [_oracle(x, quality, 22) for x in items]
        side = _side([x for x in items], quality)
        one_by_one = n - 1 - side
        ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, ZOPFLI, items, caps)
        info = lib.last_batch_info()
        assert ret == 1 and results == [1] * n, (quality, lib.last_error())
        assert outs == want
        assert info[:4] == [n, side, one_by_one, 1] and info[5:] == [0, 0, 0], (quality, info)
        if quality == 11:
            assert info[:4] == ([6, 4, 1, 1] if not gpu else [5, 4, 0, 1]) and info[4] >= 1, info
        assert lib.compress_batch(items, quality, 22, zopfli_items=True) == want
        assert lib.last_batch_info() == info
        # every bit together: the other routes take nothing at these qualities
        ret, outs, _, _ = test_batch_long._raw_ex(lib, quality, 22, LONG | QUICK | QUICK_LONG | ZOPFLI, items, caps)
        assert ret == 1 and outs == want and lib.last_batch_info() == info
        assert lib.compress_batch(items, quality, 22, long_items=True, quick_items=True, quick_long_items=True, zopfli_items=True) == want
        assert lib.last_batch_info() == info
        # routes 0, 1, 4, 16 and the plain call: nothing side by side, the same bytes
        for routes in (0, LONG, QUICK, QUICK_LONG):
            ret, outs, results, _ = test_batch_long._raw_ex(lib, quality, 22, routes, items, caps)
            assert ret == 1 and outs == want
            assert lib.last_batch_info() == [n, 0, n - 1, 1, 0, 0, 0, 0], (quality, routes)
        assert lib.compress_batch(items, quality, 22) == want
        assert lib.last_batch_info() == [n, 0, n - 1, 1, 0, 0, 0, 0]
    # the bit changes nothing at quality 5 and at quality 9
    items = [b"", b"x", a[:5000], a[:8192], synth.random_bytes(3000)]
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    for quality in (5, 9):
        want = [_oracle(x, quality, 22) for x in items]
        assert lib.compress_batch(items, quality, 22) == want
        plain = lib.last_batch_info()
        assert lib.compress_batch(items, quality, 22, zopfli_items=True) == want
        assert lib.last_batch_info() == plain
    # a route this build does not know fails the whole call, and only info[0] is set
    for routes in (2, 8, 64, ZOPFLI | 2, 1 << 31):
        ret, outs, results, sizes = test_batch_long._raw_ex(lib, 11, 22, routes, items, caps)
        assert ret == 0 and results == [0] * 5 and sizes == [0] * 5, routes
        assert lib.last_batch_info() == [5, 0, 0, 0, 0, 0, 0, 0]
        assert "route" in lib.last_error()
    assert type(lib).BATCH_ROUTE_ZOPFLI_ITEMS == 32
    with pytest.raises(ValueError):
        lib.compress_batch(items, 11, 22, dictionary=b"some dictionary", zopfli_items=True)


def test_taken_side_by_side_emu():
    _taken_side_by_side(test_cabi._load("emu"), False)


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"), True)


# ---- 2. isolation: a chain that saw its neighbour's text or trees would emit one long copy

def _isolation(lib, copies):
    a = synth.alice()
    items = [a[:3000]] * copies + [a[:2999]]
    for quality in (10, 11):
        _check(lib, items, quality, 22)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"), 8)


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"), 64)


# ---- 3. table reuse: one table, then two, groups of 50 items (settings are read once per process: one child per setting).  The
# items share content, so that a bucket or a forest node left by the item in front points at plausible text of the next one.

_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_zopfli, test_cabi
lib = test_cabi._load(%r)
items = test_batch_zopfli._reuse_items()
h = hashlib.sha256()
infos = []
for q in (10, 11):
    for out in lib.compress_batch(items, q, 22, zopfli_items=True):
        h.update(len(out).to_bytes(8, "little") + out)
    infos.append(lib.last_batch_info())
print("digest", h.hexdigest(), "infos", infos)
"""


def _reuse_items():
    a = synth.alice()
    # 200 .. 3000 bytes, most of them short (a table runs its items one after the other), all from the same 6 KB of text
    items = [a[37 * i:37 * i + 200 + 47 * (i % 13)] for i in range(112)]
    items[5:5] = [a[100:3100], a[0:2500]]
    # (largest first within a group: the random item runs in front of shorter text, and a[500:2900] in front of a[40:1900])
    items[60:60] = [synth.random_bytes(1500), a[500:2900], a[40:1900]]
    items[100:100] = [a[1000:4000], a[2000:4400], a[3000:3200]]
    assert len(items) == 120 and min(len(x) for x in items) == 200 and max(len(x) for x in items) == 3000
    return items


def _reuse(which):
    items = _reuse_items()
    h = hashlib.sha256()
    for q in (10, 11):
        for x in items:
            out = _oracle(x, q, 22)
            h.update(len(out).to_bytes(8, "little") + out)
    for tables in ("1", "2"):
        env = dict(os.environ)
        for name in ("BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_GROUP_BYTES"):
            env.pop(name, None)
        env.update({"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_GROUP_ITEMS": "50"})
        r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
        want = "digest %s infos %s" % (h.hexdigest(), [[120, 0, 120, 0, 0, 0, 0, 0], [120, 120, 0, 0, 3, 0, 0, 0]])
        assert r.returncode == 0 and want in r.stdout, (tables, want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_reuse_gpu():
    _reuse("gpu")


# ---- 4. positions skipped behind long matches (hq.rs:929-953, 1310-1340): matches beyond the Zopfli length, 150 / 325

def _skipped_positions(lib, quick_step):
    a = synth.alice()
    items = [b"abcdefgh" * 600, bytes(5000), a[:1500] * 3, b"ab" * 2000 + a[:500]]
    for quality in (10, 11):
        _check(lib, items, quality, 22)
    if quick_step:
        # The issue's case for quality 10's quick step of 16 KiB.  Quality 10 is not taken by the route (module docstring), so this
        # item goes one by one and the case runs none of the route's code: it only pins the bytes and that routing.
        _check(lib, items + [bytes(40000)], 10, 22)


def test_skipped_positions_emu():
    _skipped_positions(test_cabi._load("emu"), True)


@pytest.mark.gpu
def test_skipped_positions_gpu():
    _skipped_positions(test_cabi._load("gpu"), False)


# ---- 5. seeded set: text, mixed and random items of 1 .. 4096 bytes; windows smaller than an item (lgwin 10) exercise the
# wrap-around of the forest and max_backward_limit

_SEEDED_CASES = [(q, w, 0) for q in (10, 11) for w in (10, 16, 18, 24)] + [(q, 22, m) for q in (10, 11) for m in (0, 2, 6)]


@functools.lru_cache(maxsize=None)
def _seeded():
    return tuple(test_batch._seeded_items(256, 1, 4096, 17))


@pytest.mark.parametrize("quality,lgwin,mode", _SEEDED_CASES)
def test_seeded_emu(quality, lgwin, mode):
    _check(test_cabi._load("emu"), list(_seeded()[:96]), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _SEEDED_CASES)
def test_seeded_gpu(quality, lgwin, mode):
    _check(test_cabi._load("gpu"), list(_seeded()), quality, lgwin, mode)


# ---- 6. capacity: an item whose buffer is one byte short fails alone

def _capacity(lib, quality):
    _raw_ex, _raw_one = test_batch_long._raw_ex, test_batch._raw_one
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:3000], b"", synth.random_bytes(2000), synth.markov_text(700, 9), b"q"]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes = _raw_ex(lib, quality, 22, ZOPFLI, items, roomy)
    assert ret == 1 and results == [1] * len(items)
    side = _side(items, quality)
    assert lib.last_batch_info() == [5, side, 4 - side, 1, 1 if side else 0, 0, 0, 0]
    for x, out in zip(items, outs):
        assert out == _oracle(x, quality, 22)
    # a buffer one byte short for item k fails k alone (capacity 0 included), and the call returns 0
    for k in (0, 3, 1, 4):
        caps = list(roomy)
        caps[k] = len(outs[k]) - 1
        assert _raw_one(lib, quality, 22, items[k], caps[k])[0] == 0
        ret, got, results, sizes = _raw_ex(lib, quality, 22, ZOPFLI, items, caps)
        assert ret == 0
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
    assert _raw_ex(lib, quality, 22, ZOPFLI, [], [])[0] == 1
    ret, got, _, _ = _raw_ex(lib, quality, 22, ZOPFLI, items, roomy, with_results=False)
    assert ret == 1 and got == outs


@pytest.mark.parametrize("quality", [10, 11])
def test_capacity_emu(quality):
    _capacity(test_cabi._load("emu"), quality)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [10, 11])
def test_capacity_gpu(quality):
    _capacity(test_cabi._load("gpu"), quality)


# ---- 7. threads: four threads, each with a routed batch of its own

def _threads(lib):
    batches = [[x[:1500] for x in _seeded()[64 * t:64 * (t + 1)]] for t in range(4)]
    want = [[_oracle(x, 11, 22) for x in batches[t]] for t in range(4)]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 11, 22, zopfli_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i == [64, 64, 0, 0, 1, 0, 0, 0] for i in infos), infos


def test_threads_emu():
    _threads(test_cabi._load("emu"))


@pytest.mark.gpu
def test_threads_gpu():
    _threads(test_cabi._load("gpu"))
