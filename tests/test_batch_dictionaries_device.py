"""BrotliMi355xCompressBatchWithDictionariesDevice / Library.compress_batch_with_dictionaries_device and
compress_batch_with_dictionary_device: the dictionary batch calls on items and dictionaries that lie in device memory, their streams
left in device memory.

Item i is the stream of BrotliEncoderSetCustomDictionary(dictionaries[item_dictionaries[i]]) + one FINISH on the same bytes (the
oracle's stream API with that dictionary), whatever route it takes, and last_batch_info() is that of the host call on the same
bytes.  The CPU tests run the emulation library, where device memory is host memory and a ctypes buffer serves as "device" address:
they pin the host plan and the ABI rules.  The GPU tests run the product library on torch.uint8 CUDA tensors: they pin the staging
kernel -- per item three copies of n bytes from any address, around the copy's 32-byte threshold, its 16-byte head and tail and its
four source misalignments."""
import ctypes
import hashlib
import os
import subprocess
import sys
import threading
from ctypes import POINTER, c_int32, c_size_t, c_void_p

import pytest

import orc
import synth
import test_batch_dictionary
import test_batch_dictionary_quick
import test_cabi
from test_batch_device import FILL, GUARD, _CudaMem, _HostMem
from test_batch_dictionary_quick import _FAILS_DICTIONARY, _FAILS_ITEM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QUICK_DICTIONARY = 512  # BROTLI_MI355X_BATCH_ROUTE_QUICK_DICTIONARY_ITEMS


def _oracle(item, quality, lgwin, dictionary, mode=0):
    """the caches of the two host suites: qualities 2 .. 4 in test_batch_dictionary_quick's, the others in test_batch_dictionary's"""
    mod = test_batch_dictionary_quick if 2 <= quality <= 4 else test_batch_dictionary
    return mod._oracle(item, quality, lgwin, dictionary, mode)


def _mem(which):
    return _HostMem if which == "emu" else _CudaMem


def _exc(lib):
    return type(lib).compress_batch.__globals__["BrotliCompressorException"]


class _Layout(object):
    """One buffer for all dictionaries and items (`blocks`: [(offset, bytes)], any of which may overlap) and one for all outputs
    (out_at, default back to back behind a guard zone)."""

    def __init__(self, Mem, blocks, caps, out_at=None):
        if out_at is None:
            out_at, at = [], GUARD
            for c in caps:
                out_at.append(at)
                at += c
        self.Mem, self.caps, self.out_at = Mem, list(caps), out_at
        self.src = Mem(max([1] + [a + len(x) for a, x in blocks]), 0)
        assert self.src.ptr % 16 == 0
        for a, x in blocks:
            self.src.write(a, x)
        self.dst = Mem(max([0] + [a + c for a, c in zip(out_at, caps)]) + GUARD)
        Mem.sync()
        self.before = self.src.read()

    def outputs(self):
        return [(self.dst.ptr + a, c) for a, c in zip(self.out_at, self.caps)]

    def streams(self, sizes):
        image = self.dst.read()
        return [image[a:a + n] for a, n in zip(self.out_at, sizes)]

    def untouched_outside(self, sizes):
        """every byte of the output buffer outside [0, size) of its item still holds the fill"""
        image = bytearray(self.dst.read())
        for a, n in zip(self.out_at, sizes):
            image[a:a + n] = bytes([FILL]) * n
        return bytes(image) == bytes([FILL]) * len(image)


def _place(chunks, at=1, gap=0):
    """back to back from offset `at`: [(offset, bytes)]"""
    blocks = []
    for x in chunks:
        blocks.append((at, x))
        at += len(x) + gap
    return blocks


def _call(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, quick=False, single=False):
    """(sizes, info, exception) of the device call on the layout"""
    inputs = [(lay.src.ptr + a, len(x)) for a, x in item_blocks]
    dicts = [(lay.src.ptr + a if x else 0, len(x)) for a, x in dict_blocks]
    error = None
    try:
        if single:
            sizes = lib.compress_batch_with_dictionary_device(inputs, lay.outputs(), dicts[0], quality, lgwin, quick_items=quick)
        else:
            sizes = lib.compress_batch_with_dictionaries_device(inputs, lay.outputs(), dicts, item_dicts, quality, lgwin, quick_items=quick)
    except _exc(lib) as e:
        error, sizes = e, e.sizes
    return sizes, lib.last_batch_info(), error


def _host(lib, dictionaries, items, item_dicts, quality, lgwin, quick=False, single=False):
    """(streams, info) of the host call on the same bytes; a failed item's stream is None"""
    try:
        if single:
            got = lib.compress_batch_with_dictionary(items, dictionaries[0], quality, lgwin, quick_items=quick)
        else:
            got = lib.compress_batch_with_dictionaries(items, dictionaries, item_dicts, quality, lgwin, quick_items=quick)
    except _exc(lib) as e:
        got = e.streams
    return got, lib.last_batch_info()


def _roomy(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]


def _same_as_host(lib, Mem, dictionaries, items, item_dicts, quality, lgwin, quick=False, single=False, oracle=True):
    """the device call on a plain layout against the oracle and against the host call; returns info"""
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items, dict_blocks[-1][0] + len(dict_blocks[-1][1]) + 1 if dict_blocks else 1)
    lay = _Layout(Mem, dict_blocks + item_blocks, _roomy(lib, items))
    sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, quick, single)
    assert error is None, error
    got = lay.streams(sizes)
    named = [0] * len(items) if single else (item_dicts if item_dicts is not None else list(range(len(items))))
    if oracle:
        for i, (g, x, k) in enumerate(zip(got, items, named)):
            assert g == _oracle(x, quality, lgwin, dictionaries[k]), (quality, lgwin, i, len(x), k, len(dictionaries[k]))
    want, host_info = _host(lib, dictionaries, items, item_dicts, quality, lgwin, quick, single)
    assert got == want
    assert info == host_info, (info, host_info)
    assert lay.src.read() == lay.before and lay.untouched_outside(sizes)
    return info


# ---- 1. identity per route

_ITEM_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4097)
_DICTIONARY_SIZES = (2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 4097, 65536)
_ROUTES = [(5, 22, False), (8, 17, False), (2, 22, True), (4, 10, True)]
_ROUTE_IDS = ["q%d-w%d%s" % (q, w, "-quick" if quick else "") for q, w, quick in _ROUTES]


def _identity_batch():
    a = synth.alice()
    items = [a[7:7 + n] for n in _ITEM_SIZES]
    dictionaries = [a[11 + 13 * k:11 + 13 * k + n] for k, n in enumerate(_DICTIONARY_SIZES)]
    return items, dictionaries, [i % len(dictionaries) for i in range(len(items))]  # (21 items: every dictionary is named)


def _identity(which, quality, lgwin, quick, single):
    lib = test_cabi._load(which)
    items, dictionaries, item_dicts = _identity_batch()
    if single:
        # the 4097-byte dictionary: lgwin 10 cuts it to its last 1008 bytes, which start at an odd address
        dictionaries, item_dicts = [dictionaries[_DICTIONARY_SIZES.index(4097)]], None
        assert quality != 4 or (1 << lgwin) - 16 == 1008
    info = _same_as_host(lib, _mem(which), dictionaries, items, item_dicts, quality, lgwin, quick, single)
    assert info[:5] == [len(items), len(items), 0, 0, 1], info  # (every item went side by side: the staging kernel laid them out)


@pytest.mark.parametrize("single", [False, True], ids=["per-item", "shared"])
@pytest.mark.parametrize("quality,lgwin,quick", _ROUTES, ids=_ROUTE_IDS)
def test_identity_emu(quality, lgwin, quick, single):
    _identity("emu", quality, lgwin, quick, single)


@pytest.mark.gpu
@pytest.mark.parametrize("single", [False, True], ids=["per-item", "shared"])
@pytest.mark.parametrize("quality,lgwin,quick", _ROUTES, ids=_ROUTE_IDS)
def test_identity_gpu(quality, lgwin, quick, single):
    _identity("gpu", quality, lgwin, quick, single)


# ---- 2. addresses: 140 dictionaries, one per (start offset 0 .. 19, size), and 25 item variants, one per (start offset 0 .. 4,
# size).  Item i of 700 lies behind dictionary i mod 140 and is variant i mod 25: lcm(140, 25) = 700, so every dictionary meets
# every item offset and the places in the packed text run through every alignment.  Outputs abut between two guard zones.

_ADDRESS_DICTIONARY_SIZES = (2, 31, 32, 33, 47, 48, 49)
_ADDRESS_ITEM_SIZES = (1, 31, 32, 33, 65)
_SLOT = 128


def _address_batch(quality, lgwin):
    a = synth.alice()
    dict_blocks = []
    for k, (off, n) in enumerate((off, n) for off in range(20) for n in _ADDRESS_DICTIONARY_SIZES):
        dict_blocks.append((k * _SLOT + off, a[500 + 3 * k:500 + 3 * k + n]))
    base = len(dict_blocks) * _SLOT
    variants = [(off, n) for off in range(5) for n in _ADDRESS_ITEM_SIZES]
    item_blocks, item_dicts, want = [], [], []
    for i in range(700):
        off, n = variants[i % len(variants)]
        k = i % len(dict_blocks)
        d = dict_blocks[k][1]
        # an item that shares text with its dictionary; the first start the reference does not fail on (decided with the oracle alone)
        for shift in range(64):
            item = a[500 + 3 * k + 1 + shift:500 + 3 * k + 1 + shift + n]
            try:
                want.append(_oracle(item, quality, lgwin, d))
                break
            except orc.ReferencePanics:
                continue
        else:
            raise AssertionError("no item start that the reference encodes")
        item_blocks.append((base + i * _SLOT + off, item))
        item_dicts.append(k)
    assert {(a_ % 16, len(x)) for a_, x in dict_blocks} >= {(off % 16, n) for off in range(16) for n in _ADDRESS_DICTIONARY_SIZES}
    assert {a_ % 4 for a_, _ in item_blocks} == {0, 1, 2, 3}
    return dict_blocks, item_blocks, item_dicts, want


def _addresses(which, quality, lgwin, quick):
    lib = test_cabi._load(which)
    dict_blocks, item_blocks, item_dicts, want = _address_batch(quality, lgwin)
    lay = _Layout(_mem(which), dict_blocks + item_blocks, [len(w) for w in want])
    sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, quick)
    assert error is None, error
    assert sizes == [len(w) for w in want]
    assert lay.dst.read() == bytes([FILL]) * GUARD + b"".join(want) + bytes([FILL]) * GUARD
    assert lay.untouched_outside(sizes)
    assert lay.src.read() == lay.before
    assert info[:4] == [700, 700, 0, 0], info


@pytest.mark.parametrize("quality,lgwin,quick", [(5, 22, False), (2, 22, True)], ids=["q5", "q2-quick"])
def test_addresses_emu(quality, lgwin, quick):
    _addresses("emu", quality, lgwin, quick)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,quick", [(5, 22, False), (2, 22, True)], ids=["q5", "q2-quick"])
def test_addresses_gpu(quality, lgwin, quick):
    _addresses("gpu", quality, lgwin, quick)


# ---- 3. delta layout: the versions of a resource lie back to back in one buffer, item i is version i + 1 and its dictionary is
# version i -- the same bytes are an item and the next item's dictionary -- and three more items name version 0

def _delta(which, quality, lgwin, quick):
    lib = test_cabi._load(which)
    a = bytearray(synth.alice()[2000:5000])
    versions = []
    for v in range(10):
        a[37 * v + 5:37 * v + 9] = b"<%02d>" % v
        versions.append(bytes(a[:1500 + 111 * v]))
    blocks = _place(versions, 5)
    extra = [versions[0][100:900], versions[0][:33], versions[3]]
    extra_blocks = _place(extra, blocks[-1][0] + len(versions[-1]) + 3, gap=1)
    dict_blocks, item_blocks = blocks[:-1], blocks[1:] + extra_blocks
    items = versions[1:] + extra
    item_dicts = list(range(9)) + [0, 0, 0]
    lay = _Layout(_mem(which), blocks + extra_blocks, _roomy(lib, items))
    sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, quick)
    assert error is None, error
    got = lay.streams(sizes)
    want, host_info = _host(lib, versions[:-1], items, item_dicts, quality, lgwin, quick)
    assert got == want and info == host_info, (info, host_info)
    assert got == [_oracle(x, quality, lgwin, versions[k]) for x, k in zip(items, item_dicts)]
    assert info[:4] == [12, 12, 0, 0], info
    assert lay.src.read() == lay.before and lay.untouched_outside(sizes)


@pytest.mark.parametrize("quality,lgwin,quick", [(5, 22, False), (2, 22, True)], ids=["q5", "q2-quick"])
def test_delta_layout_emu(quality, lgwin, quick):
    _delta("emu", quality, lgwin, quick)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,quick", [(5, 22, False), (2, 22, True)], ids=["q5", "q2-quick"])
def test_delta_layout_gpu(quality, lgwin, quick):
    _delta("gpu", quality, lgwin, quick)


# ---- 4. one by one, mixed with side-by-side items, in the caller's order

def _one_by_one(which):
    lib, Mem = test_cabi._load(which), _mem(which)
    a = synth.alice()
    t = synth.markov_text(140000, 5)
    dictionaries = [a[:3000], b"", b"x", t[:70000], a[5000:5100]]
    items = [a[100:2100], b"", t[70000:140000], a[300:1300], a[400:1400], a[600:2600], a[5050:5300], b"", a[9:90]]
    item_dicts = [0, 0, 0, 1, 2, 3, 4, 4, 3]
    # quality 5: the empty items, the 70 000-byte item, dict_size 0 and 1, and the dictionary with more than 65 536 bytes in use
    info = _same_as_host(lib, Mem, dictionaries, items, item_dicts, 5, 22)
    assert info == [9, 2, 7, 0, 1, 3000 + 70000 + 100, 0, 0], info
    # quality 2 without the bit, and quality 9: every item one by one
    short = [x for x in items if len(x) < 5000]
    named = [k for x, k in zip(items, item_dicts) if len(x) < 5000]
    for quality in (2, 9):
        info = _same_as_host(lib, Mem, dictionaries, short, named, quality, 22)
        assert info[:5] == [len(short), 0, len(short), 0, 0], info
    # a shared dictionary of which more than 65 536 bytes are in use: the shared path, all one by one
    info = _same_as_host(lib, Mem, [t[:70000]], [a[600:2600], b"", a[9:90]], None, 5, 22, single=True)
    assert info == [3, 0, 3, 0, 0, 70000, 0, 0], info


def test_one_by_one_emu():
    _one_by_one("emu")


@pytest.mark.gpu
def test_one_by_one_gpu():
    _one_by_one("gpu")


# ---- 5. failures: every one of them fails its item alone

def _failure_batch():
    a = synth.alice()
    return [a[:3000], synth.random_bytes(2000), synth.markov_text(700, 9), b"q"], [a[3000:5000], synth.random_bytes(300), a[:64], a[:9]]


def _fails_alone(lib, Mem, dictionaries, items, item_dicts, quality, lgwin, quick, caps, failed, single=False):
    """the call with these capacities: `failed` fail alone, every other stream is the oracle's, nothing is written outside them"""
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items, dict_blocks[-1][0] + len(dict_blocks[-1][1]) + 1)
    out_at, at = [], GUARD
    for c in caps:
        out_at.append(at)
        at += c + GUARD
    lay = _Layout(Mem, dict_blocks + item_blocks, caps, out_at)
    sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, quick, single)
    assert error is not None and error.failed == failed and error.sizes == sizes, (error, sizes)
    named = [0] * len(items) if single else (item_dicts if item_dicts is not None else list(range(len(items))))
    got = lay.streams(sizes)
    for i, (x, k) in enumerate(zip(items, named)):
        if i in failed:
            assert sizes[i] == 0
        else:
            assert got[i] == _oracle(x, quality, lgwin, dictionaries[k]), i
    image = lay.dst.read()
    assert image[:GUARD] == bytes([FILL]) * GUARD
    assert all(image[a + c:a + c + GUARD] == bytes([FILL]) * GUARD for a, c in zip(out_at, caps))  # (a failed item stays inside its buffer)
    return error, info


def _failures(which):
    lib, Mem = test_cabi._load(which), _mem(which)
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    for quality, quick in ((5, False), (2, True)):
        items, dictionaries = _failure_batch()
        item_dicts = [0, 1, 2, 3]
        want = [_oracle(x, quality, 22, d) for x, d in zip(items, dictionaries)]
        # one byte short of the stream, and no room at all
        for k, cap in ((0, len(want[0]) - 1), (2, len(want[2]) - 1), (3, 0), (0, 0)):
            caps = [len(w) + 5 for w in want]
            caps[k] = cap
            _, info = _fails_alone(lib, Mem, dictionaries, items, item_dicts, quality, 22, quick, caps, [k])
            assert info[:4] == [4, 4, 0, 0], info
        # no stored fallback: the item of random bytes one byte short of its stream fails, and nothing stored is left in its place.
        # (No input gives a stream above BrotliEncoderMaxCompressedSize -- the seeded search of test_batch_device found none -- so a
        # buffer one byte short never holds the stored stream either; that the rule of this call has no stored answer where
        # DeliveryRule has one is pinned on the rule itself, by batch_dictionaries_device_check.cpp.)
        assert len(want[1]) <= max_size(len(items[1]))
        caps = [len(w) + 5 for w in want]
        caps[1] = len(want[1]) - 1
        _fails_alone(lib, Mem, dictionaries, items, item_dicts, quality, 22, quick, caps, [1])
    # the input the reference fails on, at quality 2: alone, with the reference's message, the others produced -- behind a
    # dictionary per item (four indices with the same bytes) and through the shared image
    a = synth.alice()
    d = _FAILS_DICTIONARY
    items = [a[:3000], _FAILS_ITEM, a[100:2000], b"tail"]
    with pytest.raises(orc.ReferencePanics):
        _oracle(_FAILS_ITEM, 2, 22, d)
    for single in (False, True):
        error, info = _fails_alone(lib, Mem, [d] if single else [d] * 4, items, None, 2, 22, True, _roomy(lib, items), [1], single)
        assert "reference encoder fails" in str(error) and "reference encoder fails" in lib.last_error()
        assert info[:6] == [4, 4, 0, 0, 1, 14 if single else 56], info
    # ... and one by one (no bit): the same verdict from the stream path
    error, info = _fails_alone(lib, Mem, [d] * 4, items, None, 2, 22, False, _roomy(lib, items), [1])
    assert "reference encoder fails" in str(error) and info[:6] == [4, 0, 4, 0, 0, 56], info


def test_failures_emu():
    _failures("emu")


@pytest.mark.gpu
def test_failures_gpu():
    _failures("gpu")


# ---- 6. validation: what fails the whole call fails it before any work is done

def _raw(lib, lay, dict_blocks, item_blocks, item_dicts, quality, lgwin, routes, num_dicts=None):
    """BrotliMi355xCompressBatchWithDictionariesDevice through ctypes: (return value, [item result], [size])"""
    n, nd = len(item_blocks), len(dict_blocks)
    dicts = (c_void_p * max(1, nd))(*[lay.src.ptr + a for a, _ in dict_blocks])
    dict_sizes = (c_size_t * max(1, nd))(*[len(x) for _, x in dict_blocks])
    named = ctypes.cast(None, POINTER(c_size_t)) if item_dicts is None else (c_size_t * max(1, n))(*item_dicts)
    inputs = (c_void_p * max(1, n))(*[lay.src.ptr + a for a, _ in item_blocks])
    in_sizes = (c_size_t * max(1, n))(*[len(x) for _, x in item_blocks])
    outputs = (c_void_p * max(1, n))(*[p for p, _ in lay.outputs()])
    out_sizes = (c_size_t * max(1, n))(*lay.caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchWithDictionariesDevice(quality, lgwin, 0, routes, nd if num_dicts is None else num_dicts, dicts, dict_sizes, n,
                                                                  named, inputs, in_sizes, outputs, out_sizes, results)
    return ret, list(results)[:n], list(out_sizes)[:n]


def _validation(which):
    lib, Mem = test_cabi._load(which), _mem(which)
    a = synth.alice()
    dictionaries, items = [a[:500], a[500:900]], [a[100:700], a[20:50], a[800:1000]]
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items, 1000)
    lay = _Layout(Mem, dict_blocks + item_blocks, _roomy(lib, items))

    def refused(item_dicts, routes=0, num_dicts=None, quality=5):
        ret, results, sizes = _raw(lib, lay, dict_blocks, item_blocks, item_dicts, quality, 22, routes, num_dicts)
        assert ret == 0 and results == [0, 0, 0] and sizes == [0, 0, 0]
        assert lib.last_batch_info() == [3, 0, 0, 0, 0, 0, 0, 0]
        assert lay.dst.read() == bytes([FILL]) * len(lay.dst.read())  # (nothing was written to device memory)
        return lib.last_error()

    assert "names dictionary 2 of 2" in refused([0, 2, 1])
    assert "item_dicts is NULL" in refused(None)  # (two dictionaries, three items)
    for routes in (1, 4, 256, QUICK_DICTIONARY | 4):
        for quality in (5, 2):
            assert "route" in refused([0, 1, 0], routes=routes, quality=quality)
    # the Python method raises for both, with every size 0
    for item_dicts in ([0, 5, 1], None):
        sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, item_dicts, 5, 22)
        assert error is not None and error.failed == [0, 1, 2] and sizes == [0, 0, 0] and info == [3, 0, 0, 0, 0, 0, 0, 0]
    # routes == 0 at quality 2: accepted, every item one by one
    ret, results, sizes = _raw(lib, lay, dict_blocks, item_blocks, [0, 1, 0], 2, 22, 0)
    assert ret == 1 and results == [1, 1, 1]
    assert lib.last_batch_info()[:5] == [3, 0, 3, 0, 0]
    assert lay.streams(sizes) == [_oracle(x, 2, 22, dictionaries[k]) for x, k in zip(items, [0, 1, 0])]
    # ... with the bit: side by side; item_dicts == NULL with as many dictionaries as items is accepted
    ret, results, sizes = _raw(lib, lay, dict_blocks + dict_blocks[:1], item_blocks, None, 2, 22, QUICK_DICTIONARY)
    assert ret == 1 and lib.last_batch_info()[:5] == [3, 3, 0, 0, 1]
    assert lay.streams(sizes) == [_oracle(x, 2, 22, dictionaries[k]) for x, k in zip(items, [0, 1, 0])]
    # no items: nothing to do
    empty = _Layout(Mem, dict_blocks, [])
    assert _raw(lib, empty, dict_blocks, [], [], 5, 22, 0)[0] == 1
    assert lib.compress_batch_with_dictionaries_device([], [], [], []) == []


def test_validation_emu():
    _validation("emu")


@pytest.mark.gpu
def test_validation_gpu():
    _validation("gpu")


# ---- 7. groups and table reuse: 40 items in groups of 7 on 3 tables (the variables are read once per process: a fresh child)

def _reuse_batch():
    a = synth.alice()
    dictionaries = [a[k:k + (20000 if k % 2 == 0 else 2)] for k in range(40)]
    items = [a[3000 + 900 * k:3000 + 900 * k + 700 + 37 * k] for k in range(40)]
    return items, dictionaries


def _reuse_child(which):
    if which == "gpu":
        import torch  # noqa: F401  (before the library, as conftest.py has it: one HIP runtime in the process, torch's)
    lib = test_cabi._load(which)
    items, dictionaries = _reuse_batch()
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items, dict_blocks[-1][0] + len(dictionaries[-1]) + 1)
    h, groups = hashlib.sha256(), []
    for quality, quick in ((5, False), (2, True)):
        lay = _Layout(_mem(which), dict_blocks + item_blocks, _roomy(lib, items))
        sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, None, quality, 22, quick)
        assert error is None, error
        assert info[:4] == [40, 40, 0, 0], info
        for out in lay.streams(sizes):
            h.update(len(out).to_bytes(8, "little") + out)
        groups.append(info[4])
    print("digest", h.hexdigest(), "groups", groups)


_REUSE_CHILD = """
import sys
sys.path.insert(0, %r)
import test_batch_dictionaries_device
test_batch_dictionaries_device._reuse_child(%r)
"""


def _reuse(which):
    items, dictionaries = _reuse_batch()
    h = hashlib.sha256()
    for quality in (5, 2):
        for x, d in zip(items, dictionaries):
            out = _oracle(x, quality, 22, d)
            h.update(len(out).to_bytes(8, "little") + out)
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
    env.update({"BROTLI_MI355X_BATCH_TABLES": "3", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "7"})
    r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
    want = "digest %s groups %s" % (h.hexdigest(), [6, 6])
    assert r.returncode == 0 and want in r.stdout, (want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu")


# ---- 8. memory: every failed allocation fails the call, and no block stays live (the emulation library counts them)

@pytest.mark.parametrize("quality,quick", [(5, False), (2, True)], ids=["q5", "q2-quick"])
def test_failed_call_frees_its_blocks_emu(quality, quick):
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    a = synth.alice()
    dictionaries = [a[100000:112000], synth.markov_text(3000, 2), a[:17]]
    items = [a[:12000], b"tiny", synth.markov_text(9000, 3), synth.random_bytes(3000)]
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items, dict_blocks[-1][0] + len(dictionaries[-1]) + 1)
    lay = _Layout(_HostMem, dict_blocks + item_blocks, _roomy(lib, items))

    def call():
        sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, [0, 1, 2, 1], quality, 22, quick)
        if error is not None:
            raise error
        assert info[:6] == [4, 4, 0, 0, 1, 15017], info
        return b"|".join(lay.streams(sizes))

    test_device_memory.sweep(L, call, _exc(lib))


# ---- 9. threads: two threads, each with its own call of 64 items and its own tensors

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[977 * t + 300 * i:977 * t + 300 * i + 150 + 29 * i] for i in range(64)] for t in range(2)]
    dicts = [[a[50000 + 911 * t + 200 * i:50000 + 911 * t + 200 * i + 100 + 61 * i] for i in range(64)] for t in range(2)]
    want = [[_oracle(x, 5, 22, d) for x, d in zip(batches[t], dicts[t])] for t in range(2)]
    got, errors = [None] * 2, []

    def work(t):
        try:
            dict_blocks = _place(dicts[t], 3 + t)
            item_blocks = _place(batches[t], dict_blocks[-1][0] + len(dicts[t][-1]) + 1)
            lay = _Layout(_CudaMem, dict_blocks + item_blocks, _roomy(lib, batches[t]))
            sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, None, 5, 22)
            got[t] = (lay.streams(sizes), info[:4], error)
        except Exception as e:  # (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert not errors, errors
    for t in range(2):
        assert got[t][2] is None, got[t][2]
        assert got[t][0] == want[t]
        assert got[t][1] == [64, 64, 0, 0], got[t][1]


# ---- 10. exactly sized heap blocks: a stand-alone host program over the emulation library (batch_dictionaries_device_check.cpp);
# built with a sanitizer by hand, it judges every read and write of the plan

def test_exact_heap_blocks_program_emu(tmp_path):
    import emu
    emu.build()
    exe = str(tmp_path / "batch_dictionaries_device_check")
    cmd = ["g++", "-std=c++17", "-O1", "-DBROTLI_HOST_EMU=1", "-I", os.path.join(ROOT, "rust-brotli_amd", "csrc"),
           os.path.join(HERE, "batch_dictionaries_device_check.cpp"), os.path.join(emu.EMU_DIR, "libbrotli_emu.so"), "-Wl,-rpath," + emu.EMU_DIR, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
