"""The frame that every batch call of the C ABI shares, pinned across all seven entry points at once: BrotliMi355xCompressBatch,
...Ex, ...Device, BrotliMi355xCompressBatchWithDictionary, ...Ex, BrotliMi355xCompressBatchWithDictionaries and ...Device.

What a call does before and after its items -- an unknown route refused before anything else, count == 0, item_results == NULL,
the last_batch_info() it leaves -- and the one dictionary body behind the three ways to put every item behind the same dictionary.
The inputs are tiny: the bytes of each route are pinned by the test files of the routes.  The CPU tests run the emulation library
(device memory is host memory there), the GPU tests the product library on CUDA tensors."""
import ctypes
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_void_p

import pytest

import synth
import test_batch_device
import test_cabi
from test_batch_dictionary import _oracle as _dictionary_oracle

PLAIN = ("BrotliMi355xCompressBatch", "BrotliMi355xCompressBatchEx", "BrotliMi355xCompressBatchDevice")
SHARED = ("BrotliMi355xCompressBatchWithDictionary", "BrotliMi355xCompressBatchWithDictionaryEx")
PER_ITEM = ("BrotliMi355xCompressBatchWithDictionaries", "BrotliMi355xCompressBatchWithDictionariesDevice")
ENTRIES = PLAIN + SHARED + PER_ITEM
# every route an entry point knows, and the entry points that take none
KNOWN_ROUTES = {"BrotliMi355xCompressBatch": None, "BrotliMi355xCompressBatchEx": 1 | 4 | 16 | 32 | 128, "BrotliMi355xCompressBatchDevice": 1 | 4 | 16 | 32 | 128,
                "BrotliMi355xCompressBatchWithDictionary": None, "BrotliMi355xCompressBatchWithDictionaryEx": 4,
                "BrotliMi355xCompressBatchWithDictionaries": 512, "BrotliMi355xCompressBatchWithDictionariesDevice": 512}
UNKNOWN_ROUTE = 2  # (reserved in the plain call, and no dictionary call knows it)


def _items():
    a = synth.alice()
    return [a[100:4100], b"", a[7000:7003], a[20000:25000], a[300:1300]]


def _dictionary():
    return synth.alice()[50000:52000]


def _call(lib, which, entry, quality, lgwin, items, caps, routes=0, dictionaries=(), item_dicts=None, with_results=True):
    """One entry point through ctypes -> (return value, [stream], [item result], [size]).  The device entry points get their items,
    dictionaries and outputs in "device" memory of the library (test_batch_device._mem).  `dictionaries`: the shared calls take
    dictionaries[0]; item_dicts: the per-item calls' index array, None for NULL."""
    n = len(items)
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    res = results if with_results else ctypes.cast(None, POINTER(c_int32))
    device = entry.endswith("Device")
    if device:
        Mem = test_batch_device._mem(which)
        src = [Mem(len(x), 0) for x in items]
        dst = [Mem(c) for c in caps]
        dic = [Mem(len(d), 0) for d in dictionaries]
        for m, x in list(zip(src, items)) + list(zip(dic, dictionaries)):
            m.write(0, x)
        Mem.sync()
        inputs = (c_void_p * max(1, n))(*[m.ptr for m in src])
        outputs = (c_void_p * max(1, n))(*[m.ptr for m in dst])
        dicts = (c_void_p * max(1, len(dic)))(*[m.ptr for m in dic])
    else:
        bufs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
        inputs = (c_char_p * max(1, n))(*items)
        outputs = (c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs])
        dicts = (c_char_p * max(1, len(dictionaries)))(*dictionaries)
    f = getattr(lib.lib, entry)
    if entry in PLAIN:
        args = (quality, lgwin, 0) + (() if entry == PLAIN[0] else (routes,)) + (n, inputs, in_sizes, outputs, out_sizes, res)
    elif entry in SHARED:
        args = (quality, lgwin, 0) + (() if entry == SHARED[0] else (routes,)) + (len(dictionaries[0]), dictionaries[0], n, inputs, in_sizes, outputs,
                                                                                   out_sizes, res)
    else:
        dict_sizes = (c_size_t * max(1, len(dictionaries)))(*[len(d) for d in dictionaries])
        named = ctypes.cast(None, POINTER(c_size_t)) if item_dicts is None else (c_size_t * max(1, n))(*item_dicts)
        args = (quality, lgwin, 0, routes, len(dictionaries), dicts, dict_sizes, n, named, inputs, in_sizes, outputs, out_sizes, res)
    ret = f(*args)
    sizes = list(out_sizes)[:n]
    if device:
        streams = [m.read()[:s] for m, s in zip(dst, sizes)]
    else:
        streams = [b.raw[:s] for b, s in zip(bufs, sizes)]
    return ret, streams, list(results)[:n], sizes


def _caps(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 1024 for x in items]


def _dictionary_args(entry, count):
    """the dictionaries and indices with which a dictionary entry point takes `count` items: all behind one dictionary"""
    if entry in PLAIN:
        return dict()
    return dict(dictionaries=[_dictionary()], item_dicts=[0] * count if entry in PER_ITEM else None)


# ---- (a) an unknown route is refused before count == 0 is looked at

def _unknown_route_without_items(which):
    lib = test_cabi._load(which)
    for entry in ENTRIES:
        if KNOWN_ROUTES[entry] is None:
            continue
        ret, _, _, _ = _call(lib, which, entry, 5, 22, [], [], routes=UNKNOWN_ROUTE, **_dictionary_args(entry, 0))
        error = lib.last_error()
        assert ret == 0 and error.startswith(entry + ": ") and "route" in error, (entry, ret, error)
        assert lib.last_batch_info() == [0] * 8, entry


def test_unknown_route_without_items_emu():
    _unknown_route_without_items("emu")


@pytest.mark.gpu
def test_unknown_route_without_items_gpu():
    _unknown_route_without_items("gpu")


# ---- (b) count == 0 with routes the call knows: done, and the info of a call of no items

def _no_items(which):
    lib = test_cabi._load(which)
    items = _items()[:3]
    for entry in ENTRIES:
        for routes in (0, KNOWN_ROUTES[entry]):
            if routes is None:
                continue
            # (a call with items in front, so that the info of the empty call is its own)
            ret, _, _, _ = _call(lib, which, entry, 5, 22, items, _caps(lib, items), routes=routes, **_dictionary_args(entry, 3))
            assert ret == 1 and lib.last_batch_info()[0] == 3, (entry, routes, lib.last_batch_info())
            ret, _, _, _ = _call(lib, which, entry, 5, 22, [], [], routes=routes, **_dictionary_args(entry, 0))
            assert ret == 1 and lib.last_batch_info() == [0] * 8, (entry, routes, ret, lib.last_batch_info())


def test_no_items_emu():
    _no_items("emu")


@pytest.mark.gpu
def test_no_items_gpu():
    _no_items("gpu")


# ---- (c) item_results == NULL: the same return value, sizes and bytes as with the array -- where every item fits, and where
# one does not (it fails alone; the stored stream of the plain call needs BrotliEncoderMaxCompressedSize bytes)

def _null_item_results(which):
    lib = test_cabi._load(which)
    items = _items()
    roomy = _caps(lib, items)
    tight = list(roomy)
    tight[3] = 10
    for entry in ENTRIES:
        for caps, want in ((roomy, 1), (tight, 0)):
            with_array = _call(lib, which, entry, 5, 22, items, caps, **_dictionary_args(entry, len(items)))
            info = lib.last_batch_info()
            without = _call(lib, which, entry, 5, 22, items, caps, with_results=False, **_dictionary_args(entry, len(items)))
            assert with_array[0] == without[0] == want, (entry, caps, with_array[0], without[0])
            assert with_array[1] == without[1] and with_array[3] == without[3], (entry, with_array[3], without[3])
            assert with_array[2] == [0 if caps is tight and i == 3 else 1 for i in range(len(items))], (entry, with_array[2])
            assert without[2] == [7] * len(items), entry  # (nothing is written through a NULL array's neighbour)
            assert (with_array[3][3] == 0) == (caps is tight), (entry, with_array[3])
            assert info == lib.last_batch_info() and info[0] == len(items), (entry, info, lib.last_batch_info())


def test_null_item_results_emu():
    _null_item_results("emu")


@pytest.mark.gpu
def test_null_item_results_gpu():
    _null_item_results("gpu")


# ---- (d) one dictionary, three ways: every item naming index 0 of the per-item call; the same call with a copy of the dictionary
# per item under distinct indices; BrotliMi355xCompressBatchWithDictionary.  The oracle's bytes from all three; the first and the
# third are one path (equal info, info[5] the dictionary's bytes in use), the second names `count` dictionaries.  Quality 5 takes the
# plain dictionary calls, quality 2 their opt-in routes: 512 in the per-item call is 4 in the shared one.

def _three_ways(which, quality, per_item_routes, shared_entry, shared_routes):
    lib = test_cabi._load(which)
    items, d = _items(), _dictionary()
    n, caps = len(items), _caps(lib, items)
    want = [_dictionary_oracle(x, quality, 22, d) for x in items]
    side = n - 1  # (all but the empty item)
    first = _call(lib, which, PER_ITEM[0], quality, 22, items, caps, routes=per_item_routes, dictionaries=[d], item_dicts=[0] * n)
    first_info = lib.last_batch_info()
    copies = [bytes(bytearray(d)) for _ in range(n)]
    second = _call(lib, which, PER_ITEM[0], quality, 22, items, caps, routes=per_item_routes, dictionaries=copies, item_dicts=None)
    second_info = lib.last_batch_info()
    third = _call(lib, which, shared_entry, quality, 22, items, caps, routes=shared_routes, dictionaries=[d])
    third_info = lib.last_batch_info()
    for got in (first, second, third):
        assert got[0] == 1 and got[2] == [1] * n and got[1] == want, (quality, got[0], got[2], got[3])
    assert first_info == third_info, (quality, first_info, third_info)
    assert first_info[:4] == [n, side, 1, 0] and first_info[4] >= 1 and first_info[5:] == [len(d), 0, 0], (quality, first_info)
    assert second_info[:4] == [n, side, 1, 0] and second_info[4] >= 1 and second_info[5:] == [n * len(d), 0, 0], (quality, second_info)


_THREE_WAYS = [(5, 0, SHARED[0], 0), (2, 512, SHARED[1], 4)]


@pytest.mark.parametrize("quality,per_item_routes,shared_entry,shared_routes", _THREE_WAYS)
def test_three_ways_behind_one_dictionary_emu(quality, per_item_routes, shared_entry, shared_routes):
    _three_ways("emu", quality, per_item_routes, shared_entry, shared_routes)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,per_item_routes,shared_entry,shared_routes", _THREE_WAYS)
def test_three_ways_behind_one_dictionary_gpu(quality, per_item_routes, shared_entry, shared_routes):
    _three_ways("gpu", quality, per_item_routes, shared_entry, shared_routes)
