"""BrotliMi355xCompressBatchWithDictionaries: an image per dictionary that many items of a group name.

A dictionary that at least BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS side-by-side items of a device group name gets an image, built
once for that group; the chains of those items replay it, every other chain files its own dictionary.  The streams must not know:
every one is the oracle's (BrotliEncoderSetCustomDictionary + one FINISH), and last_batch_info() is what it was.  What the call did
shows in last_batch_image_info(): [images built, items that replayed one, items that filed their own dictionary, 0].

Three routes: qualities 5 .. 8 (no bit), 2 .. 4 (quick_items=True, 512) and 9 (q9_items=True, 4096).  The expected
last_batch_info() of a route comes from the suite of that route (test_batch_dictionaries, _quick, _q9: the same formula with the
route's own eligibility; test_batch_dictionaries' own knows qualities 5 .. 8 only).  The settings are read once per process, so
every case that needs one runs in a child.  The CPU tests run the emulation library -- the same host plan and item code."""
import functools
import os
import random
import subprocess
import sys

import pytest

import synth
import test_batch_dictionaries
import test_batch_dictionaries_q9
import test_batch_dictionaries_quick
import test_batch_dictionary
import test_batch_dictionary_quick
import test_cabi
from test_batch_dictionary import BLOCK, GOLDEN, HERE

# (quality, lgwin) of the mixed group per route
_GREEDY = [(5, 22), (5, 17), (8, 22), (8, 17)]
_QUICK = [(q, w) for q in (2, 3, 4) for w in (22, 10)]
_Q9 = [(9, 17), (9, 22)]
_ROUTES = _GREEDY + _QUICK + _Q9
_IDS = ["q%d-w%d" % c for c in _ROUTES]


def _bits(quality):
    return dict(quick_items=2 <= quality <= 4, q9_items=quality == 9)


def _oracle(item, quality, lgwin, dictionary):
    mod = test_batch_dictionary_quick if 2 <= quality <= 4 else test_batch_dictionary
    return mod._oracle(item, quality, lgwin, dictionary)


def _expected_info(items, dictionaries, item_dicts, quality, lgwin):
    mod = test_batch_dictionaries_quick if 2 <= quality <= 4 else (test_batch_dictionaries_q9 if quality == 9 else test_batch_dictionaries)
    return mod._expected_info(items, dictionaries, item_dicts, quality, lgwin)


def _call(lib, items, dictionaries, item_dicts, quality, lgwin):
    """the call against the oracle and the route's last_batch_info; -> (streams, info, image info)"""
    got = lib.compress_batch_with_dictionaries(items, dictionaries, item_dicts, quality, lgwin, **_bits(quality))
    info, images = lib.last_batch_info(), lib.last_batch_image_info()
    assert len(got) == len(items)
    for i, (g, x, k) in enumerate(zip(got, items, item_dicts)):
        assert g == _oracle(x, quality, lgwin, dictionaries[k]), (quality, lgwin, i, len(x), k, len(dictionaries[k]))
    head, tail = _expected_info(items, dictionaries, item_dicts, quality, lgwin)
    assert info[:4] == head and info[5:] == tail, (info, head, tail)
    return got, info, images


def _child(which, env, name, *args):
    """runs _child_<name>(which, *args) of this module in a fresh process with `env` on top of the caller's"""
    e = dict(os.environ)
    for k in ("BROTLI_MI355X_BATCH_GROUP_BYTES", "BROTLI_MI355X_BATCH_GROUP_ITEMS", "BROTLI_MI355X_BATCH_TABLES", "BROTLI_MI355X_BATCH_DICT_SELF_FILE",
              "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS"):
        e.pop(k, None)
    e.update(env)
    code = "import sys\nsys.path.insert(0, %r)\nimport test_batch_dictionaries_images as t\nt._child_%s(*%r)\nprint('child ok')\n" % (HERE, name, (which,) + args)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, (name, env, r.stdout[-2000:] + r.stderr[-3000:])


# ---- 1. mixed group, counts and bytes: A 20 000 bytes x 40 items, B 65 536 x 33, C 2 x 20, D 7 x 20, E / F / G a few KiB x 1

@functools.lru_cache(maxsize=None)
def _mixed_group():
    a, m = synth.alice(), synth.markov_text(70000, 31)
    dictionaries = [a[:20000], m[:BLOCK], b"\xfe\xff", bytes(range(200, 207)), a[40000:43000], m[1000:6000], synth.random_bytes(2500)]
    named = [0] * 40 + [1] * 33 + [2] * 20 + [3] * 20 + [4, 5, 6]
    random.Random(7).shuffle(named)  # interleaved
    # stretches of the book and of generated text of the same kind, 150 .. 1200 bytes: every dictionary finds matches for its items,
    # and none repeats a dictionary's last bytes -- a match that runs into the dictionary's end is what the reference fails on
    m2 = synth.markov_text(40000, 32)
    items = [(a[50000:] if i % 3 else m2)[211 * i:211 * i + 150 + (97 * i) % 1051] for i in range(len(named))]
    return tuple(items), tuple(dictionaries), tuple(named)


def _mixed(lib, quality, lgwin, want_images=(4, 113, 3, 0)):
    items, dictionaries, named = _mixed_group()
    got, info, images = _call(lib, list(items), list(dictionaries), list(named), quality, lgwin)
    assert info[1] == len(items) and info[4] == 1, info  # one group, every item side by side
    assert images == list(want_images), images
    return got


@pytest.mark.parametrize("quality,lgwin", _ROUTES, ids=_IDS)
def test_mixed_group_emu(quality, lgwin):
    _mixed(test_cabi._load("emu"), quality, lgwin)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin", _ROUTES, ids=_IDS)
def test_mixed_group_gpu(quality, lgwin):
    _mixed(test_cabi._load("gpu"), quality, lgwin)


# ---- 2. one table serves both kinds of start in turn: replay behind 65 536 bytes, self-file behind 2, replay behind 3, self-file
# behind 65 536, with items of 1 .. 65 536 bytes -- on one table and on two.  Every item is a stretch of the long dictionaries' text,
# so a slot of the item in front left in reach would change bytes.

@functools.lru_cache(maxsize=None)
def _reuse_group():
    m = synth.markov_text(140000, 41)
    sizes = (1, 3, 4, 9, 4000, BLOCK)
    dictionaries = [m[:BLOCK], m[70:73]]  # 0: replayed, 65 536 bytes; 1: replayed, 3 bytes
    named, items = [], []
    for j, n in enumerate(sizes):
        lone_short, lone_long = len(dictionaries), len(dictionaries) + 1  # named once each: self-filed
        dictionaries += [m[300 + 2 * j:302 + 2 * j], m[1000 + 17 * j:1000 + 17 * j + BLOCK]]
        named += [0, lone_short, 1, lone_long]
        items += [m[5000 + 3000 * j + 11 * k:5000 + 3000 * j + 11 * k + n] for k in range(4)]
    return tuple(items), tuple(dictionaries), tuple(named)


def _child_reuse(which):
    lib = test_cabi._load(which)
    items, dictionaries, named = _reuse_group()
    for quality, lgwin in ((5, 22), (8, 17), (4, 22), (9, 22)):  # (quality 4: a block of 65 536 bytes on the quick route)
        got, info, images = _call(lib, list(items), list(dictionaries), list(named), quality, lgwin)
        assert info[1] == len(items) and info[4] == 1, info
        assert images == [2, 12, 12, 0], images


@pytest.mark.parametrize("tables", ["1", "2"])
def test_table_reuse_across_both_starts_emu(tables):
    _child("emu", {"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "2"}, "reuse")


@pytest.mark.gpu
@pytest.mark.parametrize("tables", ["1", "2"])
def test_table_reuse_across_both_starts_gpu(tables):
    _child("gpu", {"BROTLI_MI355X_BATCH_TABLES": tables, "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "2"}, "reuse")


# ---- 3. threshold and switch

def _child_no_images(which):
    lib = test_cabi._load(which)
    for quality, lgwin in ((5, 22), (2, 22), (9, 17)):
        _mixed(lib, quality, lgwin, (0, 0, len(_mixed_group()[0]), 0))


def _child_threshold(which):
    lib = test_cabi._load(which)
    a = synth.alice()
    dictionaries = [a[:9000], a[20000:29000]]
    items = [a[3000 + 400 * i:3000 + 400 * i + 300 + 7 * i] for i in range(5)]
    for quality, lgwin in ((5, 22), (2, 22), (9, 17)):
        got, info, images = _call(lib, items, dictionaries, [0, 1, 1, 0, 1], quality, lgwin)  # named 2 and 3 times
        assert images == [1, 3, 2, 0], images


@pytest.mark.parametrize("env", [{"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "0"}, {"BROTLI_MI355X_BATCH_DICT_SELF_FILE": "1"}], ids=["min-items-0", "self-file"])
def test_no_images_emu(env):
    _child("emu", env, "no_images")


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "0"}, {"BROTLI_MI355X_BATCH_DICT_SELF_FILE": "1"}], ids=["min-items-0", "self-file"])
def test_no_images_gpu(env):
    _child("gpu", env, "no_images")


def test_threshold_emu():
    _child("emu", {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "3"}, "threshold")


@pytest.mark.gpu
def test_threshold_gpu():
    _child("gpu", {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "3"}, "threshold")


# ---- 4. the cap: 66 dictionaries of 64 bytes in one group.  65 are named twice -- the first-appearing of them three times -- and
# one is named once: 64 * 2 + 3 + 1 = 132 items.  64 images: the one named three times, then the 63 that appear first of those
# named twice, 3 + 126 = 129 items; the last one named twice and the one named once file their own, 2 + 1 = 3 items.  (The issue
# writes [64, 129, 2, 0] for this shape, which counts 131 items where the shape has 132: the two items of the dictionary left
# without an image, and not the one item of the dictionary named once.  The shape is kept and the count is the shape's.)

def _child_cap(which):
    lib = test_cabi._load(which)
    m = synth.markov_text(20000, 51)
    # (text that ends in a byte no item has: a match that runs into the dictionary's end is what the reference fails on)
    dictionaries = [m[100 * k:100 * k + 63] + bytes([128 + k]) for k in range(66)]
    named = [k for k in range(65)] + [k for k in range(65)] + [0, 65]
    items = [m[7000 + 61 * i:7000 + 61 * i + 40 + i] for i in range(len(named))]
    for quality, lgwin in ((5, 22), (2, 22), (9, 17)):
        got, info, images = _call(lib, items, dictionaries, named, quality, lgwin)
        assert info[1] == 132 and info[4] == 1, info
        assert images == [64, 129, 3, 0], images


def test_cap_emu():
    _child("emu", {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "2"}, "cap")


@pytest.mark.gpu
def test_cap_gpu():
    _child("gpu", {"BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "2"}, "cap")


# ---- 5. images are counted per group: groups of five items, three items to an image

def _child_groups(which):
    lib = test_cabi._load(which)
    a = synth.alice()
    dictionaries = [a[1000 * k:1000 * k + 3000 + k] for k in range(8)]
    items = [a[50000 + 500 * i:50000 + 500 * i + 350 + 3 * i] for i in range(10)]
    for quality, lgwin in ((5, 22), (2, 22), (9, 17)):
        # dictionary 0 named by six items, 3 + 3 over the two groups: an image in each
        got, info, images = _call(lib, items, dictionaries, [0, 1, 0, 2, 0, 0, 3, 0, 4, 0], quality, lgwin)
        assert info[4] == 2 and images == [2, 6, 4, 0], (info, images)
        # ... 5 + 1: one image, and the sixth item files its own copy
        got, info, images = _call(lib, items, dictionaries, [0, 0, 0, 0, 0, 1, 0, 2, 3, 4], quality, lgwin)
        assert info[4] == 2 and images == [1, 5, 5, 0], (info, images)


def test_groups_emu():
    _child("emu", {"BROTLI_MI355X_BATCH_GROUP_ITEMS": "5", "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "3"}, "groups")


@pytest.mark.gpu
def test_groups_gpu():
    _child("gpu", {"BROTLI_MI355X_BATCH_GROUP_ITEMS": "5", "BROTLI_MI355X_BATCH_DICT_IMAGE_MIN_ITEMS": "3"}, "groups")


# ---- 6. failure stays local: the item the reference fails on lies behind an imaged dictionary that healthy items name too

def _failure_stays_local(lib):
    a = synth.alice()
    x = open(os.path.join(GOLDEN, "copy_of_length_one.bin"), "rb").read()
    d, bad = x[:64], x[64:]
    dictionaries = [d, a[10000:14000]]
    healthy = [a[3000 + 170 * i:3000 + 170 * i + 90 + 13 * i] for i in range(16)]  # (enough for an image at any default in 2 .. 16)
    items = [a[:900], bad, a[100:700], d + a[5:300], a[2000:2500], b"tail"] + healthy
    named = [0, 0, 0, 0, 1, 0] + [0] * 16
    caps = test_batch_dictionaries._caps(lib, items)
    ret, got, results, sizes = test_batch_dictionaries._raw(lib, 6, 20, dictionaries, named, items, caps)
    assert ret == 0 and results == [1, 0] + [1] * 20 and sizes[1] == 0, (ret, results, sizes)
    assert "the reference encoder fails on this input" in lib.last_error()
    assert lib.last_batch_info() == [22, 22, 0, 0, 1, 64 + 4000, 0, 0]
    assert lib.last_batch_image_info() == [1, 21, 1, 0]
    for k in [0] + list(range(2, 22)):
        assert got[k] == _oracle(items[k], 6, 20, dictionaries[named[k]]), k


def test_failure_stays_local_emu():
    _failure_stays_local(test_cabi._load("emu"))


@pytest.mark.gpu
def test_failure_stays_local_gpu():
    _failure_stays_local(test_cabi._load("gpu"))


# ---- 8. the other calls

def _other_calls(lib):
    a = synth.alice()
    items = [a[700 * i:700 * i + 400 + 5 * i] for i in range(6)]
    dictionaries = [a[30000:39000], a[60000:61000]]
    lib.compress_batch_with_dictionaries(items * 6, dictionaries, [0, 1] + [0] * 34, 5, 22)  # (35 names: an image at any default)
    assert lib.last_batch_image_info() == [1, 35, 1, 0]
    # a plain call: zeros
    lib.compress_batch(items, 5, 22)
    assert lib.last_batch_image_info() == [0, 0, 0, 0]
    # the shared call, and a one-index call of the per-item entry, which forwards to it
    for quality, bits in ((5, {}), (2, dict(quick_items=True)), (9, dict(q9_items=True))):
        shared = lib.compress_batch_with_dictionary(items, dictionaries[0], quality, 22, **bits)
        assert lib.last_batch_image_info() == [1, 6, 0, 0], (quality, lib.last_batch_image_info())
        single = lib.compress_batch_with_dictionaries(items, dictionaries, [0] * 6, quality, 22, **bits)
        assert single == shared and lib.last_batch_image_info() == [1, 6, 0, 0], (quality, lib.last_batch_image_info())
    # quality 2 without its bit: every item one by one, nothing side by side to count
    lib.compress_batch_with_dictionaries(items, dictionaries, [0, 1, 0, 1, 0, 0], 2, 22)
    assert lib.last_batch_info()[1:3] == [0, 6] and lib.last_batch_image_info() == [0, 0, 0, 0]
    # the Zopfli per-item route keeps filing per chain
    lib.compress_batch_with_dictionaries(items[:4], dictionaries, [0, 1, 0, 0], 11, 22, zopfli_items=True)
    assert lib.last_batch_info()[1] == 4 and lib.last_batch_image_info() == [0, 0, 4, 0]
    # a call that fails as a whole: zeros
    with pytest.raises(type(lib).compress_batch.__globals__["BrotliCompressorException"]):
        lib.compress_batch_with_dictionaries(items, dictionaries, [0, 2, 0, 1, 0, 0], 5, 22)
    assert lib.last_batch_image_info() == [0, 0, 0, 0]
    # count == 0
    assert lib.compress_batch_with_dictionaries([], dictionaries, [], 5, 22) == [] and lib.last_batch_image_info() == [0, 0, 0, 0]


def test_other_calls_emu():
    _other_calls(test_cabi._load("emu"))


@pytest.mark.gpu
def test_other_calls_gpu():
    _other_calls(test_cabi._load("gpu"))
