"""BrotliMi355xCompressBatchEx with BROTLI_MI355X_BATCH_ROUTE_QUICK_LONG_ITEMS (16): at qualities 2 to 4 the items of more than one
and at most four input blocks (16 385 to 65 536 bytes at quality 2 and 3, 65 537 to 262 144 at quality 4) run side by side on the
device, one chain on a private BasicHasher table each that walks from block to block and leaves up to four meta-blocks
(batch_quick.h).  The bit is independent of BROTLI_MI355X_BATCH_ROUTE_QUICK_ITEMS (4), which takes the items of one block; routes 0,
1, 4 and 5 behave as before.

Whatever path an item takes, its stream is what BrotliEncoderCompress gives on the same bytes: the oracle's.  last_batch_info()
proves which path was taken: [7] counts the items of several blocks taken side by side, [6] those that began side by side and were
redone one by one (a meta-block that is not the item's last took the size fallback).  Every case but the demotion case asserts
[6] == 0, so that none passes through the one-shot path unnoticed.  The CPU tests run the emulation library -- the same host plan
and the same item code -- the GPU tests the product library."""
import ctypes
import functools
import hashlib
import os
import random
import subprocess
import sys
import threading

import pytest

import brotli_parse
import orc
import synth
import test_batch
import test_batch_long
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LONG, QUICK, QUICK_LONG = 1, 4, 16  # BROTLI_MI355X_BATCH_ROUTE_LONG_ITEMS, ..._QUICK_ITEMS, ..._QUICK_LONG_ITEMS
_raw_ex = test_batch_long._raw_ex
noise = test_batch_long.noise


def _block(quality):
    return 16384 if quality < 4 else 65536  # one input block: lgblock 14 at quality 2 / 3, 16 at quality 4


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


def _short(items, quality):
    return sum(1 for x in items if 0 < len(x) <= _block(quality))


def _long(items, quality):
    return sum(1 for x in items if _block(quality) < len(x) <= 4 * _block(quality))


def _check(lib, items, quality, lgwin, mode=0, demoted=0, quick_items=True):
    """the items under routes 16 (| 4): the oracle's bytes, and the info of a call that took every eligible item side by side"""
    got = lib.compress_batch(items, quality, lgwin, mode, quick_items=quick_items, quick_long_items=True)
    info = lib.last_batch_info()
    assert len(got) == len(items)
    for i, (g, item) in enumerate(zip(got, items)):
        assert g == _oracle(item, quality, lgwin, mode), (quality, lgwin, mode, i, len(item))
    empty = sum(1 for x in items if not x)
    short, long_ = (_short(items, quality) if quick_items else 0), _long(items, quality)
    assert info[6] == demoted, info
    assert info[:4] == [len(items), short + long_ - demoted, len(items) - short - long_ - empty + demoted, empty], info
    assert info[5] == 0 and info[7] == long_ - demoted, info
    assert (info[4] >= 1) == (short + long_ > 0), info
    return got, info


def _layout(stream):
    """C<n> / U<n>: a coded / stored meta-block of n bytes, E: the empty last meta-block"""
    out = []
    for mb in brotli_parse.parse(stream)["metablocks"]:
        out.append("E" if mb.get("empty") else ("U" if mb["uncompressed"] else "C") + str(mb["mlen"]))
    return out


# ---- 1. taken side by side (fails where the library does not know the route: the call returns 0)

@functools.lru_cache(maxsize=None)
def _taken_items(quality):
    a = synth.alice()
    if quality < 4:
        return (b"", a[:5000], a[:16384], a[:16385], a[:65536], a[:65537], synth.random_bytes(3000))
    return (b"", a[:5000], a[:65536], a[:65537], a[:152089], (a[:30000] * 9)[:262144], (a[:30000] * 9)[:262145])


def _taken_side_by_side(lib, qualities):
    for quality in qualities:
        items = list(_taken_items(quality))
        caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
        want = [_oracle(x, quality, 22) for x in items]
        short, long_ = _short(items, quality), _long(items, quality)
        assert (short, long_) == ((3, 2) if quality < 4 else (2, 3))
        # routes 16: the items of several blocks alone; 4 | 16 and 1 | 4 | 16: those of one block as well
        for routes, side in ((QUICK_LONG, long_), (QUICK | QUICK_LONG, short + long_), (LONG | QUICK | QUICK_LONG, short + long_)):
            ret, outs, results, _ = _raw_ex(lib, quality, 22, routes, items, caps)
            info = lib.last_batch_info()
            assert ret == 1 and results == [1] * 7, (quality, routes, lib.last_error())
            assert info[:4] == [7, side, 6 - side, 1] and info[4] >= 1 and info[5:] == [0, 0, long_], (quality, routes, info)
            assert outs == want, (quality, routes)
        assert lib.compress_batch(items, quality, 22, quick_long_items=True) == want
        assert lib.last_batch_info()[:4] == [7, long_, 6 - long_, 1] and lib.last_batch_info()[7] == long_
        assert lib.compress_batch(items, quality, 22, quick_items=True, quick_long_items=True) == want
        assert lib.last_batch_info()[:4] == [7, short + long_, 1, 1] and lib.last_batch_info()[7] == long_
        # routes 0, 1, 4 and 5: today's info, the same bytes
        for routes, side in ((0, 0), (LONG, 0), (QUICK, short), (LONG | QUICK, short)):
            ret, outs, results, _ = _raw_ex(lib, quality, 22, routes, items, caps)
            assert ret == 1 and outs == want
            assert lib.last_batch_info() == [7, side, 6 - side, 1, 1 if side else 0, 0, 0, 0], (quality, routes)


def _other_qualities_and_unknown_routes(lib):
    # the bit changes nothing at quality 5
    items = list(_taken_items(2))
    want = [_oracle(x, 5, 22) for x in items]
    assert lib.compress_batch(items, 5, 22) == want
    plain = lib.last_batch_info()
    assert lib.compress_batch(items, 5, 22, quick_long_items=True) == want
    assert lib.last_batch_info() == plain
    # a route this build does not know fails the whole call, and only info[0] is set
    caps = [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]
    for routes in (8, 2, QUICK_LONG | 2, 1 << 31):
        ret, outs, results, sizes = _raw_ex(lib, 2, 22, routes, items, caps)
        assert ret == 0 and results == [0] * 7 and sizes == [0] * 7, routes
        assert lib.last_batch_info() == [7, 0, 0, 0, 0, 0, 0, 0]
        assert "route" in lib.last_error() and "16" in lib.last_error()
    assert type(lib).BATCH_ROUTE_QUICK_LONG_ITEMS == 16
    with pytest.raises(ValueError):
        lib.compress_batch(items, 2, 22, dictionary=b"some dictionary", quick_long_items=True)


@pytest.mark.parametrize("quality", [2, 3, 4])
def test_taken_side_by_side_emu(quality):
    _taken_side_by_side(test_cabi._load("emu"), (quality,))


def test_other_qualities_and_unknown_routes_emu():
    _other_qualities_and_unknown_routes(test_cabi._load("emu"))


@pytest.mark.gpu
def test_taken_side_by_side_gpu():
    _taken_side_by_side(test_cabi._load("gpu"), (2, 3, 4))
    _other_qualities_and_unknown_routes(test_cabi._load("gpu"))


# ---- 2. block seams and several meta-blocks, quality 2 and 3.  The layouts are the oracle's (test_layouts_emu pins them).

@functools.lru_cache(maxsize=None)
def _seam_items(lgwin):
    """((item, layout at quality 2 and 3), ...)"""
    a = synth.alice()
    rnd = synth.random_bytes
    if lgwin == 22:
        # byte 16 381 onward repeats the start: matches begin in the last three positions of block 0 (StitchToPreviousBlock)
        stitched = (a[:16381] + a[:16384] * 2)[:32768]
        assert len(stitched) == 32768 and stitched[16381:16381 + 2000] == stitched[:2000]
        return (
            (a[:65536], ["C49152", "C16384"]),  # the 0x2fff rule closes after three blocks
            (a[:50000], ["C49152", "C848"]),
            ((a[:7000] * 10)[:65536], ["C65536"]),  # copies run across every block end: extend_last_command
            (stitched, None),
        )
    if lgwin == 14:
        return ((a[:65536], ["C16384", "C32768", "C16384"]),)
    assert lgwin == 10
    return (
        (a[:65536], ["C16384"] * 4),  # past the first lap of the 32 KiB ring buffer
        (a[:16385], ["C16384", "U1", "E"]),
        (rnd(33000, 5) + a[:20000], ["U32768", "C16384", "C3848"]),  # stored by should_compress over two blocks
        (a[:20000] + rnd(33000, 5), ["C16384", "C32768", "U3848", "E"]),
        (rnd(50000, 7), ["U32768", "U17232", "E"]),  # nothing coded: the stream stored as a whole
    )


@functools.lru_cache(maxsize=None)
def _seam_items_q4(lgwin):
    a = synth.alice()
    rnd = synth.random_bytes
    assert len(a) == 152089
    five = (
        (a, ["C65536", "C65536", "C21017"]),
        ((a[:30000] * 9)[:262144], ["C65536"] * 4),
        (a[:65537], ["C65536", "U1", "E"]),
        (rnd(140000, 5) + a[:60000], ["U131072", "C65536", "C3392"]),
        (a[:60000] + rnd(140000, 5), ["C65536", "U131072", "U3392", "E"]),
    )
    sixth = (a[:70000] + rnd(70000, 9) + a[70000:140000], ["C131072", "C65536", "C13392"])
    if lgwin == 10:
        return five
    if lgwin == 16:
        return (sixth,)
    assert lgwin == 22  # every item one meta-block (the last one may be followed by the empty one); not pinned
    return tuple((x, None) for x, _ in five + (sixth,))


def _seam_set(quality, lgwin):
    return _seam_items(lgwin) if quality < 4 else _seam_items_q4(lgwin)


_SEAM_CASES = [(q, w, 0) for q in (2, 3) for w in (22, 14, 10)] + [(4, w, 0) for w in (10, 16, 22)] + [(4, 22, 1), (4, 22, 6)]


def _seams(lib, quality, lgwin, mode):
    items = [x for x, _ in _seam_set(quality, lgwin)]
    if mode != 0:
        items = items[:1] + items[3:4]
    _, info = _check(lib, items, quality, lgwin, mode)
    assert info[7] == len(items)


@pytest.mark.parametrize("quality,lgwin,mode", _SEAM_CASES)
def test_seams_emu(quality, lgwin, mode):
    _seams(test_cabi._load("emu"), quality, lgwin, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,mode", _SEAM_CASES)
def test_seams_gpu(quality, lgwin, mode):
    _seams(test_cabi._load("gpu"), quality, lgwin, mode)


@pytest.mark.parametrize("quality,lgwin", [(q, w) for q, w, m in _SEAM_CASES if m == 0])
def test_layouts_emu(quality, lgwin):
    """the inputs above still make the meta-blocks they were chosen for (a later change of inputs must not lose the coverage)"""
    for item, layout in _seam_set(quality, lgwin):
        if layout is not None:
            assert _layout(_oracle(item, quality, lgwin)) == layout, (quality, lgwin, len(item))


@pytest.mark.parametrize("quality", [2, 3, 4])
def test_demotion_layouts_emu(quality):
    """... and the demotion items (section 3): a stored first meta-block that should_compress let through, a coded one behind it"""
    block = _block(quality)
    for seed in (1, 2, 3):
        bad = _demotion_item(quality, seed)
        assert _layout(_oracle(bad, quality, DEMOTION[quality]["lgwin"])) == ["U%d" % block, "C%d" % (len(bad) - block)], (quality, seed)


# ---- 3. demotion: a meta-block that is not the item's last takes the size fallback
#
# The first block is noise that codes to no less than it takes stored, yet should_compress lets it through: its verdict rests on a
# histogram of every 13th byte, and exactly those bytes have their top bit cleared.  Repeats give the block commands, so that the
# distance cache behind it differs from the one at its start; text behind it makes the flush rule close the block as a meta-block of
# its own (the 0x2fff rule at quality 2 / 3, the window at quality 4 and lgwin 16).  The distances cycle because the literal spree
# searches and files only some positions; five hashed bytes need repeats longer than four.

def fooling(block, seed, first, every, dist, rep):
    b = noise(block, seed)
    for q in range(0, block, 13):
        b[q] &= 0x7f
    for i, p in enumerate(range(first, block - rep, every)):
        d = dist + i % 4
        b[p:p + rep] = b[p - d:p - d + rep]
    return bytes(b)


DEMOTION = {
    2: dict(block=16384, first=12800, every=300, dist=5000, rep=12, tail=20000, lgwin=22),
    3: dict(block=16384, first=12800, every=300, dist=5000, rep=12, tail=20000, lgwin=22),
    4: dict(block=65536, first=30000, every=2500, dist=20000, rep=8, tail=40000, lgwin=16),
}


@functools.lru_cache(maxsize=None)
def _demotion_item(quality, seed):
    d = DEMOTION[quality]
    return fooling(d["block"], seed, d["first"], d["every"], d["dist"], d["rep"]) + synth.alice()[:d["tail"]]


def _demotion(lib, quality):
    a = synth.alice()
    block = _block(quality)
    for seed in (1, 2, 3):
        items = [a[:3 * block], _demotion_item(quality, seed), a[:block // 2], a[1000:1000 + 2 * block + 77]]
        got, info = _check(lib, items, quality, DEMOTION[quality]["lgwin"], demoted=1)
        assert info == [4, 3, 1, 0, info[4], 0, 1, 2], info


@pytest.mark.parametrize("quality", [2, 3, 4])
def test_demotion_emu(quality):
    _demotion(test_cabi._load("emu"), quality)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [2, 3, 4])
def test_demotion_gpu(quality):
    _demotion(test_cabi._load("gpu"), quality)


# ---- 4. isolation and reuse

def _isolation(lib, copies):
    a = synth.alice()
    for quality in (2, 3, 4):
        n = 50000 if quality < 4 else 140000
        items = [a[:n]] * copies + [a[:n - 1]]  # a chain that saw its neighbour would emit one long copy
        _check(lib, items, quality, 22)


def test_isolation_emu():
    _isolation(test_cabi._load("emu"), 8)


@pytest.mark.gpu
def test_isolation_gpu():
    _isolation(test_cabi._load("gpu"), 64)


def _permutation_items(quality):
    a = synth.alice()
    block = _block(quality)
    items = [x for w in (22, 10) for x, _ in _seam_set(quality, w)]
    return items + [b"", b"x", a[:700], synth.markov_text(5000, 4), synth.random_bytes(3000), a[:block], a[:4 * block + 1]]


def _permutation(lib):
    for quality, lgwin in ((2, 10), (3, 22), (4, 16)):
        items = _permutation_items(quality)
        order = list(range(len(items)))
        random.Random(5).shuffle(order)
        straight, info = _check(lib, items, quality, lgwin)
        shuffled, info2 = _check(lib, [items[i] for i in order], quality, lgwin)
        assert info2 == info
        assert shuffled == [straight[i] for i in order]


def test_permutation_emu():
    _permutation(test_cabi._load("emu"))


@pytest.mark.gpu
def test_permutation_gpu():
    _permutation(test_cabi._load("gpu"))


# two tables, groups of five items (settings are read once per process: one child per setting).  The items share content, so that a
# slot left by the item in front points at plausible text of the next one; a random item drives the static-dictionary throttle.
_REUSE_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import test_batch_quick_long, test_cabi
lib = test_cabi._load(%r)
h = hashlib.sha256()
infos = []
for q in (2, 3, 4):
    items = test_batch_quick_long._reuse_items(q)
    for out in lib.compress_batch(items, q, 22, quick_items=True, quick_long_items=True):
        h.update(len(out).to_bytes(8, "little") + out)
    infos.append(lib.last_batch_info())
print("digest", h.hexdigest(), "infos", infos)
"""


def _reuse_items(quality):
    a = synth.alice()
    block = _block(quality)
    items = [a[37 * i:37 * i + block + 1500 + 1301 * (i % 11)] for i in range(12)]
    items[3:3] = [synth.random_bytes(block + 3000), a[500:500 + 2 * block]]
    items += [a[:900], a[40:4000], b""]
    return items


def _reuse(which):
    h = hashlib.sha256()
    infos = []
    for q in (2, 3, 4):
        items = _reuse_items(q)
        for x in items:
            out = _oracle(x, q, 22)
            h.update(len(out).to_bytes(8, "little") + out)
        short, long_ = _short(items, q), _long(items, q)
        assert (short, long_) == (2, 14)
        infos.append([len(items), short + long_, 0, 1, (short + 4) // 5 + (long_ + 4) // 5, 0, 0, long_])  # groups of their own
    env = dict(os.environ)
    env.pop("BROTLI_MI355X_BATCH_GROUP_BYTES", None)
    env.update({"BROTLI_MI355X_BATCH_TABLES": "2", "BROTLI_MI355X_BATCH_GROUP_ITEMS": "5"})
    r = subprocess.run([sys.executable, "-c", _REUSE_CHILD % (HERE, which)], env=env, capture_output=True, text=True, timeout=600)
    want = "digest %s infos %s" % (h.hexdigest(), infos)
    assert r.returncode == 0 and want in r.stdout, (want, r.stdout[-2000:] + r.stderr[-3000:])


def test_table_and_group_reuse_emu():
    _reuse("emu")


@pytest.mark.gpu
def test_table_and_group_reuse_gpu():
    _reuse("gpu")


# ---- 5. ABI semantics with an item of several blocks: the body of test_batch_long._abi_semantics at quality 2, routes 4 | 16

def _abi_semantics(lib, quality=2):
    _raw_one = test_batch._raw_one
    routes = QUICK | QUICK_LONG
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q", synth.alice()[:50000]]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes = _raw_ex(lib, quality, 22, routes, items, roomy)
    assert ret == 1 and results == [1] * len(items)
    assert lib.last_batch_info() == [6, 5, 0, 1, 2, 0, 0, 1]
    for x, cap, out in zip(items, roomy, outs):
        assert (1, out) == _raw_one(lib, quality, 22, x, cap)
        assert out == _oracle(x, quality, 22)
    # a buffer too small for item k fails k alone (capacity 0 included), and the call returns 0
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000), (5, 100), (5, 0)):
        caps = list(roomy)
        caps[k] = cap
        assert _raw_one(lib, quality, 22, items[k], cap)[0] == 0
        ret, got, results, sizes = _raw_ex(lib, quality, 22, routes, items, caps)
        assert ret == 0
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
        assert lib.last_batch_info()[6] == 0
    assert _raw_ex(lib, quality, 22, routes, [], [])[0] == 1
    ret, got, _, _ = _raw_ex(lib, quality, 22, routes, items, roomy, with_results=False)
    assert ret == 1 and got == outs
    # an incompressible item of four blocks in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    incompressible = synth.random_bytes(60000)
    cap = max_size(len(incompressible))
    ok, want = _raw_one(lib, quality, 22, incompressible, cap)
    ret, got, results, _ = _raw_ex(lib, quality, 22, routes, [b"abc", incompressible], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want
    assert lib.last_batch_info()[1] == 2 and lib.last_batch_info()[6:] == [0, 1]
    assert orc.decompress(want, len(incompressible)) == incompressible
    # the python wrapper refuses the flag together with a dictionary
    with pytest.raises(ValueError):
        lib.compress_batch(items, quality, 22, dictionary=b"some dictionary", quick_long_items=True)


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
    items = [a[:20000], b"tiny", synth.random_bytes(17000, 5) + a[:17000], synth.random_bytes(3000)]

    def call():
        out = b"|".join(lib.compress_batch(items, 3, 10, quick_items=True, quick_long_items=True))
        assert lib.last_batch_info() == [4, 4, 0, 0, 2, 0, 0, 2]
        return out

    test_device_memory.sweep(L, call, exc)


# ---- 7. threads: four threads, each with a batch of 16 items of 20 to 60 KiB

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    a = synth.alice()
    batches = [[a[t * 300 + i * 50:t * 300 + i * 50 + 20480 + 2730 * i] for i in range(16)] for t in range(4)]
    want = [[_oracle(x, 2, 22) for x in b] for b in batches]
    got, infos = [None] * 4, [None] * 4

    def work(t):
        got[t] = lib.compress_batch(batches[t], 2, 22, quick_long_items=True)
        infos[t] = lib.last_batch_info()  # (per thread)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert got == want
    assert all(i == [16, 16, 0, 0, 1, 0, 0, 16] for i in infos), infos
