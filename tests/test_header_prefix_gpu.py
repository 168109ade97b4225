"""The meta-block header in two items on the product library: its prefix (meta-block header, block-split codes, distance parameters,
context modes, context maps) is composed by workgroups of the k_build_codes launch, beside the code jobs, and k_write_headers appends
the serialised trees; the code jobs are listed per pool slot before the splitter has run and return at once for an empty slot; the
three command scans are one scan over three arrays.  Byte identity with the oracle (cmp_stream.check_bytes) on the smallest shapes
where these seams can go wrong, and the three-array scan against numpy.cumsum.

Which branch an input takes is asserted on the ORACLE's stream (brotli_parse), so a case cannot silently test another branch:
the literal context map (1, 2, 3 or 13 contexts per block type; below quality 7 the reference never picks 3, encode.rs:1885-1927,
so that outcome comes from quality 7), the number of block types per kind, and the length of the header.

The append kernel stages a header in workgroup memory up to 5120 * 64 = 327 680 bits of prefix + trees and in global memory above.
The two inputs of header_cases.py are 162 734 and 186 245 bits: both lie below that line now (they straddled the earlier one, which
counted the trees plus a fixed 163 840), and a header above it takes hundreds of prefix codes of every kind.  So the pair runs twice:
as it is (both staged in workgroup memory), and with BROTLI_MI355X_TEST_HEADER_LDS_BITS=174080 in a child process, which puts the
line between them (the longer one is then finished in global memory)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import brotli_parse
import emu
import header_cases
import orc
import synth
from cmp_stream import check_bytes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Q, W, NOCTX, SH, Q9_5 = 1, 2, 4, 5, 150
HEADER_LDS_BITS = 5120 * 64
TEST_LINE_BITS = 174080  # between the two headers of header_cases.py


@pytest.fixture(scope="module")
def L():
    import gpulib
    return gpulib.lib()


@functools.lru_cache(maxsize=None)
def markov_1m():
    return synth.markov_text(1 << 20)


def markov_with_noise():
    d = markov_1m()
    h = len(d) // 2
    return d[:h] + synth.random_bytes(200000) + d[h:]


@functools.lru_cache(maxsize=None)
def cyrillic_words():
    """216 KB of UTF-8 text in two-byte characters: the bigram statistics of DecideContexts choose 2 contexts at quality 5 and
    3 contexts at quality 7"""
    import random
    rng = random.Random(3)
    words = ["Алиса", "кролик", "страна", "чудес", "время", "слово", "где", "это", "и", "в", "не", "на", "что", "он", "она", "было",
             "the", "and", "of", "naïve", "café"]
    return " ".join(rng.choice(words) for _ in range(30000)).encode("utf-8")


def first_header(data, params):
    """the header of the first compressed meta-block of the oracle's stream"""
    stream, _ = orc.stream_compress(data, params)
    mbs = brotli_parse.parse(stream, first_header_only=True)["metablocks"]
    return [m for m in mbs if "nbltypes" in m][0]


def contexts_per_type(h):
    assert h["ntrees_l"] % h["nbltypes"][0] == 0, (h["ntrees_l"], h["nbltypes"])
    return h["ntrees_l"] // h["nbltypes"][0]


def header_bits(h):
    return h["data_bit_offset"] - h["bit_offset"]


# ---- one meta-block, one block type per kind
def test_one_block_type_per_kind(L):
    a = synth.alice()[:2000]
    p = [(Q, 5), (W, 22), (SH, len(a))]
    assert first_header(a, p)["nbltypes"] == (1, 1, 1)
    assert check_bytes(L, "alice 2000", a, p)
    z = bytes(300000)
    assert first_header(z, [(Q, 5), (W, 22)])["nbltypes"] == (1, 1, 1)
    assert check_bytes(L, "zeros 300000", z, [(Q, 5), (W, 22)])


# ---- several block types per kind (switch bits from the prefix job), a stored meta-block between compressed ones (its early
# return), three and more prefix jobs in one launch
def test_stored_metablock_between_compressed_ones(L):
    d = markov_with_noise()
    params = [(Q, 5), (W, 16), (SH, len(d))]
    _, st = emu.encode_stream(L, d, params, segment_bytes=4096)
    assert st["metablocks"] >= 3 and 1 <= st["uncompressed_metablocks"] < st["metablocks"], (st["metablocks"], st["uncompressed_metablocks"])
    assert check_bytes(L, "markov + 200 KB noise w16", d, params)


def test_several_block_types_per_kind(L):
    d = synth.mixed(256 << 10)
    p = [(Q, 5), (W, 22), (SH, len(d))]
    h = first_header(d, p)
    assert min(h["nbltypes"]) >= 2, h["nbltypes"]
    assert check_bytes(L, "mixed 256 KiB", d, p)


# ---- the literal context map
def test_context_map_trivial(L):
    a = synth.alice()  # (DecideContexts turns context modelling down)
    p = [(Q, 5), (W, 22), (SH, len(a))]
    assert contexts_per_type(first_header(a, p)) == 1
    assert check_bytes(L, "alice", a, p)
    d = cyrillic_words()  # (the parameter does)
    p = [(Q, 5), (W, 22), (SH, len(d)), (NOCTX, 1)]
    assert contexts_per_type(first_header(d, p)) == 1
    assert check_bytes(L, "cyrillic, no context modelling", d, p)


def test_context_map_2_contexts(L):
    d = cyrillic_words()
    p = [(Q, 5), (W, 22), (SH, len(d))]
    assert contexts_per_type(first_header(d, p)) == 2
    assert check_bytes(L, "cyrillic q5", d, p)


def test_context_map_3_contexts(L):
    d = cyrillic_words()
    p = [(Q, 7), (W, 22), (SH, len(d))]
    assert contexts_per_type(first_header(d, p)) == 3
    assert check_bytes(L, "cyrillic q7", d, p)


def test_context_map_13_contexts(L):
    d = markov_1m()
    p = [(Q, 5), (W, 22), (SH, len(d))]
    h = first_header(d, p)
    assert contexts_per_type(h) == 13 and h["nbltypes"][0] >= 2, (h["ntrees_l"], h["nbltypes"])
    assert check_bytes(L, "markov 1 MiB", d, p)


# ---- the line between the two stagings of the append kernel
def test_headers_staged_in_workgroup_memory(L):
    for name in ("below", "above"):
        d = header_cases.regimes(*header_cases.CASES[name])
        bits = header_bits(first_header(d, header_cases.params(d)))
        print("header of %s: %d bits (line %d)" % (name, bits, HEADER_LDS_BITS))
        assert bits <= HEADER_LDS_BITS
        assert check_bytes(L, "256 regimes, " + name, d, header_cases.params(d))


_LINE_CHILD = """
import sys
sys.path.insert(0, %r)
import gpulib, header_cases
from cmp_stream import check_bytes
L = gpulib.lib()
for name in ("below", "above"):
    d = header_cases.regimes(*header_cases.CASES[name])
    assert check_bytes(L, "256 regimes, " + name, d, header_cases.params(d))
print("line ok")
"""


def test_header_on_either_side_of_a_lowered_line():
    sides = []
    for name in ("below", "above"):
        d = header_cases.regimes(*header_cases.CASES[name])
        sides.append(header_bits(first_header(d, header_cases.params(d))))
    print("headers: %d and %d bits, line %d" % (sides[0], sides[1], TEST_LINE_BITS))
    assert sides[0] <= TEST_LINE_BITS * 0.95 and sides[1] >= TEST_LINE_BITS * 1.05, sides
    env = dict(os.environ, BROTLI_MI355X_TEST_HEADER_LDS_BITS=str(TEST_LINE_BITS))
    r = subprocess.run([sys.executable, "-c", _LINE_CHILD % HERE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "line ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the other modes of the shared kernels: kCodeFast / kCodeStatic (2), kCodePlain (3), the greedy splitter's other users (4, 9),
# the quality >= 10 job list, which is written from the results and must not meet the early return of the pool slots (10, "9.5")
@pytest.mark.parametrize("quality", [2, 3, 4, 9])
def test_other_qualities(L, quality):
    d = synth.mixed(256 << 10)
    assert check_bytes(L, "mixed 256 KiB q%d" % quality, d, [(Q, quality), (W, 22), (SH, len(d))])


def test_quality_2_static_codes(L):
    a = synth.alice()[:2000]  # (up to 128 commands: the static command and distance codes)
    assert check_bytes(L, "alice 2000 q2", a, [(Q, 2), (W, 22), (SH, len(a))])


def test_quality_10(L):
    a = synth.alice()[:16 << 10]
    assert check_bytes(L, "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))])


def test_quality_9_5(L):
    a = synth.alice()[:64 << 10]
    assert check_bytes(L, "alice 64 KiB q9.5", a, [(Q, 10), (Q9_5, 1), (W, 22), (SH, len(a))])


# ---- pool slots beyond num_histos: the literal pool of these inputs holds 150 and more slots (one per 512 literals, at most 257)
def test_pool_slots_left_empty_and_filled(L):
    a = synth.alice()
    p = [(Q, 5), (W, 22), (SH, len(a))]
    assert first_header(a, p)["ntrees_l"] == 1  # text: one literal type, the other slots stay empty
    assert check_bytes(L, "alice", a, p)
    d = synth.mixed(256 << 10)
    p = [(Q, 5), (W, 22), (SH, len(d))]
    assert first_header(d, p)["ntrees_l"] >= 16  # the mix fills many
    assert check_bytes(L, "mixed 256 KiB", d, p)


# ---- three of the above under BROTLI_MI355X_SELFTEST=1
_SELFTEST_CHILD = """
import sys
sys.path.insert(0, %r)
import gpulib, synth, test_header_prefix_gpu as t
from cmp_stream import check_bytes
L = gpulib.lib()
Q, W, SH = 1, 2, 5
d = t.markov_with_noise()
assert check_bytes(L, "markov + noise w16", d, [(Q, 5), (W, 16), (SH, len(d))])
d = t.cyrillic_words()
assert check_bytes(L, "cyrillic q7", d, [(Q, 7), (W, 22), (SH, len(d))])
d = synth.mixed(256 << 10)
assert check_bytes(L, "mixed 256 KiB", d, [(Q, 5), (W, 22), (SH, len(d))])
print("selftest ok")
"""


def test_under_selftest():
    env = dict(os.environ, BROTLI_MI355X_SELFTEST="1")
    r = subprocess.run([sys.executable, "-c", _SELFTEST_CHILD % HERE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- a stream in two pieces: PROCESS encodes the meta-blocks that are complete (the open one's commands are gathered but not
# used, so the stage hands over fewer commands than it gathered), FINISH the rest
_PIECES_CHILD = """
import sys
sys.path.insert(0, %r)
import orc, synth, test_cabi
lib = test_cabi._load("gpu")
data = synth.markov_text(3 << 19)
e = lib.encoder(params=[(1, 5), (2, 16)])
for i in range(0, len(data), 65536):
    e.write(data[i:i + 65536])
early = len(e._out)
got = e.finish()
e.close()
assert early > 0, "PROCESS encoded nothing"
assert early < len(got)
assert got == orc.writer_compress(data, 5, 16, chunk=65536), len(got)
print("pieces ok")
"""


def test_stream_in_two_pieces():
    env = dict(os.environ, BROTLI_MI355X_STREAM_BATCH=str(1 << 20))
    r = subprocess.run([sys.executable, "-c", _PIECES_CHILD % HERE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the scan over three arrays at once (brotli_mi355x_debug_scan3): one tile, the tile's edges, two and three levels
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1])
def test_scan_of_three_arrays(L, n):
    L.brotli_mi355x_debug_scan3.restype = ctypes.c_int
    L.brotli_mi355x_debug_scan3.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    rng = np.random.Generator(np.random.PCG64(n))
    # (the three command arrays: insert lengths, insert + copy lengths, 0 / 1 flags; sums stay below 2^32)
    a = np.stack([rng.integers(0, 300, n), rng.integers(2, 3000, n), rng.integers(0, 2, n)]).astype(np.uint32)
    want = np.cumsum(a, axis=1, dtype=np.uint64) - a
    assert int(want.max()) < 1 << 32
    got = np.ascontiguousarray(a)
    assert L.brotli_mi355x_debug_scan3(got.ctypes.data, n) == 0
    assert np.array_equal(got, want.astype(np.uint32))
