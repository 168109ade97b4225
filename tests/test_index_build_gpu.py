"""The index build of the LZ77 stage on the product library -- k_compute_keys (which also counts the digits of the sort's first
pass), the two k_radix_scatter passes (the second one also writes key_first / key_last) and the first gather of the stored bits:
byte identity with the oracle on the shapes where these kernels can go wrong.

A sort tile is 4096 elements and a scan tile 1024; a wave of the scatter kernel ranks a quarter of a tile.  So: inputs shorter than
the hash length and than one wave, lengths around one and two sort tiles, several thousand tiles with a ragged last one (with the
size hint, i.e. the 64-bit hash of H6), one key that owns every slot (and more than 65 536 of them: wrap marks, one non-empty key
range), nearly every key present with runs of one or two slots, the rank path of quality 9 and the 16-bit keys of quality 10,
where the tail key 0xffff can be a real key as well, and a stream in two pieces (carried ring counters).  The first four groups
run once more under BROTLI_MI355X_SELFTEST=1, where the library checks the sorted columns, the key ranges and the candidate rows
against a host recomputation."""
import functools
import os
import subprocess
import sys

import pytest

import synth
import test_streaming
from cmp_stream import check_bytes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Q, W, SH = 1, 2, 5
TILE_EDGES = [1, 7, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 1]
HINTED = [(1 << 20) + 1, (1 << 20) + 4097]


@pytest.fixture(scope="module")
def L():
    import gpulib
    return gpulib.lib()


@functools.lru_cache(maxsize=None)
def markov():
    return synth.markov_text((1 << 20) + 4097)


@pytest.mark.parametrize("length", TILE_EDGES)
def test_tile_edges(L, length):
    d = markov()[:length]
    assert len(d) == length
    assert check_bytes(L, "markov %d" % length, d, [(Q, 5), (W, 22)])


@pytest.mark.parametrize("length", HINTED)
def test_many_tiles_ragged_last_h6(L, length):
    d = markov()[:length]
    assert len(d) == length
    assert check_bytes(L, "markov %d hinted" % length, d, [(Q, 5), (W, 22), (SH, length)])


def test_one_key_owns_every_slot(L):
    assert check_bytes(L, "zeros 70000", bytes(70000), [(Q, 5), (W, 22)])


def test_nearly_every_key_present(L):
    d = synth.random_bytes(256 << 10)
    assert check_bytes(L, "random 256 KiB", d, [(Q, 5), (W, 22)])


def test_rank_path_quality_9(L):
    a = synth.alice()
    assert check_bytes(L, "alice q9", a, [(Q, 9), (W, 22)])


def test_sixteen_bit_keys_quality_10(L):
    a = synth.alice()[:16 << 10]
    assert check_bytes(L, "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))])
    d = synth.random_bytes(64 << 10)
    assert check_bytes(L, "random 64 KiB q10", d, [(Q, 10), (W, 22), (SH, len(d))])


def test_stream_in_two_pieces():
    """two writes of 100 000 bytes, each a piece of its own (the batch size is turned down to one write): the second piece's index
    is built on a text that starts with the first one's bytes, with the ring counters carried over"""
    test_streaming._run("gpu", [("markov 200000 q5 w16 in two writes", "synth.markov_text(200000, 3)", 5, 16, 100000, 0, False)], 100000,
                        flush_part=False)


_SELFTEST_CHILD = """
import sys
sys.path.insert(0, %r)
import gpulib, synth, test_index_build_gpu as t
from cmp_stream import check_bytes
L = gpulib.lib()
Q, W, SH = 1, 2, 5
for n in t.TILE_EDGES:
    assert check_bytes(L, "markov %%d" %% n, t.markov()[:n], [(Q, 5), (W, 22)])
for n in t.HINTED:
    assert check_bytes(L, "markov %%d hinted" %% n, t.markov()[:n], [(Q, 5), (W, 22), (SH, n)])
assert check_bytes(L, "zeros 70000", bytes(70000), [(Q, 5), (W, 22)])
assert check_bytes(L, "random 256 KiB", synth.random_bytes(256 << 10), [(Q, 5), (W, 22)])
print("selftest ok")
"""


def test_selftest_recomputes_the_index_on_the_host():
    env = dict(os.environ, BROTLI_MI355X_SELFTEST="1")
    r = subprocess.run([sys.executable, "-c", _SELFTEST_CHILD % HERE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
