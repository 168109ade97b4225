"""The emission and context-statistics kernels of the meta-block stage (k_emit_commands, k_emit_literals, k_context_stats) on the
product library: byte identity with the oracle on the shapes where their wave-level form can go wrong.

A wavefront of the emit kernels takes 64 consecutive commands (or literals), collects their bits in a window of workgroup memory
that starts at its first item's stream word, and writes each window word to the stream once; a piece that does not lie inside
the window goes to the stream by itself.  So the cases are: fewer than 64 items, a ragged last wavefront, meta-block boundaries
(and a stored meta-block) inside a wavefront, pieces far behind the window (long literal runs), and the other code modes that
share the kernels (qualities 2-4, 9, 10, "9.5").  k_context_stats samples 64 bytes every 4096: lengths around the first and second
sample and around 256 samples (a workgroup of the earlier kernel).  Three cases run once more under BROTLI_MI355X_SELFTEST=1, where
the library compares the stream behind mb_emit with a piece-by-piece emission and the statistics rows with a host recomputation.

k_write_headers composes a header in workgroup memory unless the meta-block's prefix codes exceed 163 840 bits, and in global memory
above that: one case on either side of the line, measured on the oracle's stream (header_cases.py)."""
import functools
import os
import random
import subprocess
import sys

import pytest

import emu
import header_cases
import synth
from cmp_stream import check_bytes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Q, W, SH, Q9_5 = 1, 2, 5, 150
STATS_LENGTHS = [63, 64, 65, 4159, 4160, 4161] + [64 + 4096 * 255 + d for d in (-1, 0, 1)]


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


def alphabet64_then_text():
    """64 KiB of uniformly random bytes out of 64 symbols (six bits of entropy each: compressible, without matches -- literal runs
    of thousands), then 64 KiB of text"""
    rng = random.Random(64)
    return bytes(rng.randrange(64) + 48 for _ in range(64 << 10)) + synth.alice()[:64 << 10]


def test_fewer_than_64_commands(L):
    a = synth.alice()[:2000]
    assert check_bytes(L, "alice 2000", a, [(Q, 5), (W, 22), (SH, len(a))])


def test_ragged_last_wave(L):
    a = synth.alice()
    assert check_bytes(L, "alice", a, [(Q, 5), (W, 22), (SH, len(a))])


def test_a_handful_of_commands(L):
    assert check_bytes(L, "zeros 300000", bytes(300000), [(Q, 5), (W, 22)])


def test_metablock_boundaries_inside_a_wave(L):
    d = markov_1m()
    params = [(Q, 5), (W, 16), (SH, len(d))]
    _, st = emu.encode_stream(L, d, params, segment_bytes=4096)
    assert st["metablocks"] >= 4, st["metablocks"]
    assert check_bytes(L, "markov 1 MiB w16", d, params)


def test_stored_metablock_between_compressed_ones(L):
    d = markov_with_noise()
    params = [(Q, 5), (W, 16), (SH, len(d))]
    _, st = emu.encode_stream(L, d, params, segment_bytes=4096)
    assert st["metablocks"] >= 4 and st["uncompressed_metablocks"] >= 1, (st["metablocks"], st["uncompressed_metablocks"])
    assert st["uncompressed_metablocks"] < st["metablocks"]
    assert check_bytes(L, "markov + 200 KB noise w16", d, params)


def test_pieces_beyond_the_window(L):
    d = alphabet64_then_text()
    params = [(Q, 5), (W, 22), (SH, len(d))]
    _, st = emu.encode_stream(L, d, params, segment_bytes=4096)
    assert st["uncompressed_metablocks"] == 0  # (the runs are inside compressed meta-blocks)
    assert check_bytes(L, "64 symbols + text", d, params)


@pytest.mark.parametrize("quality", [2, 3, 4, 9])
def test_other_qualities(L, quality):
    d = synth.mixed(256 << 10)
    assert check_bytes(L, "mixed 256 KiB q%d" % quality, d, [(Q, quality), (W, 22), (SH, len(d))])
    a = synth.alice()
    assert check_bytes(L, "alice q%d" % quality, a, [(Q, quality), (W, 18)])


def test_quality_10(L):
    a = synth.alice()[:16 << 10]
    assert check_bytes(L, "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))])


def test_quality_9_5(L):
    a = synth.alice()[:64 << 10]
    assert check_bytes(L, "alice 64 KiB q9.5", a, [(Q, 10), (Q9_5, 1), (W, 22), (SH, len(a))])


@pytest.mark.parametrize("length", STATS_LENGTHS)
def test_context_statistics_sample_counts(L, length):
    d = markov_1m()[:length]
    assert len(d) == length
    assert check_bytes(L, "markov %d" % length, d, [(Q, 5), (W, 22), (SH, length)])


def test_header_composed_in_global_memory(L):
    # k_write_headers: the prefix codes of the one meta-block exceed what the workgroup-memory buffer is sized for (header_cases.py)
    d = header_cases.input_above()
    assert check_bytes(L, "256 regimes x 6000", d, header_cases.params(d))


def test_largest_header_composed_in_workgroup_memory(L):
    d = header_cases.input_below()
    assert check_bytes(L, "256 regimes x 2800", d, header_cases.params(d))


_SELFTEST_CHILD = """
import sys
sys.path.insert(0, %r)
import gpulib, synth, test_metablock_emit_gpu as t
from cmp_stream import check_bytes
L = gpulib.lib()
Q, W, SH = 1, 2, 5
d = t.markov_1m()
assert check_bytes(L, "markov 1 MiB w16", d, [(Q, 5), (W, 16), (SH, len(d))])
d = t.markov_with_noise()
assert check_bytes(L, "markov + noise w16", d, [(Q, 5), (W, 16), (SH, len(d))])
d = t.alphabet64_then_text()
assert check_bytes(L, "64 symbols + text", d, [(Q, 5), (W, 22), (SH, len(d))])
a = synth.alice()[:16 << 10]
assert check_bytes(L, "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))])
for n in t.STATS_LENGTHS:
    assert check_bytes(L, "markov %%d" %% n, t.markov_1m()[:n], [(Q, 5), (W, 22), (SH, n)])
print("selftest ok")
"""


def test_selftest_compares_with_the_piecewise_emission():
    env = dict(os.environ, BROTLI_MI355X_SELFTEST="1")
    r = subprocess.run([sys.executable, "-c", _SELFTEST_CHILD % HERE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
