"""The front end of the LZ77 stage on the product library -- the key pass (k_compute_keys: a persistent grid, the static
dictionary's hash table in LDS, four positions per lane) and the dry runs in front of round 0 -- byte identity with the oracle on
the shapes where this code can go wrong.

Segments: inputs of one, two and three segments at the library's own segment size (256 bytes up to 512 KiB: no dry run at all, one
dry run, the first entry that builds on a guessed one), and 65 536 + 10 bytes, whose second block is shorter than the dry run and
than the hash length.  Zeros: a copy reaches the end of every block.  Random data: no command anywhere, the literal spree runs
through whole blocks and the forecast finds the static dictionary's death early.  A mix: stretches without commands begin and end
inside blocks.  Text with the size hint (H6) and without it, alice29 on the rank path of quality 9, and a stream in two pieces
(carried distance cache and dictionary counters).  Key pass: a workgroup steps through 4096 positions and the grid (two workgroups
per CU, 512 on an MI355X) through 2 MiB, so lengths just behind a multiple of either with n mod 16 of 1, 7 and 15, the short
lengths in front of the first full group of four, and the 16-bit keys of quality 10.  Everything is cut at the library's own
segment size (seg=0).  The groups run once more in a child process under BROTLI_MI355X_SELFTEST=1, where the stage compares all 16
words of every entry the device composed, and its forecast, with the host's WarmupEnd and forecast on the same exits, and the
first three groups once with BROTLI_MI355X_HOST_WARMUP=1, which keeps the host path alive."""
import functools
import os
import subprocess
import sys

import pytest

import synth
import test_streaming
import cmp_stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Q, W, SH = 1, 2, 5
SEGMENTS = [256, 512, 768, 65536 + 10]
KEY_LENGTHS = [1, 3, 5, 4095, 4096, 4097, 4096 * 3 + 1, 4096 * 3 + 7, 4096 * 3 + 15]
GRID_LAPS = [(2 << 20) + 1, (2 << 20) + 7, (2 << 20) + 15]


def check_bytes(L, name, data, params):
    return cmp_stream.check_bytes(L, name, data, params, seg=0)


@pytest.fixture(scope="module")
def L():
    import gpulib
    return gpulib.lib()


@functools.lru_cache(maxsize=None)
def markov():
    return synth.markov_text((2 << 20) + 15)


@pytest.mark.parametrize("length", SEGMENTS)
def test_segment_counts(L, length):
    assert check_bytes(L, "markov %d" % length, markov()[:length], [(Q, 5), (W, 22)])


def test_zeros_copy_reaches_every_block_end(L):
    assert check_bytes(L, "zeros 200000", bytes(200000), [(Q, 5), (W, 22)])


@pytest.mark.parametrize("size", [256 << 10, 4 << 20])
def test_random_no_command_anywhere(L, size):
    assert check_bytes(L, "random %d" % size, synth.random_bytes(size), [(Q, 5), (W, 22)])


def test_mixed_runs_without_commands_inside_blocks(L):
    assert check_bytes(L, "mixed 1 MiB", synth.mixed(1 << 20), [(Q, 5), (W, 22)])


@pytest.mark.parametrize("hinted", [True, False])
def test_text(L, hinted):
    n = (1 << 20) + 4097
    assert check_bytes(L, "markov %d%s" % (n, " hinted" if hinted else ""), markov()[:n], [(Q, 5), (W, 22)] + ([(SH, n)] if hinted else []))


def test_rank_path_quality_9(L):
    assert check_bytes(L, "alice q9", synth.alice(), [(Q, 9), (W, 22)])


def test_stream_in_two_pieces():
    test_streaming._run("gpu", [("markov 200000 q5 w16 in two writes", "synth.markov_text(200000, 3)", 5, 16, 100000, 0, False)], 100000,
                        flush_part=False)


@pytest.mark.parametrize("length", KEY_LENGTHS)
def test_key_pass_lengths(L, length):
    assert check_bytes(L, "markov %d keys" % length, markov()[:length], [(Q, 5), (W, 22)])


@pytest.mark.parametrize("length", GRID_LAPS)
def test_key_pass_second_lap_of_the_grid(L, length):
    assert check_bytes(L, "markov %d keys" % length, markov()[:length], [(Q, 5), (W, 22), (SH, length)])


def test_key_pass_quality_10(L):
    a = synth.alice()[:16 << 10]
    assert check_bytes(L, "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))])


_CHILD = """
import sys
sys.path.insert(0, %r)
import gpulib, synth, test_warmup_entries_gpu as t
from test_warmup_entries_gpu import check_bytes
L = gpulib.lib()
Q, W, SH = 1, 2, 5
everything = %r
for n in t.SEGMENTS + (t.KEY_LENGTHS if everything else []):
    assert check_bytes(L, "markov %%d" %% n, t.markov()[:n], [(Q, 5), (W, 22)])
assert check_bytes(L, "zeros 200000", bytes(200000), [(Q, 5), (W, 22)])
assert check_bytes(L, "random 256 KiB", synth.random_bytes(256 << 10), [(Q, 5), (W, 22)])
assert check_bytes(L, "random 4 MiB", synth.random_bytes(4 << 20), [(Q, 5), (W, 22)])
if everything:
    assert check_bytes(L, "mixed 1 MiB", synth.mixed(1 << 20), [(Q, 5), (W, 22)])
    n = (1 << 20) + 4097
    assert check_bytes(L, "markov hinted", t.markov()[:n], [(Q, 5), (W, 22), (SH, n)])
    assert check_bytes(L, "markov unhinted", t.markov()[:n], [(Q, 5), (W, 22)])
    assert check_bytes(L, "alice q9", synth.alice(), [(Q, 9), (W, 22)])
print("child ok")
"""


def _child(everything, **extra):
    env = dict(os.environ, **extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % (HERE, everything)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_selftest_compares_the_entries_with_the_hosts():
    _child(True, BROTLI_MI355X_SELFTEST="1")


def test_host_switch_keeps_the_host_path_alive():
    _child(False, BROTLI_MI355X_HOST_WARMUP="1")
