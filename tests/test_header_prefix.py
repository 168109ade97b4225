"""The meta-block header in two items (mb_item_header_prefix, mb_item_header_trees), on the emulation: composed one behind the other
they give the header of before -- the emulation's streams against the oracle say so on every input of the suite.  Here the seam itself:
the bit position the prefix item leaves in header_prefix_bits[m] is where the oracle's stream starts its first prefix code, counted
from the start of the meta-block (brotli_parse), and it is never beyond header_bits[m].  With the streams byte-identical, the prefix
words are then a bit prefix of the header.

The encoder prints both figures per meta-block under BROTLI_MI355X_DEBUG_MB (a child process: the variable is read at the call)."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = r"""
import sys
sys.path.insert(0, %(tests)r)
import emu, orc, synth, brotli_parse
import test_header_prefix as t
L = emu.lib()
name, data, params = t.CASES[%(case)d]()
out, st = emu.encode_stream(L, data, params, segment_bytes=4096)
want, _ = orc.stream_compress(data, params)
assert out == want, (name, len(out), len(want))
mb = [m for m in brotli_parse.parse(want, first_header_only=True)["metablocks"] if "nbltypes" in m][0]
header = mb["data_bit_offset"] - mb["bit_offset"]
print("ORACLE first compressed meta-block: header %%d bits, %%d in front of the trees" %% (header, header - sum(sum(c) for c in mb["code_bits"])))
"""

Q, W, NOCTX, SH = 1, 2, 4, 5


def _alice():
    import synth
    a = synth.alice()
    return "alice", a, [(Q, 5), (W, 22), (SH, len(a))]


def _zeros():
    return "zeros", bytes(300000), [(Q, 5), (W, 22)]


def _mixed():
    import synth
    d = synth.mixed(256 << 10)
    return "mixed 256 KiB", d, [(Q, 5), (W, 22), (SH, len(d))]


def _markov_13_contexts():
    import synth
    d = synth.markov_text(1 << 20)
    return "markov 1 MiB", d, [(Q, 5), (W, 22), (SH, len(d))]


def _mixed_q2():
    import synth
    d = synth.mixed(256 << 10)
    return "mixed 256 KiB q2", d, [(Q, 2), (W, 22), (SH, len(d))]


def _alice_q10():
    import synth
    a = synth.alice()[:16 << 10]
    return "alice 16 KiB q10", a, [(Q, 10), (W, 22), (SH, len(a))]


CASES = [_alice, _zeros, _mixed, _markov_13_contexts, _mixed_q2, _alice_q10]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c.__name__.strip("_") for c in CASES])
def test_prefix_ends_where_the_oracles_trees_begin(case):
    env = dict(os.environ, BROTLI_MI355X_DEBUG_MB="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(tests=HERE, case=case)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    ours = [(int(h), int(p)) for h, p in re.findall(r"header (\d+) bits, (\d+) in front of the trees", r.stderr)]
    oracle = re.search(r"ORACLE first compressed meta-block: header (\d+) bits, (\d+) in front of the trees", r.stdout)
    assert ours and oracle, r.stdout[-1000:] + r.stderr[-2000:]
    for header_bits, prefix_bits in ours:
        assert prefix_bits <= header_bits, ours
    compressed = [x for x in ours if x[0] != 0]  # (a stored meta-block has neither)
    assert compressed[0] == (int(oracle.group(1)), int(oracle.group(2))), (compressed[0], oracle.groups())
    assert 0 < compressed[0][1] < compressed[0][0]
