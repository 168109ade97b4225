"""Inputs that put k_write_headers on either side of its threshold: a meta-block's header is composed in workgroup memory unless
its serialised prefix codes exceed 5120 * 64 - 160 * 1024 = 163 840 bits, above that in global memory.

The input is a sequence of regimes: every segment draws its bytes from its own permutation of all 256 values with weights u ** 8
(u uniform), so the block splitter gives (nearly) every segment a literal block type of its own -- 256 literal codes of about 250
used symbols with scattered depths -- and the last 8 of every 200 bytes repeat the 8 before them, so the encoder sees enough
commands not to store the meta-block.  Below 2 Mi literals at lgwin 24 the whole input is ONE meta-block.

tree_bits() takes its figure from the ORACLE's stream alone (tests/brotli_parse.py): the sum over the literal, command and distance
prefix codes as they stand in the header, which is what the kernel adds up (tree_nbits of every histogram row)."""
import functools

import numpy as np

import brotli_parse
import orc

Q, W, SH = 1, 2, 5
THRESHOLD_BITS = 5120 * 64 - 160 * 1024
# name -> (segments, bytes per segment); the oracle's figures: 181 685 bits (+10.9 %) and 158 173 bits (-3.5 %)
CASES = {"above": (256, 6000), "below": (256, 2800)}


@functools.lru_cache(maxsize=None)
def regimes(segments, segment_bytes, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(segments):
        perm = rng.permutation(256)
        w = rng.random(256) ** 8
        seg = perm[rng.choice(256, size=segment_bytes, p=w / w.sum())].astype(np.uint8)
        rows = seg[:segment_bytes // 200 * 200].reshape(-1, 200)
        rows[:, 192:] = rows[:, 184:192]
        out.append(seg)
    return np.concatenate(out).tobytes()


def params(data):
    return [(Q, 9), (W, 24), (SH, len(data))]


@functools.lru_cache(maxsize=None)
def tree_bits(name):
    """(input, bits of all prefix codes of the oracle's one meta-block)"""
    data = regimes(*CASES[name])
    assert len(data) <= 4 << 20
    stream, _ = orc.stream_compress(data, params(data))
    mb = brotli_parse.parse(stream, first_header_only=True)["metablocks"]
    # the first meta-block is compressed, is the last one and holds the whole input: there is no other
    assert len(mb) == 1 and not mb[0]["uncompressed"] and mb[0]["is_last"] and mb[0]["mlen"] == len(data), (len(mb), mb[0].get("mlen"))
    codes = mb[0]["code_bits"]
    assert [len(c) for c in codes] == [mb[0]["ntrees_l"], mb[0]["nbltypes"][1], mb[0]["ntrees_d"]]
    return data, sum(sum(c) for c in codes)


def input_above():
    data, bits = tree_bits("above")
    print("prefix codes of the meta-block: %d bits (threshold %d)" % (bits, THRESHOLD_BITS))
    assert bits >= THRESHOLD_BITS * 1.05, bits  # composed in global memory, with a margin of 5 %
    return data


def input_below():
    data, bits = tree_bits("below")
    print("prefix codes of the meta-block: %d bits (threshold %d)" % (bits, THRESHOLD_BITS))
    assert THRESHOLD_BITS * 0.9 <= bits <= THRESHOLD_BITS, bits  # the largest header that is still composed in workgroup memory
    return data
