"""Texts made of the static dictionary's words under its transforms, and what a stream says about them.  Test infrastructure only.

The words and the transforms come from libbrotlicommon (brotli_parse._Tables.word), not from the tables of the library under test."""
import functools

import numpy as np

import brotli_parse

NUM_TRANSFORMS = 121
# the transforms BrotliFindAllStaticDictionaryMatches cannot find (static_dict.rs:309-1300 has no test for them): the omit-first ones
OMIT_FIRST = (3, 11, 26, 34, 39, 40, 54, 55)
CASCADE = tuple(t for t in range(NUM_TRANSFORMS) if t not in OMIT_FIRST)  # 113
# what SearchInStaticDictionary of qualities 5 .. 9 can produce: the word as it is, and with its last 1 .. 9 bytes left out
HASH_SEARCH = (0, 12, 27, 23, 42, 63, 56, 48, 59, 64)
WORD_LENGTHS = tuple(range(4, 25))


def tables():
    return brotli_parse._Tables.get()


@functools.lru_cache(maxsize=None)
def word(length, index, transform):
    return tables().word(length, index, transform)


def decode_match(m):
    """(length code, index, transform) of an entry (distance << 5 | length code) of BrotliFindAllStaticDictionaryMatches"""
    T = tables()
    len_code = m & 31
    distance = m >> 5
    bits = T.size_bits[len_code]
    return len_code, distance & ((1 << bits) - 1), distance >> bits


@functools.lru_cache(maxsize=None)
def stream_text(size=12288, seed=20261):
    """`size` bytes of transform(word) for the 113 transforms the dictionary search knows, all word lengths, with a short separator
    between two of them"""
    T = tables()
    rng = np.random.default_rng(seed)
    seps = (b"", b"", b"\n", b"#", b"7", b"@@")
    cells = [(t, l) for t in CASCADE for l in WORD_LENGTHS]
    out = bytearray()
    while len(out) < size:
        for c in rng.permutation(len(cells)):
            t, l = cells[c]
            out += word(l, int(rng.integers(0, 1 << T.size_bits[l])), t)
            out += seps[int(rng.integers(0, len(seps)))]
            if len(out) >= size:
                break
    return bytes(out[:size])


def dictionary_references(stream):
    """(number of dictionary references, set of their transforms) of a stream: a command whose distance exceeds min(position, max
    backward) copies a word, and its transform is word id >> size_bits[copy length]"""
    T = tables()
    p = brotli_parse.parse(stream)
    max_backward = (1 << p["wbits"]) - 16
    count, transforms = 0, set()
    for mb in p["metablocks"]:
        for insert_len, copy_len, _, distance, cmd_pos in mb.get("cmds", ()):
            if copy_len == 0:
                continue
            reach = min(cmd_pos + insert_len, max_backward)
            if distance > reach:
                count += 1
                transforms.add((distance - reach - 1) >> T.size_bits[copy_len])
    return count, transforms


Q, W = 1, 2  # BROTLI_PARAM_QUALITY, BROTLI_PARAM_LGWIN


def stream_params(quality):
    return [(Q, quality), (W, 22)]


@functools.lru_cache(maxsize=None)
def oracle_stream(quality):
    """The oracle's stream of stream_text() at `quality` (its stream entry, the parameters of stream_params), after the condition that
    makes the input worth sending, asserted on that stream alone: it is full of dictionary references.
      qualities 10 and 11: at least 400 references over at least 100 distinct transforms.  The oracle gives 677 references over all 113
        transforms at quality 11 and 663 over 112 at quality 10 -- through the stream entry, which runs quality 10 with the Zopfli
        parse; its one-shot entry runs quality 10 with the parse of quality 9 and gives 356 over 10 -- where alice29.txt reaches 79
        transforms in the match finder and fewer in the stream.
      qualities 5 and 9: at least 200 references over exactly the ten transforms SearchInStaticDictionary (lz77_chain.h) can produce,
        the word as it is and with its last 1 .. 9 bytes left out.  The oracle gives 357 and 356."""
    import orc
    data = stream_text()
    stream, _ = orc.stream_compress(data, stream_params(quality))
    assert orc.decompress(stream, len(data)) == data
    count, transforms = dictionary_references(stream)
    if quality >= 10:
        assert count >= 400 and len(transforms) >= 100, (quality, count, sorted(transforms))
        assert transforms <= set(CASCADE)
    else:
        assert count >= 200 and transforms == set(HASH_SEARCH), (quality, count, sorted(transforms))
    return stream


def check_streams(L, qualities):
    """stream_text() through the library at every quality: byte identity with the oracle (cmp_stream.check_bytes, as the neighbouring
    stream cases have it); the round trip of that stream through the independent decoder is part of oracle_stream"""
    from cmp_stream import check_bytes
    data = stream_text()
    for q in qualities:
        oracle_stream(q)  # (the condition first)
        assert check_bytes(L, "dictionary words q%d" % q, data, stream_params(q)), q
