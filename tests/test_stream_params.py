"""The stream parameters that change the bytes, beyond quality, lgwin, size hint and the framing bits: BROTLI_PARAM_LGBLOCK (3),
BROTLI_PARAM_LITERAL_BYTE_SCORE (154), BROTLI_PARAM_MODE (0: FONT and the forced context modes), BROTLI_PARAM_DISABLE_LITERAL_CONTEXT_MODELING
(4) and BROTLI_PARAM_BARE_STREAM (173), on the main path: one FINISH, the one-shot and multi-shard entries, chunks, streams with
flushes and a custom dictionary.  The reference's setter takes all of them (encode.rs:196-286), so a user of its bindings can
set them.

Every case is written once and runs twice: on the emulation build (the host plan and the chain code compiled for the CPU) and,
marked gpu, on the product library.  Expected bytes always come from the oracle.

No identity case is empty: it first asserts, on the oracle alone, that every parameter under test changes the oracle's bytes for
the chosen input -- each one dropped in turn, so that none rides on another.  A parameter that does not matter there fails the
case; nothing in this file skips.  Where the oracle shows that a parameter changes nothing (a set lgblock and FONT at qualities 2
and 3, FONT at quality "9.5"), a case of its own asserts exactly that, on the oracle and on the product."""
import functools
import os

import pytest

import emu
import orc
import synth
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MODE, Q, W, LGB, NOCTX, SH, LARGE, Q9_5, LBS, BARE = 0, 1, 2, 3, 4, 5, 6, 150, 154, 173
FONT = (MODE, 2)


# ---- inputs and oracle streams, computed once per process and shared

@functools.lru_cache(maxsize=None)
def _input(name):
    if name == "alice":
        return synth.alice()
    if name == "alice40k":
        return synth.alice()[:40000]
    if name == "alice100k":
        return synth.alice()[:100000]
    if name == "mixed":
        return synth.mixed(600000, 7)
    if name == "markov":
        return synth.markov_text(400000, 5)
    if name == "markov5M":
        return synth.markov_text(5 << 20)
    if name == "markov1.5M":
        return synth.markov_text(3 << 19, 5)
    if name == "rtu":
        return open(os.path.join(GOLDEN, "random_then_unicode"), "rb").read()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, params):
    return orc.stream_compress(_input(name), list(params))[0]


def _library(kind):
    """the library behind emu.encode_stream: the emulation build or the product"""
    if kind == "emu":
        return emu.lib()
    import gpulib
    return gpulib.lib()


def _decode(comp, size, params):
    return orc.decompress_large_window(comp, size) if (LARGE, 1) in params else orc.decompress(comp, size)


def _first_difference(got, want):
    i = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "first difference at byte %d (sizes %d and %d)" % (i, len(got), len(want))


# ---- 1. identity with the oracle, one FINISH
#
# A case: (input, base parameters, the parameters under test, segment size).  The guard compares the oracle under base + under test
# with the oracle under the same list less one parameter under test, for each of them.

def _case(name, base, under_test, seg=4096):
    return pytest.param(name, tuple(base), tuple(under_test), seg,
                        id="%s-%s+%s%s" % (name, "_".join("%d=%d" % kv for kv in base), "_".join("%d=%d" % kv for kv in under_test),
                                           "" if seg == 4096 else "-seg%d" % seg))


def _identity_cases():
    cases = []
    # qualities 4, 5 and 7 (quick_device.h at 4, H5 at 5 and 7) on 600 000 bytes: two whole blocks and a ragged one at lgblock 18,
    # four and a ragged one at lgblock 17, one block at lgblock 24
    for q in (4, 5, 7):
        base = [(Q, q), (W, 22)]
        for lgblock in (17, 18, 24):
            cases.append(_case("mixed", base, [(LGB, lgblock)]))
        cases.append(_case("mixed", base, [FONT]))
        for mode in (3, 6):
            cases.append(_case("mixed", base, [(MODE, mode)]))
        for score in (1, 100, 340, 1000):
            cases.append(_case("mixed", base, [(LBS, score)]))
        cases.append(_case("mixed", base, [(BARE, 1)]))
    # lgblock above lgwin: the ring is 1 << (1 + lgblock) bytes (encode.rs:587-601), the positions go past its first lap; lgwin 16
    # is the H6 family the reference falls through to (encoder_params.h)
    for q in (5, 8):
        cases.append(_case("mixed", [(Q, q), (W, 16)], [(LGB, 18)]))
    # segment edges and block edges coincide
    cases.append(_case("mixed", [(Q, 5), (W, 22)], [(LGB, 17)], seg=512))
    # H6 (size hint above 4 MiB) and H54 (quality 4 with a size hint of 1 MiB and more)
    cases.append(_case("markov5M", [(Q, 5), (W, 22), (SH, 5 << 20)], [(LGB, 18), FONT]))
    cases.append(_case("markov1.5M", [(Q, 4), (W, 22), (SH, 3 << 19)], [(LGB, 18), FONT]))
    # FONT under large_window: a distance alphabet of 16 + 12 + (62 << 2) = 276 symbols
    for q in (5, 9):
        cases.append(_case("mixed", [(Q, q), (LARGE, 1), (W, 28), (SH, 600000)], [FONT]))
    for q in (7, 9):
        cases.append(_case("rtu", [(Q, q), (W, 22)], [(NOCTX, 1)]))
    # quality 9 (H9): the default lgblock is 18 there
    base = [(Q, 9), (W, 22)]
    for lgblock in (16, 17, 20):
        cases.append(_case("markov", base, [(LGB, lgblock)]))
    for under_test in ([FONT], [(MODE, 3)], [(LBS, 340)], [(BARE, 1)]):
        cases.append(_case("markov", base, under_test))
    # quality "9.5": the quality >= 10 meta-block builder behind the greedy search.  FONT changes nothing there, alone or beside
    # another parameter (its distance-parameter search chooses again): it sits in the base here, and _NO_EFFECT below has it
    for q in (10, 11):
        base = [(Q, q), (Q9_5, 1), (W, 22)]
        cases.append(_case("alice", base, [(LGB, 16)]))
        cases.append(_case("alice", base + [FONT], [(NOCTX, 1)]))
        cases.append(_case("alice", base, [(LBS, 340)]))
    # qualities 10 and 11 proper (H10 + Zopfli): short inputs, the device runs these at a few hundredths of a MB/s; the literal
    # byte score plays no part there.  No lgblock above 18 at quality 11: the match array is 128 * block_bytes eight-byte words.
    for q in (10, 11):
        base = [(Q, q), (W, 22)]
        cases.append(_case("alice40k", base, [FONT]))
        cases.append(_case("alice40k", base, [(NOCTX, 1)]))
        cases.append(_case("alice40k", [(Q, q), (LARGE, 1), (W, 26)], [FONT]))
        cases.append(_case("alice100k", base, [(LGB, 16)]))  # two blocks where the default gives one
    return cases


_IDENTITY = _identity_cases()


def _identity(kind, name, base, under_test, seg):
    data = _input(name)
    params = base + under_test
    want = _oracle(name, params)
    for one in under_test:
        rest = tuple(x for x in params if x != one)
        assert want != _oracle(name, rest), "the case is empty: %r changes nothing in the oracle's stream of %s under %r" % (one, name, rest)
    got, _ = emu.encode_stream(_library(kind), data, list(params), segment_bytes=seg)
    assert got == want, _first_difference(got, want)
    if (BARE, 1) not in params:  # (a bare stream has no header to decode from)
        assert _decode(got, len(data), params) == data


@pytest.mark.parametrize("name,base,under_test,seg", _IDENTITY)
def test_identity_emu(name, base, under_test, seg):
    _identity("emu", name, base, under_test, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("name,base,under_test,seg", _IDENTITY)
def test_identity_gpu(name, base, under_test, seg):
    _identity("gpu", name, base, under_test, seg)


# What the oracle says of a parameter, asserted either way, and the product must agree: (input, base, parameter, whether it changes
# the oracle's bytes).
# Qualities 2 and 3: ComputeLgBlock forces lgblock 14 (encode.rs:570-585), so a set lgblock changes nothing; ChooseDistanceParams
# leaves the distance code alone below quality 4 (encode.rs:2169-2190) and there is no context modelling, so FONT changes nothing
# either.  The literal byte score does scale the match scores.
_LOW = [pytest.param("alice", ((Q, q), (W, 22)), one, changes, id="q%d+%d=%d" % ((q,) + one))
        for q in (2, 3) for one, changes in ((FONT, False), ((LBS, 100), True), ((LGB, 18), False))]
# Quality "9.5": the builder's distance-parameter search (metablock.rs:133-307) chooses npostfix and ndirect again whatever the
# mode set, so FONT changes nothing -- beside DISABLE_LITERAL_CONTEXT_MODELING, and under large_window at lgwin 26, where it would
# have been the 276-symbol distance code.  (Both were proposed as identity cases; the oracle shows them empty with respect to
# FONT, so they assert that instead.)
_FONT_AT_9_5 = [pytest.param("alice", base, FONT, False, id="q%d%s+font" % (q, tag))
                for q in (10, 11) for tag, base in (("-noctx", ((Q, q), (Q9_5, 1), (W, 22), (NOCTX, 1))),
                                                    ("-large-w26", ((Q, q), (Q9_5, 1), (LARGE, 1), (W, 26))))]


def _as_the_oracle_says(kind, name, base, one, changes):
    data = _input(name)
    params = base + (one,)
    want = _oracle(name, params)
    assert (want != _oracle(name, base)) == changes, "the oracle says otherwise about %r under %r" % (one, base)
    got, _ = emu.encode_stream(_library(kind), data, list(params), segment_bytes=4096)
    assert got == want, _first_difference(got, want)
    if not changes:
        default, _ = emu.encode_stream(_library(kind), data, list(base), segment_bytes=4096)
        assert got == default
    assert _decode(got, len(data), params) == data


@pytest.mark.parametrize("name,base,one,changes", _LOW)
def test_qualities_2_3_emu(name, base, one, changes):
    _as_the_oracle_says("emu", name, base, one, changes)


@pytest.mark.gpu
@pytest.mark.parametrize("name,base,one,changes", _LOW)
def test_qualities_2_3_gpu(name, base, one, changes):
    _as_the_oracle_says("gpu", name, base, one, changes)


@pytest.mark.parametrize("name,base,one,changes", _FONT_AT_9_5)
def test_font_at_quality_9_5_emu(name, base, one, changes):
    _as_the_oracle_says("emu", name, base, one, changes)


@pytest.mark.gpu
@pytest.mark.parametrize("name,base,one,changes", _FONT_AT_9_5)
def test_font_at_quality_9_5_gpu(name, base, one, changes):
    _as_the_oracle_says("gpu", name, base, one, changes)


# ---- 2. through the C ABI

_ONE_SHOT = [(q, mode) for q in (4, 5, 9) for mode in (2, 3)]


def _one_shot(kind, q, mode):
    a = _input("alice")
    want = orc.compress(a, q, 22, mode)
    assert want != orc.compress(a, q, 22), "the case is empty: mode %d changes nothing at quality %d" % (mode, q)
    got = test_cabi._load(kind).compress(a, q, 22, mode)
    assert got == want, _first_difference(got, want)
    assert orc.decompress(got, len(a)) == a


@pytest.mark.parametrize("q,mode", _ONE_SHOT)
def test_one_shot_mode_emu(q, mode):
    _one_shot("emu", q, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("q,mode", _ONE_SHOT)
def test_one_shot_mode_gpu(q, mode):
    _one_shot("gpu", q, mode)


# BrotliEncoderCompressMulti: (base, under test, shards)
_MULTI = [pytest.param(tuple(base), tuple(under_test), shards, id="%s+%s-x%d" % ("_".join("%d=%d" % kv for kv in base), "_".join("%d=%d" % kv for kv in under_test), shards))
          for base, under_test, shards in (([(Q, 5)], [FONT], 3),
                                           ([(Q, 7), (W, 18)], [(LGB, 17)], 4),
                                           ([(Q, 4), (W, 20)], [FONT, (LGB, 18)], 2),
                                           ([(Q, 9)], [(LBS, 340)], 3))]


def _multi(kind, base, under_test, shards):
    d = _input("mixed")
    params = list(base + under_test)
    want = orc.compress_multi(d, params, shards)
    for one in under_test:
        assert want != orc.compress_multi(d, [x for x in params if x != one], shards), "the case is empty: %r" % (one,)
    got = bytes(test_cabi._load(kind).BrotliCompress(d, params, shards))
    assert got == want, _first_difference(got, want)
    assert orc.decompress(got, len(d)) == d


@pytest.mark.parametrize("base,under_test,shards", _MULTI)
def test_multi_emu(base, under_test, shards):
    _multi("emu", base, under_test, shards)


@pytest.mark.gpu
@pytest.mark.parametrize("base,under_test,shards", _MULTI)
def test_multi_gpu(base, under_test, shards):
    _multi("gpu", base, under_test, shards)


def _chunks(kind):
    """BrotliMi355xCompressChunk + BrotliMi355xConcatChunks (one chunk per process in the multi-GPU run): the stream of the
    multi-shard entry"""
    lib = test_cabi._load(kind)
    d = _input("mixed")
    params = [(Q, 5), FONT, (LGB, 17)]
    want = orc.compress_multi(d, params, 4)
    for one in params[1:]:
        assert want != orc.compress_multi(d, [x for x in params if x != one], 4), "the case is empty: %r" % (one,)
    got = lib.concat_chunks([lib.compress_chunk(d, len(d), t, 4, params) for t in range(4)])
    assert got == want, _first_difference(got, want)
    assert orc.decompress(got, len(d)) == d


def test_chunks_emu():
    _chunks("emu")


@pytest.mark.gpu
def test_chunks_gpu():
    _chunks("gpu")


# Streams with BROTLI_OPERATION_FLUSH.  The cuts sit on, one past and far from the block edge of lgblock 17 (131 072 bytes); the
# writes between two flushes are PROCESS calls of write_size bytes (0: everything in the flushing call).
_FLUSH_PARAMS = ([(Q, 5), (W, 22), (LGB, 17)],
                 [(Q, 6), (W, 16), (LGB, 18)],
                 [(Q, 4), (W, 18), (LGB, 17), FONT],
                 [(Q, 9), (W, 20), (LGB, 20)],
                 [(Q, 5), (W, 22), FONT, (LBS, 340), (NOCTX, 1)])
_FLUSH_SHAPES = (([131072, 131073, 400000], 0), ([100000, 262144], 4096), ([], 65536), ([300000], 100000))
_FLUSHES = [pytest.param(tuple(params), tuple(cuts), write_size, id="%s-cuts%s-w%d" % ("_".join("%d=%d" % kv for kv in params), "_".join(str(c) for c in cuts) or "none", write_size))
            for params in _FLUSH_PARAMS for cuts, write_size in _FLUSH_SHAPES]


def _write_and_flush(lib, data, params, cuts, write_size, dictionary=None):
    """the product's side of orc.stream_with_flushes"""
    e = lib.encoder(params=list(params), dictionary=dictionary)
    pieces, pos = [], 0
    for cut in list(cuts) + [len(data)]:
        if write_size:
            while cut - pos > write_size:
                e.write(data[pos:pos + write_size])
                pos += write_size
        if len(pieces) < len(cuts):
            pieces.append(e.flush(data[pos:cut]))
        else:
            pieces.append(e.finish(data[pos:cut]))  # BROTLI_OPERATION_FINISH with the rest of the input
        pos = cut
    e.close()
    return pieces


def _flushes(kind, params, cuts, write_size):
    d = _input("mixed")
    want = orc.stream_with_flushes(d, list(params), list(cuts), write_size=write_size)
    got = _write_and_flush(test_cabi._load(kind), d, params, cuts, write_size)
    assert [len(p) for p in got] == [len(p) for p in want]
    assert got == want
    assert orc.decompress(b"".join(got), len(d)) == d


@pytest.mark.parametrize("params,cuts,write_size", _FLUSHES)
def test_flushes_emu(params, cuts, write_size):
    _flushes("emu", params, cuts, write_size)


@pytest.mark.gpu
@pytest.mark.parametrize("params,cuts,write_size", _FLUSHES)
def test_flushes_gpu(params, cuts, write_size):
    _flushes("gpu", params, cuts, write_size)


def _dictionary_and_flush(kind):
    """a custom dictionary in front of a flushed stream (such a stream needs the dictionary to decode: no round trip here)"""
    a = _input("alice")
    dic, d = a[:20000], a[20000:]
    params = [(Q, 5), (LGB, 17), FONT]
    want = orc.stream_with_flushes(d, params, [70000], dictionary=dic)
    for one in params[1:]:
        assert want != orc.stream_with_flushes(d, [x for x in params if x != one], [70000], dictionary=dic), "the case is empty: %r" % (one,)
    got = _write_and_flush(test_cabi._load(kind), d, params, [70000], 0, dictionary=dic)
    assert got == want


def test_dictionary_and_flush_emu():
    _dictionary_and_flush("emu")


@pytest.mark.gpu
def test_dictionary_and_flush_gpu():
    _dictionary_and_flush("gpu")


# ---- 3. the setter's contract (host code: the emulation build links the same encoder_params.cpp and cabi.cpp)

# the arms of the reference's match (encode.rs:203-282; everything else: `_ => return false`, :283).  Ids 7 and 8 (NPOSTFIX,
# NDIRECT), 163 and 170 (NO_DICTIONARY) have no arm, although the C header's enum names 7, 8 and 170.
ACCEPTED_IDS = (0, 1, 2, 3, 4, 5, 6,
                150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162,
                164, 165, 166, 167, 168, 169,
                171, 172, 173)
# of those, the ones that only drive the reference's optional prior / IR research code
RESEARCH_KNOBS = (152, 153, 155, 156, 157, 158, 159, 160, 161, 162, 164, 165, 166)


def test_setter_accepts_the_ids_of_the_reference():
    lib = test_cabi._load("emu")
    for pid in range(256):
        e = lib.encoder()
        assert e.set_parameter(pid, 1) == (pid in ACCEPTED_IDS), pid
        e.close()
    for pid in (7, 8, 163, 170):
        assert pid not in ACCEPTED_IDS
    # DISABLE_LITERAL_CONTEXT_MODELING takes 0 and 1 only (encode.rs:255-260)
    e = lib.encoder()
    assert e.set_parameter(NOCTX, 0) and e.set_parameter(NOCTX, 1)
    assert not e.set_parameter(NOCTX, 2)
    # everything is refused once the stream has started (encode.rs:289-295)
    e.set_parameter(Q, 5)
    e.write(b"started")
    for pid in range(256):
        assert not e.set_parameter(pid, 1), pid
    e.finish()
    for pid in ACCEPTED_IDS:
        assert not e.set_parameter(pid, 0), pid
    e.close()


@pytest.mark.parametrize("pid", RESEARCH_KNOBS)
def test_research_knobs_leave_the_bytes_alone(pid):
    """encoder_params.h: "research knobs of the reference that never change the default output; stored, not acted upon".  The
    oracle refuses these ids, so the product is compared with itself here: the default's stream, which test_cabi pins on the
    oracle."""
    lib = test_cabi._load("emu")
    a = _input("alice")

    def stream(params):
        e = lib.encoder(params=params)
        e.write(a)
        got = e.finish()
        e.close()
        return got

    default = stream([(Q, 5), (W, 22)])
    assert default == _oracle("alice", ((Q, 5), (W, 22)))
    for value in (1, 7):
        assert stream([(Q, 5), (W, 22), (pid, value)]) == default, (pid, value)
