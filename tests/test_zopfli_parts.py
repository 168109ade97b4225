"""The static dictionary search, the logarithms and the cost model of qualities 10 and 11 (rust-brotli_amd/csrc/zopfli_device.h,
entropy_device.h) against the oracle, part by part.

Whole streams cannot steer these parts.  The device finds the 113 transforms of BrotliFindAllStaticDictionaryMatches through five
tables of affix rows where the reference (and the oracle, orc_static_dict.c) spells out a cascade of character tests; a row shows in a
stream only where the text reaches it AND the shortest path picks it -- over every position of alice29.txt 42 of the 121 transform ids
never even occur.  The costs are f32 / f64 arithmetic that must equal the oracle's to the last bit, and a last-bit difference flips a
parse only where two paths tie that closely.  The logarithm behind both (br_log2f: glibc's log2f restated) was compared with libm on
the CPU only.  Four introspection entries of both libraries (zopfli_entry.inc, not in the public header) take the inputs of these
parts directly; the oracle's side is the code its streams go through (orc_find_all_static_dictionary_matches, orc_debug_*).

Everything is compared exactly: integers equal, f32 as bit patterns.  Every family first asserts -- in plain Python or on the oracle's
answers, never on the library under test -- that its inputs reach what it is named for, then compares; each is an _emu test (the
scalar twins) and a gpu test (the kernels).  The dictionary families carry a third, independent reference: every entry the library
reports is decoded and the word rebuilt by libbrotlicommon, which must stand in the text."""
import functools
import os

import numpy as np
import pytest

import dict_words
import emu
import orc
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = orc.INVALID_MATCH
TAIL = bytes(64)  # what the entry (and the product's text buffer) carries behind the text


def _lib(kind):
    if kind == "emu":
        return emu.lib()
    import gpulib
    return gpulib.lib()


# ------------------------------------------------------------------------------------------------ dictionary search: comparison
def decode_all(matches):
    """(query, length, length code, index, transform) arrays of every reported entry"""
    T = dict_words.tables()
    q, length = np.nonzero(matches != INVALID)
    m = matches[q, length].astype(np.int64)
    len_code = m & 31
    distance = m >> 5
    bits = np.array(T.size_bits, dtype=np.int64)[len_code]
    return q, length, len_code, distance & ((1 << bits) - 1), distance >> bits


def assert_sound(text, at, max_length, matches):
    """the third reference: the word libbrotlicommon builds from an entry stands in the text over exactly the reported length"""
    q, length, len_code, idx, t = decode_all(matches)
    assert len(q) > 0
    assert int(len_code.min()) >= 4 and int(len_code.max()) <= 24 and int(t.max()) < dict_words.NUM_TRANSFORMS
    assert np.all(length <= np.asarray(max_length, dtype=np.int64)[q]), "an entry longer than max_length"
    at = np.asarray(at, dtype=np.int64)
    bad = []
    for qi, ln, lc, ix, tr in zip(q.tolist(), length.tolist(), len_code.tolist(), idx.tolist(), t.tolist()):
        w = dict_words.word(lc, ix, tr)
        a = int(at[qi])
        if len(w) != ln or text[a:a + ln] != w:
            bad.append((qi, ln, lc, ix, tr))
    assert not bad, "entries that are not in the text (query, length, length code, index, transform): %s" % bad[:8]


def compare_dictionary(L, text, at, lo, hi, want, want_any):
    got, got_any = emu.dictionary_matches(L, text, at, lo, hi)
    diff = np.flatnonzero((got != want).any(axis=1) | (got_any != want_any))
    if len(diff):
        lines = []
        for q in diff[:8].tolist():
            for ln in np.flatnonzero(got[q] != want[q]).tolist():
                g, w = int(got[q, ln]), int(want[q, ln])
                lines.append("query %d at %d min %d max %d text %r: length %d: got %s, oracle %s (length code, index, transform)" % (
                    q, at[q], lo[q], hi[q], text[at[q]:at[q] + min(int(hi[q]), 48)], ln,
                    dict_words.decode_match(g) if g != INVALID else None, dict_words.decode_match(w) if w != INVALID else None))
            if got_any[q] != want_any[q]:
                lines.append("query %d: any %d, oracle %d" % (q, got_any[q], want_any[q]))
        raise AssertionError("%d of %d queries differ from the oracle:\n%s" % (len(diff), len(at), "\n".join(lines)))
    assert_sound(text, at, hi, got)


# ------------------------------------------------------------------------------------------------ A: constructed queries
FILLERS = (b"\x01", b" ", b"ing ", b" of ", b" of the ", b" and ", b". The ", b". This ", b"=\"", b"='", b"\n\t", b", ", b"(", b"]",
           b"\xc2\xa0")  # (U+00A0)
MIN_LENGTHS = (4, 5, 9, 17, 38)
INDICES_PER_CELL = 6
ROOM = 44  # every text is followed by fillers and 0x01 up to this many bytes: max_length goes up to L + 40


@functools.lru_cache(maxsize=None)
def constructed():
    """-> dict(text, at, lo, hi, item (of every query), items [(transform, word length, L, first query, one past the last query)])"""
    T = dict_words.tables()
    rng = np.random.default_rng(31337)
    text = bytearray()
    at, lo, hi, item_of, items = [], [], [], [], []
    for t in range(dict_words.NUM_TRANSFORMS):
        for l in dict_words.WORD_LENGTHS:
            for idx in rng.integers(0, 1 << T.size_bits[l], INDICES_PER_CELL).tolist():
                w = dict_words.word(l, idx, t)
                big_l = len(w)
                start = len(text)
                fill = FILLERS[int(rng.integers(0, len(FILLERS)))] + FILLERS[int(rng.integers(0, len(FILLERS)))]
                text += (w + fill + b"\x01" * ROOM)[:big_l + ROOM]
                first = len(at)
                # where the search's own bounds tests (l + 6 >= max_length, l + 2 < max_length, l + 1 >= max_length,
                # max_length >= 5 / 6 / 9) change sides
                for m in (big_l + 40, big_l + 7, big_l + 6, big_l + 3, big_l + 2, big_l + 1, big_l, big_l - 1, l - 1, int(rng.integers(1, 13))):
                    if m < 1:
                        continue
                    at.append(start)
                    hi.append(m)
                    lo.append(MIN_LENGTHS[int(rng.integers(0, len(MIN_LENGTHS)))])
                    item_of.append(len(items))
                items.append((t, l, big_l, first, len(at)))
    return dict(text=bytes(text), at=np.array(at, dtype=np.uint32), lo=np.array(lo, dtype=np.uint32), hi=np.array(hi, dtype=np.uint32),
                item=np.array(item_of), items=items)


@functools.lru_cache(maxsize=None)
def constructed_oracle():
    c = constructed()
    want, want_any = orc.find_all_static_dictionary_matches(c["text"] + TAIL, c["at"], c["lo"], c["hi"])
    # ---- the conditions, on the oracle's answers alone
    own = set()      # transforms reported with their own id at exactly the length L of their text
    for t, l, big_l, first, last in c["items"]:
        if big_l > 37:
            continue
        for m in want[first:last, big_l].tolist():
            if m != INVALID and dict_words.decode_match(m)[2] == t:
                own.add(t)
                break
    assert own >= set(dict_words.CASCADE), "(i) transforms never reported at their own length: %s" % sorted(set(dict_words.CASCADE) - own)
    assert not own & set(dict_words.OMIT_FIRST), "(ii) an omit-first transform reported: %s" % sorted(own & set(dict_words.OMIT_FIRST))
    empty = float(np.mean(want_any == 0))
    assert empty <= 1.0 / 3.0, "(iii) %.3f of the queries come back empty" % empty
    assert np.array_equal(want_any != 0, (want != INVALID).any(axis=1))
    assert_sound(c["text"], c["at"], c["hi"], want)
    return want, want_any, dict(queries=len(c["at"]), transforms=len(own), empty=empty)


def _constructed(kind):
    c = constructed()
    want, want_any, figures = constructed_oracle()
    print("constructed queries:", figures)
    assert 140000 <= figures["queries"] <= 1 << 20
    compare_dictionary(_lib(kind), c["text"], c["at"], c["lo"], c["hi"], want, want_any)


def test_dictionary_constructed_emu():
    _constructed("emu")


@pytest.mark.gpu
def test_dictionary_constructed_gpu():
    _constructed("gpu")


# ------------------------------------------------------------------------------------------------ B: natural and hostile text
@functools.lru_cache(maxsize=None)
def natural():
    """[(label, text, at, lo, hi, want, want_any)]: one launch each"""
    out = []
    a = synth.alice()[:20000]
    pos = np.arange(len(a), dtype=np.uint32)
    rest = len(a) - pos
    # every position, and the last 40 once more with max_length = rest: the maximum length runs from 40 down to 1
    at = np.concatenate((pos, pos[-40:]))
    hi = np.concatenate((np.minimum(rest, 325), rest[-40:])).astype(np.uint32)
    lo = np.full(len(at), 4, dtype=np.uint32)
    assert hi[-40] == 40 and hi[-1] == 1 and hi[0] == 325
    out.append(("alice", a, at, lo, hi) + orc.find_all_static_dictionary_matches(a + TAIL, at, lo, hi))
    r = np.random.default_rng(99).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    at = np.arange(len(r), dtype=np.uint32)
    hi = np.minimum(len(r) - at, 325).astype(np.uint32)
    lo = np.full(len(at), 4, dtype=np.uint32)
    out.append(("random", r, at, lo, hi) + orc.find_all_static_dictionary_matches(r + TAIL, at, lo, hi))
    # (random bytes: the buckets are mostly empty -- the share of empty answers is no condition here; alice must find words)
    assert float(np.mean(out[0][6] != 0)) > 0.25, "alice finds too few words to test anything"
    assert_sound(a, out[0][2], out[0][4], out[0][5])
    return out


def _natural(kind):
    L = _lib(kind)
    for label, text, at, lo, hi, want, want_any in natural():
        print(label, "queries", len(at), "with a match", int(np.count_nonzero(want_any)))
        if np.count_nonzero(want_any) == 0:  # (nothing to decode: equality is all there is)
            got, got_any = emu.dictionary_matches(L, text, at, lo, hi)
            assert np.array_equal(got, want) and np.array_equal(got_any, want_any), label
        else:
            compare_dictionary(L, text, at, lo, hi, want, want_any)


def test_dictionary_natural_and_hostile_emu():
    _natural("emu")


@pytest.mark.gpu
def test_dictionary_natural_and_hostile_gpu():
    _natural("gpu")


def test_dictionary_entry_refuses():
    L = emu.lib()
    text = b"the quick brown fox"
    for at, lo, hi in (([0], [4], [0]), ([0], [4], [len(text) + 1]), ([len(text)], [4], [1]), ([0xffffffff], [4], [2])):
        r, got, _ = emu.dictionary_matches_raw(L, text, at, lo, hi)
        assert r == -1 and np.all(got == 0xeeeeeeee), (at, hi)
    assert emu.dictionary_matches_raw(L, text, [], [], [])[0] == -1
    r, got, anyv = emu.dictionary_matches_raw(L, text, [0, len(text) - 1], [4, 4], [len(text), 1])
    assert r == 0 and np.all(got[1] == INVALID) and anyv[1] == 0


# ------------------------------------------------------------------------------------------------ C: log2 on the device
def edges(k_lo, k_hi):
    return np.array([(1 << k) + d for k in range(k_lo, k_hi + 1) for d in (-1, 0, 1)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def log2_range(stride):
    v = np.arange(0, (1 << 24) + 1, stride, dtype=np.uint64)
    if v[-1] != 1 << 24:
        v = np.append(v, np.uint64(1 << 24))
    v = np.unique(np.concatenate((v, np.arange(0, 1024, dtype=np.uint64), edges(8, 23))))
    return v, orc.debug_fast_log2(v)


def report_log2(label, values, got, want):
    diff = np.flatnonzero(got != want)
    if len(diff):
        raise AssertionError("%s: %d of %d values differ; value, library bits, libm bits: %s" % (
            label, len(diff), len(values), [(int(values[i]), hex(int(got[i])), hex(int(want[i]))) for i in diff[:16]]))


def _log2(kind, stride):
    L = _lib(kind)
    v, want = log2_range(stride)
    assert v[0] == 0 and v[-1] == 1 << 24 and (stride > 1 or len(v) == (1 << 24) + 1)
    assert 255 in v and 256 in v  # the table gives way to the restated log2f at 256
    print("log2: %d values from 0 to 2^24 in modes 0 and 1" % len(v))
    report_log2("z_fast_log2 (mode 0)", v, emu.fast_log2(L, 0, v), want)
    report_log2("br_fast_log2 (mode 1)", v, emu.fast_log2(L, 1, v), want)
    # 64-bit counts: the conversion to f32 is part of what is compared (round to nearest even at 2^k + 1 from k = 24 on)
    big = edges(24, 63)
    assert int(big.max()) == (1 << 63) + 1
    report_log2("z_fast_log2 (mode 0), 2^k - 1, 2^k, 2^k + 1", big, emu.fast_log2(L, 0, big), orc.debug_fast_log2(big))
    # br_fast_log2 takes 32 bits: 2^32 and 2^32 + 1 arrive as 0 and 1
    mid = edges(24, 32)
    report_log2("br_fast_log2 (mode 1), 2^k - 1, 2^k, 2^k + 1", mid, emu.fast_log2(L, 1, mid), orc.debug_fast_log2(mid & np.uint64(0xffffffff)))
    t = np.arange(65536, dtype=np.uint64)
    report_log2("logs_16 (mode 2)", t, emu.fast_log2(L, 2, t), orc.logs_16())
    report_log2("logs_16 (mode 2), index wraps", t + np.uint64(65536), emu.fast_log2(L, 2, t + np.uint64(65536)), orc.logs_16())


def test_log2_emu():
    _log2("emu", 97)


@pytest.mark.gpu
def test_log2_gpu():
    _log2("gpu", 1)


def test_log2_entry_refuses():
    L = emu.lib()
    with pytest.raises(RuntimeError, match="returned -1"):
        emu.fast_log2(L, 3, [1, 2])
    with pytest.raises(RuntimeError, match="returned -1"):
        emu.fast_log2(L, 0, [])


# ------------------------------------------------------------------------------------------------ D: literal costs
# the two window halves (495 and 2000) twice each, the `i < 2000` ramp, the 25 and 500 of the statistics level, with their neighbours
LENGTHS = (1, 2, 3, 24, 25, 26, 494, 495, 496, 497, 989, 990, 991, 992, 1999, 2000, 2001, 2002, 3999, 4000, 4001, 4002, 20000, 65536)
SHARES = (0.70, 0.74, 0.75, 0.76, 0.80)  # of ASCII in front of 0x80 bytes: BrotliIsMostlyUTF8 asks for more than 0.75


def _repeat(b, n):
    return (b * (n // len(b) + 1))[:n]


@functools.lru_cache(maxsize=None)
def literal_classes():
    rng = np.random.default_rng(4242)
    n = max(LENGTHS)
    a = synth.alice()
    ascii_text = _repeat(a, n)
    cyr = [chr(c) for c in range(0x430, 0x450)]
    two = "".join("".join(cyr[i] for i in rng.integers(0, 32, int(rng.integers(2, 9)))) + (" " if rng.integers(0, 9) else ". ")
                  for _ in range(n // 6)).encode("utf-8")
    three = "".join(chr(int(c)) if rng.integers(0, 12) else "。" for c in rng.integers(0x4e00, 0x9fff, n // 3 + 8)).encode("utf-8")
    rnd = rng.integers(0, 256, n, dtype=np.uint8)
    f4 = rnd.copy()
    f4[::3] = 0xf4
    golden = open(os.path.join(HERE, "golden", "random_then_unicode"), "rb").read()
    classes = [("ascii", ascii_text), ("random", rnd.tobytes()), ("zeros", bytes(n)), ("two-byte utf-8", two), ("three-byte utf-8", three),
               ("invalid four-byte heads", f4.tobytes()), ("random_then_unicode", _repeat(golden, n))]
    for name, data in classes:
        assert len(data) >= n, name
    return classes, ascii_text


@functools.lru_cache(maxsize=None)
def literal_jobs():
    """[(label, block, oracle cost bits, oracle prefix bits)] and the conditions, on the oracle's two extra outputs"""
    classes, ascii_text = literal_classes()
    jobs, verdict, level = [], {}, {}
    for n in LENGTHS:
        blocks = [(name, data[:n]) for name, data in classes]
        for s in SHARES:
            k = int(round(s * n))
            blocks.append(("ascii share %.2f" % s, ascii_text[:k] + b"\x80" * (n - k)))
        for name, b in blocks:
            assert len(b) == n
            cost, prefix, utf8, lvl = orc.debug_literal_costs(b)
            jobs.append(("%s, %d bytes" % (name, n), b, cost, prefix))
            verdict[(name, n)], level[(name, n)] = utf8, lvl
    assert set(verdict.values()) == {True, False}
    on_utf8_side = {level[k] for k in verdict if verdict[k]}
    # Level 2 cannot occur: the reference's DecideMultiByteStatsLevel assigns 1 in both branches (literal_cost.rs:20-46) and the oracle
    # and the device restate that as it is (zopfli_device.h, z_literal_costs: `if (counts[2] < 500) max_utf8 = 1;`).  Not a slip to repair.
    assert on_utf8_side == {0, 1}, on_utf8_side
    assert level[("three-byte utf-8", 65536)] == 1  # (more than 500 third bytes, and still level 1)
    for n in LENGTHS:
        if n >= 496:
            assert not verdict[("ascii share 0.74", n)] and verdict[("ascii share 0.76", n)], n
        assert verdict[("ascii", n)] and not verdict[("zeros", n)], n
    return jobs


def _literal_costs(kind):
    jobs = literal_jobs()
    assert len(jobs) == len(LENGTHS) * 12
    got = emu.literal_costs(_lib(kind), [b for _, b, _, _ in jobs])
    bad = []
    for (label, b, cost, prefix), (g_cost, g_prefix) in zip(jobs, got):
        for what, g, w in (("cost", g_cost, cost), ("prefix sum", g_prefix, prefix)):
            if not np.array_equal(g, w):
                i = int(np.flatnonzero(g != w)[0])
                bad.append("%s: %s differs first at %d (byte 0x%02x): got 0x%08x, oracle 0x%08x, %d entries differ" % (
                    label, what, i, b[min(i, len(b) - 1)], int(g[i]), int(w[i]), int(np.count_nonzero(g != w))))
    assert not bad, "\n".join(bad[:16])


def test_literal_costs_emu():
    _literal_costs("emu")


@pytest.mark.gpu
def test_literal_costs_gpu():
    _literal_costs("gpu")


# ------------------------------------------------------------------------------------------------ E: costs from histograms
ROW_SIZES = ((256, True), (704, False), (140, False), (64, False), (544, False))


@functools.lru_cache(maxsize=None)
def histogram_jobs():
    rng = np.random.default_rng(777)
    jobs = []
    for size, literal in ROW_SIZES:
        def add(label, row):
            row = np.asarray(row, dtype=np.uint32)
            assert row.shape == (size,)
            jobs.append(("%s, %d counts%s" % (label, size, ", literal" if literal else ""), row, literal))

        def blank():
            return np.zeros(size, dtype=np.uint32)
        add("all zero", blank())
        r = blank()
        r[rng.integers(0, size)] = 1
        add("one count of 1", r)
        add("counts 0..2", rng.integers(0, 3, size))
        add("counts 0..299", rng.integers(0, 300, size))
        r = rng.integers(250, 260, size)
        assert r.min() < 256 <= r.max()  # the table gives way to br_log2f at 256
        add("counts 250..259", r)
        r = rng.integers(1, 70001, size) * (rng.integers(0, 10, size) == 0)
        r[rng.integers(0, size)] = 70000
        assert 0 < np.count_nonzero(r) < size // 4 + 8 and r.max() > 65536
        add("sparse counts up to 70 000", r)
        r = blank()
        at = int(rng.integers(0, size - 6))
        r[at:at + 6] = (255, 256, 257, 65535, 65536, 65537)
        add("255 256 257 65535 65536 65537", r)
        r = blank()
        r[rng.integers(0, size)] = (1 << 24) + 1
        add("one count of 2^24 + 1", r)
        add("counts up to 2^20", rng.integers(0, (1 << 20) + 1, size))
        add("all 0xffffffff", np.full(size, 0xffffffff, dtype=np.uint32))
        r = blank()
        r[rng.choice(size, 2, replace=False)] = 1 << 31
        assert int(r.sum(dtype=np.uint64)) == 1 << 32  # (a sum that needs the 64-bit accumulator)
        add("two counts of 2^31", r)
        add("counts of 0 or 16 777 217", rng.integers(0, 2, size) * 16777217)
    return [(label, row, literal, orc.debug_cost_from_histogram(row, literal)) for label, row, literal in jobs]


def _histogram_costs(kind):
    jobs = histogram_jobs()
    assert len(jobs) == 60
    got = emu.cost_from_histogram(_lib(kind), [row for _, row, _, _ in jobs], [lit for _, _, lit, _ in jobs])
    bad = []
    for (label, row, _, want), g in zip(jobs, got):
        if not np.array_equal(g, want):
            i = int(np.flatnonzero(g != want)[0])
            bad.append("%s: first at %d (count %d, sum %d): got 0x%08x, oracle 0x%08x" % (label, i, row[i], int(row.sum(dtype=np.uint64)),
                                                                                          int(g[i]), int(want[i])))
    assert not bad, "\n".join(bad)


def test_histogram_costs_emu():
    _histogram_costs("emu")


@pytest.mark.gpu
def test_histogram_costs_gpu():
    _histogram_costs("gpu")


def test_cost_entries_refuse():
    import ctypes
    L = emu.lib()
    with pytest.raises(RuntimeError, match="returned -1"):
        emu.literal_costs(L, [b"abc", b""])
    with pytest.raises(RuntimeError, match="returned -1"):
        emu.literal_costs(L, [bytes(65537)])
    with pytest.raises(RuntimeError, match="returned -1"):
        emu.cost_from_histogram(L, [np.zeros(1201, dtype=np.uint32)], [False])
    L.brotli_mi355x_debug_cost_from_histogram.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    assert L.brotli_mi355x_debug_cost_from_histogram(0, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ for tests/zopfli_parts_check.cpp
def dump_constructed(path):
    """family A's text and queries for the stand-alone check program: u32 n_text, u32 n_queries, the text, at[], min_length[], max_length[]"""
    c = constructed()
    with open(path, "wb") as f:
        f.write(np.array([len(c["text"]), len(c["at"])], dtype=np.uint32).tobytes())
        f.write(c["text"])
        for k in ("at", "lo", "hi"):
            f.write(c[k].tobytes())


if __name__ == "__main__":
    import sys
    dump_constructed(sys.argv[1])
