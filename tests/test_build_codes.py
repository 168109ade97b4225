"""The prefix-code builder (mb_build_codes) against the oracle, histogram by histogram.

On the device k_build_codes runs one wavefront per histogram and takes code paths that the emulation build never compiles: the
rank sort of 13 and more items, the ballot / popcount leaf build, the depths climbed from the leaves through parent links, the
count_limit *= 2 retry around them, the ballot prologue of the RLE optimiser, its register-resident smoothing walk (64 counts to a
register, special cases for a length that is a multiple of 64 and for 704, a look two positions ahead into the next register,
collapsed strides written 64 at a time) and the cooperative code assignment.  Whole streams cannot steer this stage: LZ77, the block
splitter and the optimiser shape every histogram first.  brotli_mi355x_debug_build_codes hands rows to the builder directly; the
oracle's orc_build_code is optimize_huffman_counts_for_rle (when asked) + build_and_store_huffman_tree, the functions its stream
path uses.

Every family states in plain Python (or on the oracle's result alone) that its rows reach the branch it is named for, then compares
every row exactly: optimised histogram, depth[], bits[], tree_nbits and the first tree_nbits bits of the serialised tree.  One seam
call per (kind, alphabet, mode); the oracle's rows are computed once and shared by the emulation and the device test."""
import functools
import random

import numpy as np
import pytest

import emu
import orc
import synth

LIT, CMD, DIST = 0, 1, 2
PLAIN, OPT = emu.CODE_PLAIN, emu.CODE_OPTIMIZED
ROW = emu.ROW_LEN
KIND_NAME = ("literal", "command", "distance")
DIST_HISTO = 544  # BROTLI_NUM_HISTOGRAM_DISTANCE_SYMBOLS
LARGE_WINDOW_DIST = 16 + 120 + (62 << 4)  # the large-window distance alphabet at NPOSTFIX 3, NDIRECT 120


def code_shape(kind, nds):
    """(histogram length, alphabet size, optimised length) of one prefix code, as the reference's stream path sets them:
    BrotliOptimizeHistograms (metablock.rs:1076-1108) and build_and_store_entropy_codes (brotli_bit_stream.rs:1860-1889)"""
    if kind == LIT:
        return 256, 256, 256
    if kind == CMD:
        return 704, 704, 704
    effective = min(nds, DIST_HISTO)
    return effective, nds, effective


class Family:
    def __init__(self, name, kind, mode, nds=DIST_HISTO):
        self.name, self.kind, self.mode, self.nds = name, kind, mode, nds
        self.hist_len = code_shape(kind, nds)[0]
        self.rows, self.labels = [], []

    def add(self, label, counts):
        """counts: dict symbol -> count, or a sequence that starts at symbol 0"""
        row = np.zeros(ROW[self.kind], dtype=np.uint32)
        if isinstance(counts, dict):
            for s, c in counts.items():
                row[s] = c
            assert not counts or max(counts) < self.hist_len
        else:
            assert len(counts) <= self.hist_len, (label, len(counts))
            row[:len(counts)] = counts
        assert int(row.astype(np.uint64).sum()) < 1 << 32, label  # (a well-formed histogram: the tree's counts are 32 bits)
        self.rows.append(row)
        self.labels.append(label)
        return row

    def array(self):
        return np.stack(self.rows)

    def title(self):
        return "%s/%s/%s/nds=%d" % (self.name, KIND_NAME[self.kind], "plain" if self.mode == PLAIN else "optimized", self.nds)


_ORACLE = {}


def oracle_rows(fam):
    """the oracle's five outputs for every row of a family, computed once"""
    key = fam.title()
    if key not in _ORACLE:
        hist_len, alphabet, opt_len = code_shape(fam.kind, fam.nds)
        _ORACLE[key] = [orc.build_code(hist_len, alphabet, opt_len, fam.mode == OPT, row, ROW[fam.kind]) for row in fam.rows]
    return _ORACLE[key]


def tree_bits_equal(a, b, nbits):
    full = nbits >> 3
    if not np.array_equal(a[:full], b[:full]):
        return False
    rest = nbits & 7
    return rest == 0 or (int(a[full]) ^ int(b[full])) & ((1 << rest) - 1) == 0


def compare(L, fam, note=""):
    """every row of the family through the seam (one call), every output against the oracle's; returns the seam's outputs"""
    got_h, got_d, got_b, got_t, got_n = emu.build_codes(L, fam.kind, fam.nds, fam.mode, fam.array())
    ref = oracle_rows(fam)
    assert len(ref) == len(fam.rows) == got_h.shape[0]
    bad = []
    for r, (h, d, b, t, n) in enumerate(ref):
        wrong = []
        if not np.array_equal(got_h[r], h):
            wrong.append("histogram")
        if not np.array_equal(got_d[r], d):
            wrong.append("depth")
        if not np.array_equal(got_b[r], b):
            wrong.append("bits")
        if int(got_n[r]) != n:
            wrong.append("tree_nbits %d != %d" % (got_n[r], n))
        elif not tree_bits_equal(got_t[r], t, n):
            wrong.append("tree")
        if wrong:
            bad.append("row %d [%s]: %s" % (r, fam.labels[r], ", ".join(wrong)))
    assert not bad, "%s%s: %d of %d rows differ from the oracle\n%s" % (fam.title(), note, len(bad), len(ref), "\n".join(bad[:12]))
    return got_h, got_d, got_b, got_t, got_n


# ------------------------------------------------------------------------------------------------ plain-Python statements
def huffman_max_depth(counts):
    """depth of the deepest leaf of the Huffman tree over the non-zero counts, no limit: the textbook two-queue construction over
    the leaves ordered by (count, symbol descending), a leaf before an inner node of the same weight"""
    leaves = sorted((c, -s) for s, c in enumerate(counts) if c)
    n = len(leaves)
    if n == 1:
        return 1
    weight = [c for c, _ in leaves]
    parent = {}
    i, j = 0, n
    for _ in range(n - 1):
        pick = []
        for _ in range(2):
            if i < n and (j >= len(weight) or weight[i] <= weight[j]):
                pick.append(i)
                i += 1
            else:
                pick.append(j)
                j += 1
        weight.append(weight[pick[0]] + weight[pick[1]])
        parent[pick[0]] = parent[pick[1]] = len(weight) - 1
    deepest = 0
    for leaf in range(n):
        d, p = 0, leaf
        while p in parent:
            p = parent[p]
            d += 1
        deepest = max(deepest, d)
    return deepest


def doublings_needed(counts, limit_depth=15):
    """how often the reference doubles count_limit (counts clamped from below to 1, 2, 4, ...) until the tree fits; every clamped
    total must still fit the tree's 32-bit counts"""
    t, limit = 0, 1
    while True:
        clamped = [max(c, limit) if c else 0 for c in counts]
        assert sum(clamped) < 1 << 32
        if huffman_max_depth(clamped) <= limit_depth:
            return t
        t += 1
        limit *= 2


M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def py_optimize(counts, length):
    """BrotliOptimizeHuffmanCountsForRle (entropy_encode.rs:211-345) in plain Python with the reference's integer widths.  Returns
    (counts after, info): info['stage'] = where it returned, 'filled' = the fill-in rule changed a count, 'strides' = (end, stride)
    of every collapsed stride, 'wide' / 'narrow' = a division whose operands left / fitted 32 bits, 'marks' = good_for_rle."""
    c = list(counts)
    info = dict(stage="lt16", filled=False, strides=[], wide=False, narrow=False, marks=None, length=length)
    if sum(1 for v in c[:length] if v) < 16:
        return c, info
    while length and c[length - 1] == 0:
        length -= 1
    info["length"] = length
    used = [v for v in c[:length] if v]
    info["smallest"], info["zeros"] = min(used), length - len(used)
    if min(used) < 4 and length - len(used) < 6:
        for i in range(1, length - 1):
            if c[i - 1] and not c[i] and c[i + 1]:
                c[i] = 1
                info["filled"] = True
    info["stage"] = "lt28"
    if len(used) < 28:
        return c, info
    info["stage"] = "full"
    good = [0] * (length + 1)
    i = 0
    while i < length:
        k = i
        while k < length and c[k] == c[i]:
            k += 1
        if (c[i] == 0 and k - i >= 5) or (c[i] != 0 and k - i >= 7):
            for m in range(i, k):
                good[m] = 1
        i = k
    info["marks"] = good[:length]

    def div(a, b):
        info["wide" if (a | b) >> 32 else "narrow"] = True
        return a // b

    stride = total = 0
    limit = ((256 * (c[0] + c[1] + c[2])) & M32) // 3 + 420
    for i in range(length + 1):
        if i == length or good[i] or (i and good[i - 1]) or ((((256 * c[i]) & M32) - limit + 1240) & M64) >= 2480:
            if stride >= 4 or (stride >= 3 and total == 0):
                count = div(total + stride // 2, stride)
                if count == 0:
                    count = 1
                if total == 0:
                    count = 0
                for k in range(stride):
                    c[i - k - 1] = count & M32
                info["strides"].append((i, stride))
            stride = total = 0
            if i + 2 < length:
                limit = ((256 * (c[i] + c[i + 1] + c[i + 2])) & M32) // 3 + 420
            elif i < length:
                limit = (256 * c[i]) & M32
            else:
                limit = 0
        stride += 1
        if i != length:
            total += c[i]
            if stride >= 4:
                limit = div(256 * total + stride // 2, stride)
            if stride == 4:
                limit += 120
    return c, info


def jag(i):
    """a background that forms neither runs nor strides: neighbours 3000 apart"""
    return 40 if i % 2 == 0 else 3040


def kinds_with_alphabet():
    return [(LIT, DIST_HISTO), (CMD, DIST_HISTO), (DIST, DIST_HISTO)]


# ------------------------------------------------------------------------------------------------ family: depth limit
FIB = [1, 1]
while len(FIB) < 45:
    FIB.append(FIB[-1] + FIB[-2])


@functools.lru_cache(maxsize=None)
def depth_limit_families():
    fams = []
    rng = random.Random(1597)
    for kind, nds in kinds_with_alphabet():
        fam = Family("depth limit", kind, PLAIN, nds)  # kCodePlain: the counts reach the builder untouched
        doublings = []
        for n in range(16, 46):
            for rep in range(6):
                places = rng.sample(range(fam.hist_len), n)
                values = FIB[:n]
                rng.shuffle(values)
                row = fam.add("fibonacci on %d symbols, placement %d" % (n, rep), dict(zip(places, values)))
                deepest = huffman_max_depth(row.tolist())
                if n == 16:
                    assert deepest == 15  # fits exactly: no retry
                if n == 17:
                    assert deepest == 16  # one level too deep
                if n >= 17:
                    assert deepest > 15, (n, deepest)  # the retry is certain
                doublings.append(doublings_needed(row.tolist()))
                assert (doublings[-1] == 0) == (n == 16)
                assert (doublings[-1] >= 2) == (n >= 31), (n, doublings[-1])  # (one doubling halves the depth of a Fibonacci chain)
        assert sum(1 for t in doublings if t >= 2) == 90 and max(doublings) >= 8, sorted(set(doublings))
        fam.doublings = doublings
        fams.append(fam)
    return fams


# ------------------------------------------------------------------------------------------------ family: sort and leaf build
USED_SYMBOLS = [1, 2, 3, 4, 5, 12, 13, 14, 56, 57, 58, 63, 64, 65, 128, 129, 255, 256, 703, 704]
COUNT_SHAPES = {
    "equal": lambda i, n: 7,
    "pairs": lambda i, n: 1 + i // 2,
    "increasing": lambda i, n: 1 + i,
    "decreasing": lambda i, n: n - i,
}


@functools.lru_cache(maxsize=None)
def sort_families():
    fams = []
    rng = random.Random(13)
    for kind, nds in kinds_with_alphabet():
        fam = Family("sort and leaf build", kind, PLAIN, nds)
        A = fam.hist_len
        fam.used = []
        for n in USED_SYMBOLS:
            if n > A:
                continue
            placements = {"first": list(range(n)), "last": list(range(A - n, A))}
            if n <= 64:
                placements["one chunk"] = sorted(rng.sample(range(64, 128), n))
            if n > 1:
                placements["spread"] = [(i * (A - 1)) // (n - 1) for i in range(n)]  # (one per 64-symbol chunk where n allows)
            for pname, places in placements.items():
                assert len(set(places)) == n and places == sorted(places)
                if pname in ("first", "spread"):
                    assert places[0] == 0
                if pname in ("last", "spread"):
                    assert places[-1] == A - 1
                if pname == "one chunk":
                    assert places[0] // 64 == places[-1] // 64
                if pname == "spread" and n <= A // 64:
                    assert len(set(p // 64 for p in places)) == n
                for sname, shape in COUNT_SHAPES.items():
                    row = fam.add("%d used, %s, %s" % (n, pname, sname), {p: shape(i, n) for i, p in enumerate(places)})
                    assert int(np.count_nonzero(row)) == n
                    fam.used.append(n)
        assert {12, 13} <= set(fam.used)  # the insertion sort's last size and the first size of the other sort
        # both tree shapes of the four-symbol simple code (depths 2 2 2 2 and 1 2 3 3), by the oracle's own depths
        shapes = set()
        for r, (h, d, b, t, nb) in enumerate(oracle_rows(fam)):
            if fam.used[r] == 4:
                shapes.add(tuple(sorted(int(x) for x in d if x)))
        assert shapes == {(2, 2, 2, 2), (1, 2, 3, 3)}, shapes
        fams.append(fam)
    return fams


# ------------------------------------------------------------------------------------------------ family: RLE optimiser
LAST_USED = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 639, 640, 641, 703, 704]


def flat(i):
    return 500 + (i % 2)  # (never seven equal counts in a row: no good_for_rle marks; one stride as long as it lasts)


def add_stride_row(fam, label, start, s):
    """a background of jag() with `s` near-equal counts from `start`: returns the row"""
    end = min(fam.hist_len, max(start + s + 8, 40))
    return fam.add(label, [flat(i) if start <= i < start + s else jag(i) for i in range(end)])


@functools.lru_cache(maxsize=None)
def rle_families():
    fams = []
    for kind, nds in kinds_with_alphabet():
        fam = Family("RLE optimiser", kind, OPT, nds)
        A = fam.hist_len
        expect = {}  # label -> check on (py_optimize info, row before, oracle row after)

        def add(label, counts, check=None):
            fam.add(label, counts)
            if check:
                expect[label] = check

        def changed(info, before, after):
            return not np.array_equal(before, after)

        # --- either side of the early returns (fewer than 16 / 28 used symbols; 5 is never the deciding one once 16 are used)
        sixteen = [0 if i in (2, 5, 8, 11, 14) else 3 for i in range(21)]
        assert sum(1 for v in sixteen if v) == 16 and sum(1 for v in sixteen[:20] if v) == 15
        add("16 used, smallest 3, 5 isolated zeros", sixteen, lambda i, b, a: i["stage"] == "lt28" and i["filled"] and changed(i, b, a))
        add("15 used, smallest 3, 5 isolated zeros", sixteen[:20], lambda i, b, a: i["stage"] == "lt16" and not changed(i, b, a))
        add("28 used, flat", [flat(i) for i in range(28)], lambda i, b, a: i["stage"] == "full" and changed(i, b, a))
        add("27 used, flat", [flat(i) for i in range(27)], lambda i, b, a: i["stage"] == "lt28" and not changed(i, b, a))
        add("5 used", {0: 3, 2: 3, 4: 3, 6: 3, 8: 3}, lambda i, b, a: i["stage"] == "lt16" and not changed(i, b, a))
        add("4 used", {0: 3, 2: 3, 4: 3, 6: 3}, lambda i, b, a: i["stage"] == "lt16" and not changed(i, b, a))
        # --- the fill-in rule: smallest count below 4 and fewer than 6 zeros
        for used in (20, 30):
            for smallest in (3, 4):
                for zeros in (5, 6):
                    row, k = [], 0
                    while k < used:
                        if len(row) % 3 == 2 and row.count(0) < zeros:
                            row.append(0)
                        else:
                            row.append(smallest + 9 * (k % 3) if used == 20 else smallest + 3000 * (k % 2))
                            k += 1
                    assert row.count(0) == zeros and min(v for v in row if v) == smallest and len(row) == used + zeros
                    fills = smallest == 3 and zeros == 5
                    add("%d used, smallest %d, %d isolated zeros" % (used, smallest, zeros), row,
                        lambda i, b, a, fills=fills, used=used: i["filled"] == fills and i["smallest"] == b[b > 0].min() and
                        (used == 30 or changed(i, b, a) == fills))
        # --- the last used symbol around every register edge, with a stride alive at the end (it closes exactly at `length`),
        #     with a jagged end, and with noise
        rng = random.Random(704)
        for length in sorted(set(LAST_USED) | set(v + 1 for v in LAST_USED)):  # (as the length, and as the last symbol's index)
            if length <= A:
                what = "length %d" % length
                add("flat to the end, " + what, [flat(i) for i in range(length)],
                    lambda i, b, a, n=length: i["length"] == n and i["strides"] and i["strides"][-1] == (n, n))
                add("flat tail of 5, " + what, [jag(i) if i < length - 5 else flat(i) for i in range(length)],
                    lambda i, b, a, n=length: i["length"] == n and (n, 5) in i["strides"])
                add("flat, unused symbols behind, " + what, [flat(i) for i in range(length)] + [0] * min(7, A - length),
                    lambda i, b, a, n=length: i["length"] == n and i["stage"] == "full")
                add("noise, " + what, [rng.randrange(1, 2000) for _ in range(length)], lambda i, b, a, n=length: i["length"] == n and i["stage"] == "full")
                add("jagged, " + what, [jag(i) for i in range(length)], lambda i, b, a, n=length: i["length"] == n and not i["strides"])
        # --- runs of zeros (marked from 5) and of equal counts (marked from 7) that start at, end at and straddle a register edge
        for edge in [e for e in (64, 128, 640) if e + 40 <= A]:
            for value, lengths, marked_from in ((0, (4, 5, 6), 5), (77, (6, 7, 8), 7)):
                for r in lengths:
                    for where, first in (("starts at", edge), ("ends at", edge - r), ("straddles", edge - r // 2)):
                        row = [value if first <= i < first + r else jag(i) for i in range(edge + 40)]
                        if where == "straddles":
                            assert first < edge - 1 + 1 and first + r > edge
                        add("run of %d x %d %s lane %d|%d" % (r, value, where, edge - 1, edge), row,
                            lambda i, b, a, first=first, r=r, marked=r >= marked_from:
                            i["stage"] == "full" and i["marks"][first:first + r] == [1 if marked else 0] * r and sum(i["marks"]) == (r if marked else 0))
        # --- strides of 3 (zeros only), 4, 63, 64, 65 and 200 symbols, inside a register and across an edge
        for s in (3, 4, 63, 64, 65, 200):
            for start in sorted({1, 50, 64 - s if 1 < s < 64 else 30}):
                if start + s + 8 > A:
                    continue
                if s == 3:
                    row = [0 if start <= i < start + 3 else jag(i) for i in range(max(start + 12, 40))]
                else:
                    row = [flat(i) if start <= i < start + s else jag(i) for i in range(max(start + s + 8, 40))]
                add("stride of %d from %d" % (s, start), row,
                    lambda i, b, a, s=s, start=start: i["stage"] == "full" and [t for t in i["strides"] if t[1] == s and t[0] - s <= start + 1] != [])
        # a stride that begins in the last two lanes of a register: its first limit averages counts of the next register
        for edge in [e for e in (64, 128, 640) if e + 40 <= A]:
            for start in (edge - 2, edge - 1, edge):
                add("stride of 30 from %d" % start, [flat(i) if start <= i < start + 30 else jag(i) for i in range(start + 36)],
                    lambda i, b, a, start=start: (start + 30, 30) in i["strides"])
        crossing = [flat(i) if 50 <= i < 80 else jag(i) for i in range(100)]
        add("stride across lane 63|64", crossing, lambda i, b, a: any(e - s < 63 and e > 65 for e, s in i["strides"]))
        # --- counts for which 256 * count and 256 * sum leave 32 bits: both arms of the division, the 32-bit wraps
        big = 1 << 24
        wraps = lambda b: any(256 * int(v) > M32 for v in b)
        add("ramp through 1 << 24", [big - 20 + i for i in range(40)], lambda i, b, a: i["stage"] == "full" and wraps(b) and not wraps(b[:20]))
        add("1 << 24 among small counts", [big if i % 9 == 4 else flat(i) for i in range(60)],
            lambda i, b, a: i["narrow"] and wraps(b))  # (256 * count wraps to 0: the stride breaks there)
        # (a stride lives on only while 256 * count fits 32 bits; from four counts of 1 << 22 on, 256 * sum does not)
        add("near 1 << 22, flat, then small", [(1 << 22) + (i % 2) for i in range(48)] + [flat(i) for i in range(40)],
            lambda i, b, a: i["wide"] and i["narrow"] and len(i["strides"]) >= 2 and not wraps(b))
        add("near 1 << 22, flat, 200 symbols", [(1 << 22) + (i % 2) for i in range(200)], lambda i, b, a: i["wide"] and (200, 200) in i["strides"])
        add("near 1 << 23, flat", [(1 << 23) + (i % 2) for i in range(48)] + [flat(i) for i in range(40)], lambda i, b, a: i["stage"] == "full" and i["narrow"])
        add("1 << 24 - 1, flat, then 1 << 24", [big - 1] * 3 + [big - 1 - (i % 2) for i in range(30)] + [big] * 3 + [big + (i % 2) for i in range(30)],
            lambda i, b, a: i["wide"])
        add("one count of 1 << 24 at the end", [flat(i) for i in range(63)] + [big], lambda i, b, a: i["stage"] == "full")
        # every row: the plain-Python optimiser agrees with the oracle, and the row reaches what its label says
        ref = oracle_rows(fam)
        for r, label in enumerate(fam.labels):
            before = fam.rows[r]
            after, info = py_optimize(before.tolist(), A)
            assert after == ref[r][0].tolist(), label
            if label in expect:
                assert expect[label](info, before, ref[r][0]), (fam.title(), label, info["stage"], info["strides"][:8])
        assert len(expect) == len(fam.labels) == len(set(fam.labels))
        fams.append(fam)
    return fams


# ------------------------------------------------------------------------------------------------ family: distance alphabets
@functools.lru_cache(maxsize=None)
def distance_families():
    fams = []
    for nds in (64, 140, DIST_HISTO, LARGE_WINDOW_DIST):
        for mode in (PLAIN, OPT):
            fam = Family("distance alphabets", DIST, mode, nds)
            hist_len, alphabet, opt_len = code_shape(DIST, nds)
            assert hist_len == opt_len == min(nds, 544) and alphabet == nds and fam.hist_len == hist_len
            max_bits = (nds - 1).bit_length()
            assert max_bits == {64: 6, 140: 8, 544: 10, LARGE_WINDOW_DIST: 11}[nds]
            rng = random.Random(nds)
            simple = {}
            for n in (1, 2, 3, 4):
                for pname, places in (("first", list(range(n))), ("last", list(range(hist_len - n, hist_len))),
                                      ("ends", [0] + list(range(hist_len - n + 1, hist_len)))):
                    label = "%d used, %s" % (n, pname)
                    fam.add(label, {p: 1 + 2 * i for i, p in enumerate(places)})
                    simple[label] = n
            for n in (5, 12, 13, 16, 28, 63, hist_len):
                n = min(n, hist_len)
                fam.add("%d used, last symbols" % n, {hist_len - 1 - i: 1 + i for i in range(n)})
                fam.add("%d used, random" % n, {p: rng.randrange(1, 500) for p in rng.sample(range(hist_len), n)})
            fam.add("flat over the whole histogram", [flat(i) for i in range(hist_len)])
            fam.add("flat, last symbol unused", [flat(i) for i in range(hist_len - 1)])
            fam.add("noise over the whole histogram", [rng.randrange(1, 3000) for _ in range(hist_len)])
            fam.add("fibonacci on 30 symbols", dict(zip(rng.sample(range(hist_len), 30), FIB[:30])))
            # a simple code spends max_bits of the ALPHABET per symbol, whatever the histogram's length: the oracle's bit counts
            ref = oracle_rows(fam)
            for r, label in enumerate(fam.labels):
                if label in simple:
                    n = simple[label]
                    assert ref[r][4] == (4 + max_bits if n == 1 else 4 + n * max_bits + (1 if n == 4 else 0)), (nds, label, ref[r][4])
            fams.append(fam)
    return fams


# ------------------------------------------------------------------------------------------------ family: seeded sweep
SWEEP_SEED = 20260419
SWEEP_ROWS = 3000


@functools.lru_cache(maxsize=None)
def alice_symbols():
    """literal bytes, command prefixes and distance prefixes of alice29.txt as the oracle's quality 5 codes them"""
    data = synth.alice()
    _, trace = orc.stream_compress(data, [(1, 5), (2, 22), (5, len(data))], collect_trace=True)
    cmds = [c for t in trace for c in t[3]]
    command = np.array([c[3] for c in cmds], dtype=np.int64)
    distance = np.array([c[4] & 0x3ff for c in cmds if c[3] >= 128 and (c[1] & 0x1ffffff)], dtype=np.int64)
    assert len(command) > 10000 and len(distance) > 5000 and command.max() < 704 and distance.max() < 64
    return np.frombuffer(data, dtype=np.uint8).astype(np.int64), command, distance


@functools.lru_cache(maxsize=None)
def sweep_families():
    fams = []
    for kind, nds in kinds_with_alphabet():
        rs = np.random.RandomState(SWEEP_SEED + kind)
        symbols = alice_symbols()[kind]
        rows = []
        A = code_shape(kind, nds)[0]
        for r in range(SWEEP_ROWS):
            row = np.zeros(A, dtype=np.int64)
            what = r % 4
            if what == 0:  # sparse
                n = rs.randint(1, 40)
                row[rs.choice(A, n, replace=False)] = rs.randint(1, 1 + 10 ** rs.randint(1, 6), n)
                label = "sparse"
            elif what == 1:  # dense, with some holes and a random last symbol
                length = rs.randint(28, A + 1)
                row[:length] = rs.randint(1, 2 + 10 ** rs.randint(0, 5), length) // rs.randint(1, 4)
                row[:length][rs.rand(length) < rs.choice([0.0, 0.05, 0.3])] = 0
                label = "dense"
            elif what == 2:  # power law over the ranks, in order or shuffled
                length = rs.randint(5, A + 1)
                ranks = np.arange(1, length + 1, dtype=np.float64)
                v = (rs.randint(100, 10 ** 7) / ranks ** rs.uniform(0.5, 2.5)).astype(np.int64)
                if rs.rand() < 0.5:
                    rs.shuffle(v)
                row[:length] = v
                label = "power law"
            else:  # a window of alice29.txt
                w = min(int(10 ** rs.uniform(1.5, 4.6)), len(symbols) // 2)
                o = rs.randint(0, len(symbols) - w)
                row = np.bincount(symbols[o:o + w], minlength=A)[:A]
                label = "alice window %d+%d" % (o, w)
            rows.append((label, row))
        for mode in (PLAIN, OPT):
            fam = Family("seeded sweep (seed %d)" % SWEEP_SEED, kind, mode, nds)
            for r, (label, row) in enumerate(rows):
                fam.add("%s #%d" % (label, r), row)
            fams.append(fam)
    return fams


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def emulation():
    return emu.lib()


@pytest.fixture(scope="module")
def device():
    import gpulib
    return gpulib.lib()


def run_families(L, fams):
    for fam in fams:
        compare(L, fam)


def run_sweep(L):
    largest = 0
    for fam in sweep_families():
        got = compare(L, fam, " seed %d" % SWEEP_SEED)
        largest = max(largest, int(got[4].max()))
    assert 0 < largest <= emu.TREE_BITS_WORDS * 64, largest


def test_depth_limit_emu(emulation):
    run_families(emulation, depth_limit_families())


def test_sort_and_leaf_build_emu(emulation):
    run_families(emulation, sort_families())


def test_rle_optimiser_emu(emulation):
    run_families(emulation, rle_families())


def test_distance_alphabets_emu(emulation):
    run_families(emulation, distance_families())


def test_seeded_sweep_emu(emulation):
    run_sweep(emulation)


@pytest.mark.gpu
def test_depth_limit_gpu(device):
    run_families(device, depth_limit_families())


@pytest.mark.gpu
def test_sort_and_leaf_build_gpu(device):
    run_families(device, sort_families())


@pytest.mark.gpu
def test_rle_optimiser_gpu(device):
    run_families(device, rle_families())


@pytest.mark.gpu
def test_distance_alphabets_gpu(device):
    run_families(device, distance_families())


@pytest.mark.gpu
def test_seeded_sweep_gpu(device):
    run_sweep(device)


def test_seam_refuses_bad_arguments_emu(emulation):
    import ctypes
    L = emulation
    L.brotli_mi355x_debug_build_codes.restype = ctypes.c_int
    L.brotli_mi355x_debug_build_codes.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p] * 5
    h = np.zeros((1, 704), dtype=np.uint32)
    d = np.zeros((1, 704), dtype=np.uint8)
    b = np.zeros((1, 704), dtype=np.uint16)
    w = np.zeros((1, 64), dtype=np.uint64)
    n = np.zeros(1, dtype=np.uint32)
    ptrs = [x.ctypes.data for x in (h, d, b, w, n)]
    assert L.brotli_mi355x_debug_build_codes(LIT, 544, PLAIN, 1, *ptrs) == 0
    for kind, nds, mode, rows in ((3, 544, PLAIN, 1), (LIT, 544, 2, 1), (LIT, 544, 3, 1), (LIT, 544, 7, 1), (DIST, 15, PLAIN, 1),
                                  (DIST, LARGE_WINDOW_DIST + 1, PLAIN, 1), (CMD, 544, OPT, 0), (CMD, 544, OPT, (1 << 16) + 1)):
        assert L.brotli_mi355x_debug_build_codes(kind, nds, mode, rows, *ptrs) == -1, (kind, nds, mode, rows)
    assert L.brotli_mi355x_debug_build_codes(LIT, 544, PLAIN, 1, None, *ptrs[1:]) == -1
