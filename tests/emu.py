"""ctypes binding of tests/emu/libbrotli_emu.so: the product's host driver + chain code compiled for
the CPU (one lane per wave).  Test infrastructure only."""
import ctypes, os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")


class Command(ctypes.Structure):
    _fields_ = [("insert_len_", ctypes.c_uint32), ("copy_len_", ctypes.c_uint32), ("dist_extra_", ctypes.c_uint32),
                ("cmd_prefix_", ctypes.c_uint16), ("dist_prefix_", ctypes.c_uint16)]


class MetaBlockInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("start", "end", "cmd_offset", "n_cmds", "n_literals", "uncompressed",
                                               "is_last", "pad")] + [("dist_cache_after", ctypes.c_int32 * 4)]


def build():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])


def bind_trace(L):
    L.brotli_mi355x_lz77_trace.restype = ctypes.c_long
    L.brotli_mi355x_lz77_trace.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p,
                                           ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(Command), ctypes.c_size_t, ctypes.POINTER(MetaBlockInfo),
                                           ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = bind_trace(ctypes.CDLL(os.path.join(EMU_DIR, "libbrotli_emu.so")))
    return _lib


def lz77_trace(L, data, quality=5, lgwin=22, size_hint=None, catable=False, prefix=b"", segment_bytes=4096):
    """returns (metablocks, stats): metablocks = list of dict(start,end,uncompressed,cmds=[tuples],dist_cache_after)"""
    if size_hint is None:
        size_hint = len(data)
    cap = len(data) // 2 + len(data) // 65536 * 4 + 1024
    cmds = (Command * cap)()
    mbs = (MetaBlockInfo * 4096)()
    nmb = ctypes.c_size_t(0)
    stats = (ctypes.c_uint32 * 12)()
    err = ctypes.create_string_buffer(512)
    n = L.brotli_mi355x_lz77_trace(quality, lgwin, size_hint, 1 if catable else 0, prefix, len(prefix), data, len(data),
                                   segment_bytes, cmds, cap, mbs, 4096, ctypes.byref(nmb), stats, err, 512)
    if n < 0:
        raise RuntimeError(err.value.decode())
    out = []
    for i in range(nmb.value):
        m = mbs[i]
        cl = [(cmds[j].insert_len_, cmds[j].copy_len_, cmds[j].dist_extra_, cmds[j].cmd_prefix_, cmds[j].dist_prefix_)
              for j in range(m.cmd_offset, m.cmd_offset + m.n_cmds)]
        out.append(dict(start=m.start, end=m.end, uncompressed=bool(m.uncompressed), is_last=bool(m.is_last), cmds=cl,
                        n_literals=m.n_literals, dist_cache_after=tuple(m.dist_cache_after)))
    names = ('keys', 'sort', 'init', 'rank', 'parse', 'resolve', 'gather', 'total')
    return out, dict(rounds=stats[0], segments_parsed=stats[1], searches=stats[2], total_cmds=stats[3],
                     ms={n: stats[4 + i] / 1000.0 for i, n in enumerate(names)})


def bind_encode(L):
    L.brotli_mi355x_encode_stream.restype = ctypes.c_long
    L.brotli_mi355x_encode_stream.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32,
                                              ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double),
                                              ctypes.c_char_p, ctypes.c_size_t]
    return L


def encode_stream(L, data, params, prefix=b"", continuation=True, segment_bytes=0):
    """params: list of (BrotliEncoderParameter id, value).  Returns (bytes, stats dict)."""
    bind_encode(L)
    keys = (ctypes.c_int * len(params))(*[k for k, _ in params])
    vals = (ctypes.c_uint32 * len(params))(*[v for _, v in params])
    cap = len(data) + len(data) // 4 + 4096
    out = ctypes.create_string_buffer(cap)
    st = (ctypes.c_double * 32)()
    err = ctypes.create_string_buffer(512)
    buf = ctypes.create_string_buffer(data, len(data) if data else 1)
    n = L.brotli_mi355x_encode_stream(keys, vals, len(params), prefix, len(prefix), 1 if continuation else 0,
                                      ctypes.cast(buf, ctypes.c_void_p), len(data), 0, segment_bytes, out, cap, st, err, 512)
    if n < 0:
        raise RuntimeError(err.value.decode())
    names = ["lz77_rounds", "searches", "commands", "literals", "metablocks", "uncompressed_metablocks",
             "fallback_retries", "ms_lz77", "ms_metablock", "ms_total"]
    d = {k: st[i] for i, k in enumerate(names)}
    d["ms_phase"] = [st[10 + i] for i in range(16)]
    d["chains_launched"] = st[28]  # over all launches: warm-up dry runs, round 0, re-parses
    d["num_segments"] = st[29]
    return out.raw[:n], d


ROW_LEN = (256, 704, 544)  # kRowLen: literal, command, distance histogram rows
TREE_BITS_WORDS = 64       # kTreeBitsWords
CODE_OPTIMIZED, CODE_PLAIN = 0, 1


def build_codes(L, kind, num_distance_symbols, mode, histograms):
    """brotli_mi355x_debug_build_codes: `histograms` (numpy uint32, n_rows x ROW_LEN[kind]) through the prefix-code builder of the
    library (k_build_codes on the device, the scalar form in the emulation).  Returns (histograms after, depth, bits, tree bytes
    [n_rows x 512], tree_nbits) as numpy arrays."""
    import numpy as np
    L.brotli_mi355x_debug_build_codes.restype = ctypes.c_int
    L.brotli_mi355x_debug_build_codes.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p] * 5
    h = np.array(histograms, dtype=np.uint32, order="C")
    n = h.shape[0]
    assert h.shape == (n, ROW_LEN[kind])
    depth = np.full((n, ROW_LEN[kind]), 0xee, dtype=np.uint8)
    bits = np.full((n, ROW_LEN[kind]), 0xeeee, dtype=np.uint16)
    words = np.full((n, TREE_BITS_WORDS), 0xeeeeeeeeeeeeeeee, dtype=np.uint64)
    nbits = np.full(n, 0xeeeeeeee, dtype=np.uint32)
    r = L.brotli_mi355x_debug_build_codes(kind, num_distance_symbols, mode, n, h.ctypes.data, depth.ctypes.data, bits.ctypes.data,
                                          words.ctypes.data, nbits.ctypes.data)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_build_codes returned %d" % r)
    return h, depth, bits, words.view(np.uint8).reshape(n, TREE_BITS_WORDS * 8), nbits


def hq_split_raw(L, kind, n_jobs, lengths, symbols):
    """brotli_mi355x_debug_hq_split as it is: returns (status, phase1_blocks, phase1_ids, num_types, num_blocks, types, block_lengths)."""
    import numpy as np
    L.brotli_mi355x_debug_hq_split.restype = ctypes.c_int
    L.brotli_mi355x_debug_hq_split.argtypes = [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 8
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    symbols = np.ascontiguousarray(symbols, dtype=np.uint16)
    total = max(1, len(symbols))
    n = max(1, len(lengths))
    p1n = np.full(n, 0xeeeeeeee, dtype=np.uint32)
    p1 = np.full(total, 0xee, dtype=np.uint8)
    nt = np.full(n, 0xeeeeeeee, dtype=np.uint32)
    nb = np.full(n, 0xeeeeeeee, dtype=np.uint32)
    types = np.full(total, 0xee, dtype=np.uint8)
    bl = np.full(total, 0xeeeeeeee, dtype=np.uint32)
    r = L.brotli_mi355x_debug_hq_split(kind, n_jobs, lengths.ctypes.data, symbols.ctypes.data, p1n.ctypes.data, p1.ctypes.data,
                                       nt.ctypes.data, nb.ctypes.data, types.ctypes.data, bl.ctypes.data)
    return r, p1n, p1, nt, nb, types, bl


def hq_split(L, kind, vectors):
    """`vectors` (sequences of symbols of one kind: 0 literals, 1 commands, 2 distance prefixes) through FindBlocks + ClusterBlocks of
    the library (k_hq_* on the device, the scalar twins in the emulation), side by side in one launch.  Returns one dict per vector:
    phase1_blocks, phase1_ids (numpy uint8, after mb_hq_find_blocks), num_types, num_blocks, types, lengths (the final split)."""
    import numpy as np
    vectors = [np.asarray(v, dtype=np.uint16) for v in vectors]
    lengths = np.array([len(v) for v in vectors], dtype=np.uint32)
    symbols = np.concatenate(vectors) if vectors else np.zeros(0, dtype=np.uint16)
    r, p1n, p1, nt, nb, types, bl = hq_split_raw(L, kind, len(vectors), lengths, symbols)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_hq_split returned %d" % r)
    out, at = [], 0
    for i, v in enumerate(vectors):
        out.append(dict(phase1_blocks=int(p1n[i]), phase1_ids=p1[at:at + len(v)].copy(), num_types=int(nt[i]), num_blocks=int(nb[i]),
                        types=types[at:at + int(nb[i])].copy(), lengths=bl[at:at + int(nb[i])].copy()))
        at += len(v)
    return out


def hq_cluster_raw(L, kind, n_jobs, in_sizes, rows, expand64):
    """brotli_mi355x_debug_hq_cluster as it is: returns (status, out_count, out_rows, out_total, out_cost, slot_cost, map)."""
    import numpy as np
    L.brotli_mi355x_debug_hq_cluster.restype = ctypes.c_int
    L.brotli_mi355x_debug_hq_cluster.argtypes = [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 9
    in_sizes = np.ascontiguousarray(in_sizes, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    expand64 = np.ascontiguousarray(expand64, dtype=np.uint32)
    total = max(1, rows.shape[0] if rows.ndim == 2 else 0)
    count = np.full(max(1, len(in_sizes)), 0xeeeeeeee, dtype=np.uint32)
    out_rows = np.full((total, ROW_LEN[kind] if kind < 3 else 1), 0xeeeeeeee, dtype=np.uint32)
    out_total = np.full(total, 0xeeeeeeee, dtype=np.uint32)
    out_cost = np.full(total, 0xeeeeeeee, dtype=np.uint32)
    slot_cost = np.full(total, 0xeeeeeeee, dtype=np.uint32)
    cmap = np.full(total * 64, 0xeeeeeeee, dtype=np.uint32)
    r = L.brotli_mi355x_debug_hq_cluster(kind, n_jobs, in_sizes.ctypes.data, rows.ctypes.data, expand64.ctypes.data, count.ctypes.data,
                                         out_rows.ctypes.data, out_total.ctypes.data, out_cost.ctypes.data, slot_cost.ctypes.data,
                                         cmap.ctypes.data)
    return r, count, out_rows, out_total, out_cost, slot_cost, cmap


def hq_cluster(L, kind, jobs, expand64=None):
    """`jobs` (numpy uint32 arrays of in_size x ROW_LEN[kind], kind 0 literal or 2 distance) through BrotliClusterHistograms of the
    library, side by side in one launch.  Returns one dict per job: rows (out_count x len), totals, costs (uint32 bit patterns of the
    output rows' cached costs), slot_costs (bit patterns, one per input slot, behind the remap) and map (in_size entries, 64 x in_size
    where expand64[i] is set)."""
    import numpy as np
    jobs = [np.ascontiguousarray(j, dtype=np.uint32) for j in jobs]
    for j in jobs:
        assert j.ndim == 2 and j.shape[1] == ROW_LEN[kind], j.shape
    if expand64 is None:
        expand64 = [0] * len(jobs)
    in_sizes = [j.shape[0] for j in jobs]
    r, count, out_rows, out_total, out_cost, slot_cost, cmap = hq_cluster_raw(L, kind, len(jobs), in_sizes, np.concatenate(jobs),
                                                                              expand64)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_hq_cluster returned %d" % r)
    out, at, mat = [], 0, 0
    for i, j in enumerate(jobs):
        n, msz = int(count[i]), in_sizes[i] * (64 if expand64[i] else 1)
        out.append(dict(rows=out_rows[at:at + n].copy(), totals=out_total[at:at + n].copy(), costs=out_cost[at:at + n].copy(),
                        slot_costs=slot_cost[at:at + in_sizes[i]].copy(), map=cmap[mat:mat + msz].copy()))
        at += in_sizes[i]
        mat += msz
    return out


DICT_WORDS = 38  # dict_matches[0 .. 37]


def dictionary_matches_raw(L, text, at, min_length, max_length):
    """brotli_mi355x_debug_dictionary_matches as it is: returns (status, matches [n x 38], any [n])."""
    import numpy as np
    f = L.brotli_mi355x_debug_dictionary_matches
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    text = bytes(text)
    at = np.ascontiguousarray(at, dtype=np.uint32)
    lo = np.ascontiguousarray(min_length, dtype=np.uint32)
    hi = np.ascontiguousarray(max_length, dtype=np.uint32)
    n = len(at)
    assert len(lo) == n and len(hi) == n
    out = np.full((max(n, 1), DICT_WORDS), 0xeeeeeeee, dtype=np.uint32)
    anyv = np.full(max(n, 1), 0xeeeeeeee, dtype=np.uint32)
    r = f(text, len(text), n, at.ctypes.data, lo.ctypes.data, hi.ctypes.data, out.ctypes.data, anyv.ctypes.data)
    return r, out[:n], anyv[:n]


def dictionary_matches(L, text, at, min_length, max_length):
    """z_find_all_dictionary_matches of the library at every text + at[q] (one query per lane on the device), one launch.  Returns
    (matches [n x 38] numpy uint32 -- 0x0fffffff where no word matches that length --, any [n])."""
    r, out, anyv = dictionary_matches_raw(L, text, at, min_length, max_length)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_dictionary_matches returned %d" % r)
    return out, anyv


def fast_log2(L, mode, values):
    """brotli_mi355x_debug_fast_log2: mode 0 z_fast_log2, 1 br_fast_log2 of the low 32 bits, 2 logs_16[v & 0xffff]; bit patterns"""
    import numpy as np
    f = L.brotli_mi355x_debug_fast_log2
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    v = np.ascontiguousarray(values, dtype=np.uint64)
    out = np.full(max(1, len(v)), 0xeeeeeeee, dtype=np.uint32)
    r = f(mode, len(v), v.ctypes.data, out.ctypes.data)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_fast_log2 returned %d" % r)
    return out[:len(v)]


def literal_costs(L, blocks):
    """brotli_mi355x_debug_literal_costs of the blocks (bytes, 1 .. 65536 each), one launch.  Returns one (cost bits [len], prefix bits
    [len + 1]) pair per block."""
    import numpy as np
    f = L.brotli_mi355x_debug_literal_costs
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    lengths = np.array([len(b) for b in blocks], dtype=np.uint32)
    data = b"".join(bytes(b) for b in blocks)
    cost = np.full(max(1, len(data)), 0xeeeeeeee, dtype=np.uint32)
    prefix = np.full(len(data) + len(blocks) + 1, 0xeeeeeeee, dtype=np.uint32)
    r = f(len(blocks), lengths.ctypes.data, data, cost.ctypes.data, prefix.ctypes.data)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_literal_costs returned %d" % r)
    out, at = [], 0
    for j, b in enumerate(blocks):
        out.append((cost[at:at + len(b)].copy(), prefix[at + j:at + j + len(b) + 1].copy()))
        at += len(b)
    return out


def cost_from_histogram(L, rows, literal):
    """brotli_mi355x_debug_cost_from_histogram of the rows (numpy uint32, 1 .. 1200 counts each; literal[j]: a literal histogram), one
    launch.  Returns the bit patterns of the costs, one array per row."""
    import numpy as np
    f = L.brotli_mi355x_debug_cost_from_histogram
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    rows = [np.ascontiguousarray(r, dtype=np.uint32) for r in rows]
    sizes = np.array([len(r) for r in rows], dtype=np.uint32)
    lit = np.array([1 if x else 0 for x in literal], dtype=np.uint32)
    flat = np.concatenate(rows)
    cost = np.full(len(flat), 0xeeeeeeee, dtype=np.uint32)
    r = f(len(rows), sizes.ctypes.data, lit.ctypes.data, flat.ctypes.data, cost.ctypes.data)
    if r != 0:
        raise RuntimeError("brotli_mi355x_debug_cost_from_histogram returned %d" % r)
    return np.split(cost, np.cumsum(sizes)[:-1])
