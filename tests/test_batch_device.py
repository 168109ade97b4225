"""BrotliMi355xCompressBatchDevice / Library.compress_batch_device: the batch call on items that lie in device memory, their
streams left in device memory.

Item i is what BrotliEncoderCompress gives on the same bytes (the oracle's stream), whatever route it takes, and
last_batch_info() is that of compress_batch on the same items.  The CPU tests run the emulation library, where device memory is
host memory and a ctypes buffer serves as "device" address: they pin the host plan and the ABI rules.  The GPU tests run the
product library on torch.uint8 CUDA tensors: they pin the kernels -- a copy of n bytes from any address to any address that
writes exactly [dst, dst + n)."""
import ctypes
import functools
import os
import random
import subprocess
import threading
from ctypes import POINTER, c_int32, c_size_t, c_void_p

import pytest

import orc
import synth
import test_batch
import test_cabi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 64
FILL = 0xAA


@functools.lru_cache(maxsize=None)
def _oracle(item, quality, lgwin, mode=0):
    return orc.compress(item, quality, lgwin, mode)


# ---- "device" memory of either library: one buffer, bytes in, bytes out, its address

class _HostMem(object):
    def __init__(self, nbytes, fill=FILL):
        self.buf = (ctypes.c_uint8 * max(1, nbytes))()
        ctypes.memset(self.buf, fill, max(1, nbytes))
        self.ptr = ctypes.addressof(self.buf)

    def write(self, at, data):
        ctypes.memmove(self.ptr + at, data, len(data))

    def read(self):
        return bytes(self.buf)

    @staticmethod
    def sync():
        pass


class _CudaMem(object):
    def __init__(self, nbytes, fill=FILL):
        import torch
        self.t = torch.full((max(1, nbytes),), fill, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def write(self, at, data):
        import torch
        if data:
            self.t[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    def read(self):
        return self.t.cpu().numpy().tobytes()

    @staticmethod
    def sync():
        import torch
        torch.cuda.synchronize()


def _mem(which):
    return _HostMem if which == "emu" else _CudaMem


def _run(lib, Mem, items, caps, quality, lgwin, in_at=None, out_at=None, raises=False, **flags):
    """Lays the items into ONE input buffer (at in_at, default back to back from offset 1) and the outputs into ONE output buffer
    (at out_at, default back to back behind a guard zone), calls compress_batch_device, and returns (sizes, output buffer bytes,
    out_at, info, exception)."""
    if in_at is None:
        in_at, at = [], 1
        for x in items:
            in_at.append(at)
            at += len(x)
    if out_at is None:
        out_at, at = [], GUARD
        for c in caps:
            out_at.append(at)
            at += c
    src = Mem(max([1] + [a + len(x) for a, x in zip(in_at, items)]), 0)
    for a, x in zip(in_at, items):
        src.write(a, x)
    dst = Mem(max([0] + [a + c for a, c in zip(out_at, caps)]) + GUARD)
    Mem.sync()
    error = None
    try:
        sizes = lib.compress_batch_device([(src.ptr + a, len(x)) for a, x in zip(in_at, items)], [(dst.ptr + a, c) for a, c in zip(out_at, caps)],
                                          quality, lgwin, **flags)
    except Exception as e:  # (BrotliCompressorException of the module the library was loaded from)
        if not raises:
            raise
        error, sizes = e, e.sizes
    info = lib.last_batch_info()
    return sizes, dst.read(), out_at, info, error


def _streams(sizes, image, out_at):
    return [image[a:a + n] for a, n in zip(out_at, sizes)]


def _roomy(lib, items):
    return [lib.lib.BrotliEncoderMaxCompressedSize(len(x)) + 16 for x in items]


def _small_items():
    a = synth.alice()
    return [a[7:7 + n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4097)]


# ---- 1. identity per route

# (quality, lgwin, flags, smallest and largest identity item the route takes, most items).  Where every item goes one by one
# (quality 9 without its route) or the small ones do (quick_long_items alone) the cut keeps the emulation's one-shot path short;
# quality 11: a Zopfli walk costs about 37 us per byte.
_ROUTES = [
    (5, 22, {}, 0, 65536, None),
    (8, 17, {}, 0, 65536, None),
    (5, 22, {"long_items": True}, 0, 262144, None),
    (2, 22, {"quick_items": True}, 0, 16384, None),
    (4, 10, {"quick_items": True}, 0, 65536, None),
    (3, 22, {"quick_long_items": True}, 16385, 65536, None),
    (9, 18, {"q9_items": True}, 0, 262144, None),
    (11, 22, {"zopfli_items": True}, 0, 2048, 24),
    (0, 22, {}, 0, 1 << 30, None),
    (1, 18, {}, 0, 1 << 30, None),
    (9, 22, {}, 0, 30000, None),
]
_ROUTE_IDS = ["q%d-w%d-%s" % (q, w, "-".join(sorted(f)) or "plain") for q, w, f, _, _, _ in _ROUTES]


def _route_items(lo, hi, most):
    items = [x for x in test_batch._identity_items(reduced=True) if lo <= len(x) <= hi or not x] + [x for x in _small_items() if len(x) <= hi]
    return items[:most] if most else items


def _identity(which, quality, lgwin, flags, lo, hi, most):
    lib = test_cabi._load(which)
    items = _route_items(lo, hi, most)
    sizes, image, out_at, info, _ = _run(lib, _mem(which), items, _roomy(lib, items), quality, lgwin, **flags)
    for i, (got, x) in enumerate(zip(_streams(sizes, image, out_at), items)):
        assert got == _oracle(x, quality, lgwin), (quality, lgwin, flags, i, len(x))
    lib.compress_batch(items, quality, lgwin, **flags)
    assert info == lib.last_batch_info(), (info, lib.last_batch_info())
    assert info[0] == len(items)


@pytest.mark.parametrize("quality,lgwin,flags,lo,hi,most", _ROUTES, ids=_ROUTE_IDS)
def test_identity_emu(quality, lgwin, flags, lo, hi, most):
    _identity("emu", quality, lgwin, flags, lo, hi, most)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,flags,lo,hi,most", _ROUTES, ids=_ROUTE_IDS)
def test_identity_gpu(quality, lgwin, flags, lo, hi, most):
    _identity("gpu", quality, lgwin, flags, lo, hi, most)


# ---- 2. alignment and neighbours: items back to back from offset 1, outputs back to back with exactly the stream's size

def _seeded_small(seed):
    rng = random.Random(seed)
    text, noise = synth.alice(), synth.random_bytes(1 << 16)
    items = []
    for _ in range(200):
        n, kind = rng.randrange(1, 301), rng.randrange(3)
        off = rng.randrange(0, 60000)
        items.append(text[off:off + n] if kind == 0 else (noise[off:off + n] if kind == 1 else bytes(n)))
    return items


def _misalignments(base, at):
    return {(base + a) & 15 for a in at}


def _neighbours(which, items, quality, lgwin, **flags):
    lib, Mem = test_cabi._load(which), _mem(which)
    want = [_oracle(x, quality, lgwin) for x in items]
    caps = [len(w) for w in want]
    sizes, image, out_at, info, _ = _run(lib, Mem, items, caps, quality, lgwin, **flags)
    assert sizes == caps
    assert image == bytes([FILL]) * GUARD + b"".join(want) + bytes([FILL]) * GUARD
    assert info[1] == len(items), info  # (all side by side: the kernels wrote them)
    # an odd stride between the items and a one-byte gap between the outputs: every gap byte survives
    stride = 7 + 2 * (max(len(x) for x in items) // 2) + 2
    in_at = [3 + i * stride for i in range(len(items))]
    out_at, at = [], GUARD
    for c in caps:
        out_at.append(at)
        at += c + 1
    sizes, image, out_at, info, _ = _run(lib, Mem, items, caps, quality, lgwin, in_at=in_at, out_at=out_at, **flags)
    assert sizes == caps
    assert image == bytes([FILL]) * GUARD + b"".join(w + bytes([FILL]) for w in want) + bytes([FILL]) * (GUARD - 1)


def _aligned_everywhere(which, quality, lgwin):
    """~200 items of 1 .. 300 bytes, reseeded here on the CPU until the sources and the destinations of the first layout show every
    misalignment 0 .. 15 (buffers of either kind start on a 16-byte boundary at least: checked)"""
    Mem = _mem(which)
    probe = Mem(64)
    assert probe.ptr % 16 == 0
    for seed in range(100):
        items = _seeded_small(seed)
        in_at, out_at, a, b = [], [], 1, GUARD
        for x in items:
            in_at.append(a)
            out_at.append(b)
            a += len(x)
            b += len(_oracle(x, quality, lgwin))
        if len(_misalignments(0, in_at)) == 16 and len(_misalignments(0, out_at)) == 16:
            return items
    raise AssertionError("no seed gives every misalignment")


_NEIGHBOUR_CASES = [(5, 22, {}), (2, 22, {"quick_items": True})]


@pytest.mark.parametrize("quality,lgwin,flags", _NEIGHBOUR_CASES, ids=["q5", "q2-quick"])
def test_alignment_and_neighbours_emu(quality, lgwin, flags):
    _neighbours("emu", _aligned_everywhere("emu", quality, lgwin), quality, lgwin, **flags)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,flags", _NEIGHBOUR_CASES, ids=["q5", "q2-quick"])
def test_alignment_and_neighbours_gpu(quality, lgwin, flags):
    _neighbours("gpu", _aligned_everywhere("gpu", quality, lgwin), quality, lgwin, **flags)


def _long_items():
    # five items of 65 537 .. 70 001 bytes: two input blocks each, the context bytes of the second gathered at the block boundary
    t = synth.markov_text(400000, 17)
    return [t[off:off + n] for off, n in ((0, 65537), (70001, 66001), (140003, 67890), (210007, 69999), (290011, 70001))]


def test_alignment_and_neighbours_long_emu():
    _neighbours("emu", _long_items(), 5, 22, long_items=True)


@pytest.mark.gpu
def test_alignment_and_neighbours_long_gpu():
    _neighbours("gpu", _long_items(), 5, 22, long_items=True)


# ---- 3. ABI semantics: the body of test_batch_greedy._abi_semantics on device memory

def _raw_device(lib, Mem, quality, lgwin, items, caps, routes=0, with_results=True):
    """BrotliMi355xCompressBatchDevice through ctypes.  Every output lies between two sentinel zones of its own.
    Returns (return value, [stream], [item result], [size], sentinels intact)."""
    n = len(items)
    in_at, at = [], 1
    for x in items:
        in_at.append(at)
        at += len(x)
    src = Mem(at, 0)
    for a, x in zip(in_at, items):
        src.write(a, x)
    out_at, at = [], GUARD
    for c in caps:
        out_at.append(at)
        at += c + GUARD
    dst = Mem(at)
    Mem.sync()
    inputs = (c_void_p * max(1, n))(*[src.ptr + a for a in in_at])
    in_sizes = (c_size_t * max(1, n))(*[len(x) for x in items])
    outputs = (c_void_p * max(1, n))(*[dst.ptr + a for a in out_at])
    out_sizes = (c_size_t * max(1, n))(*caps)
    results = (c_int32 * max(1, n))(*([7] * n))
    ret = lib.lib.BrotliMi355xCompressBatchDevice(quality, lgwin, 0, routes, n, inputs, in_sizes, outputs, out_sizes,
                                                  results if with_results else ctypes.cast(None, POINTER(c_int32)))
    image = dst.read()
    intact = image[:GUARD] == bytes([FILL]) * GUARD and all(image[a + c:a + c + GUARD] == bytes([FILL]) * GUARD for a, c in zip(out_at, caps))
    return ret, [image[out_at[i]:out_at[i] + out_sizes[i]] for i in range(n)], list(results)[:n], list(out_sizes)[:n], intact


def _abi_semantics(which, quality=5):
    lib, Mem = test_cabi._load(which), _mem(which)
    _raw_one = test_batch._raw_one
    max_size = lib.lib.BrotliEncoderMaxCompressedSize
    items = [synth.alice()[:9000], b"", synth.random_bytes(5000), synth.markov_text(700, 9), b"q"]
    roomy = [max_size(len(x)) + 16 for x in items]
    ret, outs, results, sizes, intact = _raw_device(lib, Mem, quality, 22, items, roomy)
    assert ret == 1 and results == [1] * len(items) and intact
    assert lib.last_batch_info()[:4] == [5, 4, 0, 1]
    assert outs[1] == b"\x06"  # the empty item, in device memory
    for x, cap, out in zip(items, roomy, outs):
        assert (1, out) == _raw_one(lib, quality, 22, x, cap)
    # a buffer too small for item k fails k alone (capacity 0 included), and the call returns 0
    for k, cap in ((0, 100), (3, 5), (1, 0), (2, 1000)):
        caps = list(roomy)
        caps[k] = cap
        assert _raw_one(lib, quality, 22, items[k], cap)[0] == 0
        ret, got, results, sizes, intact = _raw_device(lib, Mem, quality, 22, items, caps)
        assert ret == 0 and intact
        assert results == [0 if i == k else 1 for i in range(len(items))]
        assert sizes[k] == 0
        assert [g for i, g in enumerate(got) if i != k] == [o for i, o in enumerate(outs) if i != k]
    assert _raw_device(lib, Mem, quality, 22, [], [])[0] == 1
    ret, got, _, _, intact = _raw_device(lib, Mem, quality, 22, items, roomy, with_results=False)
    assert ret == 1 and got == outs and intact
    # an unknown route bit fails the whole call and sets only info[0]
    for routes in (2, 8, 64, 256):
        ret, got, results, sizes, intact = _raw_device(lib, Mem, quality, 22, items, roomy, routes=routes)
        assert ret == 0 and results == [0] * len(items) and sizes == [0] * len(items) and intact
        assert lib.last_batch_info() == [len(items), 0, 0, 0, 0, 0, 0, 0]
    # an incompressible item of one input block in a buffer of exactly BrotliEncoderMaxCompressedSize bytes
    noise = synth.random_bytes(60000)
    cap = max_size(len(noise))
    ok, want = _raw_one(lib, quality, 22, noise, cap)
    ret, got, results, _, intact = _raw_device(lib, Mem, quality, 22, [b"abc", noise], [64, cap])
    assert ok == 1 and ret == 1 and results == [1, 1] and got[1] == want and intact
    assert lib.last_batch_info()[1] == 2
    assert orc.decompress(want, len(noise)) == noise


def test_abi_semantics_emu():
    _abi_semantics("emu")


@pytest.mark.gpu
def test_abi_semantics_gpu():
    _abi_semantics("gpu")


def test_python_raises_with_failed_and_sizes_emu():
    lib = test_cabi._load("emu")
    items = [synth.alice()[:3000], b"abc", synth.alice()[:100]]
    caps = _roomy(lib, items)
    caps[1] = 2
    sizes, image, out_at, info, error = _run(lib, _HostMem, items, caps, 5, 22, raises=True)
    assert error is not None and error.failed == [1] and error.sizes == sizes
    assert sizes == [len(_oracle(items[0], 5, 22)), 0, len(_oracle(items[2], 5, 22))]


# ---- 4. mixed call: the empty item, one block, three blocks, five blocks (one by one through the device one-shot path)

def _mixed(which):
    lib = test_cabi._load(which)
    t = synth.markov_text(5 * 65536, 23)
    items = [t[:4 * 65536 + 1000], b"", t[1000:1000 + 2 * 65536 + 500], t[7:5007]]
    sizes, image, out_at, info, _ = _run(lib, _mem(which), items, _roomy(lib, items), 5, 22, long_items=True)
    for i, (got, x) in enumerate(zip(_streams(sizes, image, out_at), items)):
        assert got == _oracle(x, 5, 22), (i, len(x))
    assert info[:4] == [4, 2, 1, 1] and info[7] == 1, info
    lib.compress_batch(items, 5, 22, long_items=True)
    assert info == lib.last_batch_info()


def test_mixed_emu():
    _mixed("emu")


@pytest.mark.gpu
def test_mixed_gpu():
    _mixed("gpu")


# ---- 5. stored-stream fallback.  A seeded search with the oracle (10 000 items of at most 4 KiB -- noise, noise and text, noise
# and zeros -- at qualities 0 .. 11) found no input whose stream exceeds BrotliEncoderMaxCompressedSize, so the branch is covered
# by calling the factored delivery rule and the device writer of the stored stream directly, from a stand-alone host program
# (batch_device_check.cpp) over the emulation library; the stream it leaves must decode to the input.

def _check_program(tmp_path_factory):
    import emu
    emu.build()
    exe = str(tmp_path_factory.mktemp("batch_device_check") / "batch_device_check")
    cmd = ["g++", "-std=c++17", "-O1", "-DBROTLI_HOST_EMU=1", "-I", os.path.join(ROOT, "rust-brotli_amd", "csrc"), os.path.join(HERE, "batch_device_check.cpp"),
           os.path.join(emu.EMU_DIR, "libbrotli_emu.so"), "-Wl,-rpath," + emu.EMU_DIR, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return _check_program(tmp_path_factory)


@pytest.mark.parametrize("nbytes", [1, 4096, 65536, 65537, (1 << 20) + 1])
def test_stored_fallback_program_emu(check_program, nbytes):
    r = subprocess.run([check_program, "stored", str(nbytes)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("stored "), r.stdout[-2000:] + r.stderr[-2000:]
    _, size, digits = r.stdout.split()
    stream = bytes.fromhex(digits)
    assert len(stream) == int(size) and stream[:2] == b"\x21\x03" and stream[-1] == 3
    assert len(stream) <= test_cabi._load("emu").lib.BrotliEncoderMaxCompressedSize(nbytes)
    item = orc.decompress(stream, nbytes)
    assert len(item) == nbytes and item in stream  # (stored: the input lies in the stream as it is)


def test_exact_heap_blocks_program_emu(check_program):
    # every item and every output in a heap block of exactly its size (the layouts a sanitizer build of the program judges)
    r = subprocess.run([check_program, "layouts"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 6. memory: every failed allocation fails the call, and no block stays live

@pytest.mark.parametrize("quality,flags", [(5, {}), (2, {"quick_items": True})], ids=["q5", "q2-quick"])
def test_failed_call_frees_its_blocks_emu(quality, flags):
    import test_device_memory
    lib = test_cabi._load("emu")
    L = lib.lib
    L.brotli_emu_live_blocks.restype = ctypes.c_long
    L.brotli_emu_alloc_count.restype = ctypes.c_long
    L.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    L.brotli_emu_fail_alloc.restype = None
    exc = type(lib).compress_batch.__globals__["BrotliCompressorException"]
    items = [synth.alice()[:12000], b"tiny", synth.markov_text(9000, 3), synth.random_bytes(3000)]
    caps = _roomy(lib, items)

    def call():
        sizes, image, out_at, info, _ = _run(lib, _HostMem, items, caps, quality, 22, **flags)
        assert info[:5] == [4, 4, 0, 0, 1]
        return b"|".join(_streams(sizes, image, out_at))

    test_device_memory.sweep(L, call, exc)


# ---- 7. threads: two threads, each with its own call of 64 items and its own tensors

@pytest.mark.gpu
def test_threads_gpu():
    lib = test_cabi._load("gpu")
    batches = [test_batch._seeded_items(64, 100, 20000, 31 + t) for t in range(2)]
    want = [[_oracle(x, 5, 22) for x in b] for b in batches]
    got, errors = [None] * 2, []

    def work(t):
        try:
            sizes, image, out_at, info, _ = _run(lib, _CudaMem, batches[t], _roomy(lib, batches[t]), 5, 22)
            got[t] = (_streams(sizes, image, out_at), info[:4])
        except Exception as e:  # (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(600)
    assert not errors, errors
    for t in range(2):
        side = sum(1 for x in batches[t] if x)
        assert got[t][0] == want[t]
        assert got[t][1] == [64, side, 0, 64 - side], got[t][1]
