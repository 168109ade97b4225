"""Device memory has one scoped owner (DevBlocks, device_api.h): a call that fails gives back every block it took.

The emulation library counts live blocks and allocations and can make the k-th allocation from now throw
(tests/emu/device_emu.cpp, brotli_emu_*).  Every sweep below runs one clean call, takes its number of allocations N, and then
fails the call at EVERY allocation 1..N: the call must report the failure and the live count must be back where it was before the
call.  Afterwards the same call must still produce the same bytes."""
import ctypes
import importlib.util
import os

import pytest

import emu
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
Q, W = 1, 2


@pytest.fixture(scope="module")
def L():
    lib = emu.lib()
    lib.brotli_emu_live_blocks.restype = ctypes.c_long
    lib.brotli_emu_alloc_count.restype = ctypes.c_long
    lib.brotli_emu_fail_alloc.argtypes = [ctypes.c_long]
    lib.brotli_emu_fail_alloc.restype = None
    return lib


@pytest.fixture(scope="module")
def cabi(L):
    """the Python binding of the product over the emulation library (the same shared object as L: one set of counters)"""
    path = os.path.join(emu.EMU_DIR, "libbrotli_emu.so")
    spec = importlib.util.spec_from_file_location("brotli_mi355x_emu_mem", os.path.join(ROOT, "rust-brotli_amd", "brotli_mi355x", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BROTLI_MI355X_LIB", path)  # (the module insists on its default library at import: this copy's is the emulation)
        spec.loader.exec_module(mod)
    return mod, mod.Library(path)


def sweep(L, call, failure):
    """call() -> bytes; raises `failure` when the library reports an error"""
    clean = call()  # warm: what a process allocates once (tables, thread-local scratch) is there afterwards
    live = L.brotli_emu_live_blocks()
    before = L.brotli_emu_alloc_count()
    assert call() == clean
    n = L.brotli_emu_alloc_count() - before
    assert n > 0
    assert L.brotli_emu_live_blocks() == live
    try:
        for k in range(1, n + 1):
            L.brotli_emu_fail_alloc(k)
            with pytest.raises(failure):
                call()
            leaked = L.brotli_emu_live_blocks() - live
            assert leaked == 0, "a failure at allocation %d of %d leaves %d blocks live" % (k, n, leaked)
    finally:
        L.brotli_emu_fail_alloc(0)
    assert call() == clean
    assert L.brotli_emu_live_blocks() == live


@pytest.mark.parametrize("quality", [2, 4, 5, 9, 10])
def test_failed_oneshot_call_frees_its_blocks(L, quality):
    data = synth.alice()[:20000]
    sweep(L, lambda: emu.encode_stream(L, data, [(Q, quality), (W, 22)])[0], RuntimeError)


def test_failed_oneshot_call_frees_its_blocks_live_chains(L, monkeypatch):
    monkeypatch.setenv("BROTLI_MI355X_LIVE", "1")  # (read at every Setup: any input goes down the live-chain path)
    data = synth.alice()[:20000]
    sweep(L, lambda: emu.encode_stream(L, data, [(Q, 5), (W, 22)])[0], RuntimeError)


@pytest.mark.parametrize("quality", [0, 1])
def test_failed_fragment_call_frees_its_blocks(L, cabi, quality):
    mod, lib = cabi
    data = synth.alice()[:20000]
    sweep(L, lambda: lib.compress(data, quality, 22), mod.BrotliCompressorException)


def _stream(mod, lib, L, quality, pieces, fail_in_second=0):
    """PROCESS / FLUSH pieces, FINISH, destroy; with fail_in_second = k the k-th allocation of the second piece throws.
    Returns (bytes or None, allocations of the second piece)."""
    enc = mod.Encoder(lib, [(Q, quality), (W, 22)])
    out = b""
    allocs = 0
    try:
        for i, piece in enumerate(pieces):
            half = len(piece) // 2
            before = L.brotli_emu_alloc_count()
            if i == 1:
                L.brotli_emu_fail_alloc(fail_in_second)
            try:
                enc.write(piece[:half])
                out += enc.flush(piece[half:])
            finally:
                if i == 1:
                    L.brotli_emu_fail_alloc(0)
                    allocs = L.brotli_emu_alloc_count() - before
        out += enc.finish()
        return out, allocs
    finally:
        enc.close()


@pytest.mark.parametrize("quality", [2, 5, 10])
def test_stream_frees_its_blocks_and_carries(L, cabi, quality):
    mod, lib = cabi
    text = synth.alice()
    pieces = [text[i * 30000:(i + 1) * 30000] for i in range(4)]
    clean, _ = _stream(mod, lib, L, quality, pieces)  # warm
    live = L.brotli_emu_live_blocks()
    again, n = _stream(mod, lib, L, quality, pieces)
    assert again == clean
    assert L.brotli_emu_live_blocks() == live
    assert n > 0
    for k in range(1, n + 1):
        with pytest.raises(mod.BrotliCompressorException):
            _stream(mod, lib, L, quality, pieces, fail_in_second=k)
        leaked = L.brotli_emu_live_blocks() - live
        assert leaked == 0, "a failure at allocation %d of %d of the second piece leaves %d blocks live" % (k, n, leaked)
    assert _stream(mod, lib, L, quality, pieces)[0] == clean
    assert L.brotli_emu_live_blocks() == live
