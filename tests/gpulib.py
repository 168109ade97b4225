"""ctypes binding of the product library rust-brotli_amd/libbrotli_mi355x.so (HIP backed)."""
import ctypes
import os

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BROTLI_MI355X_LIB") or os.path.join(ROOT, "rust-brotli_amd", "libbrotli_mi355x.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("product library not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = emu.bind_trace(ctypes.CDLL(LIB_PATH))
    return _lib


# the introspection seams are the same flat entry points in both libraries: the bindings of emu.py serve lib() as well
build_codes = emu.build_codes
hq_split = emu.hq_split
hq_cluster = emu.hq_cluster
dictionary_matches = emu.dictionary_matches
fast_log2 = emu.fast_log2
literal_costs = emu.literal_costs
cost_from_histogram = emu.cost_from_histogram
