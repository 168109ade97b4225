// tests/emu: same flat entry points as the product library, linked against the CPU emulation seam (the scalar zopfli_debug_* twins)
#include "../../rust-brotli_amd/csrc/zopfli_entry.inc"
