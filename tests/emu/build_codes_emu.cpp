// tests/emu: same flat entry point as the product library, linked against the CPU emulation seam (the scalar mb_build_codes)
#include "../../rust-brotli_amd/csrc/build_codes_entry.inc"
