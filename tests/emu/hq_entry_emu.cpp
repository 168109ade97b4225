// tests/emu: same flat entry points as the product library, linked against the CPU emulation seam (the scalar mb_hq_* twins)
#include "../../rust-brotli_amd/csrc/hq_entry.inc"
