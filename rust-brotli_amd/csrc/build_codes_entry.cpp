// build_codes_entry.cpp -- exports brotli_mi355x_debug_build_codes from the product library (HIP backed).
#include "build_codes_entry.inc"
