// fragment_seam_emu.inc -- host emulation of the batch seam of qualities 0 and 1 (fragment_api.h: frag_compress_jobs,
// frag_join_bounded), compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu; fragment_stream.cpp includes it there):
// the same item code (fragment_device.h) on plain memory, one fragment after the other, in the order of the index list.  A table
// that the kernel keeps in workgroup memory lives in a thread-local array here, and the item code zeroes what it uses of it.
#include <string.h>

#include <stdexcept>

#include "fragment_device.h"

namespace brotli_mi355x {

void frag_compress_jobs(int quality, const uint8_t* input, const FragmentJob* jobs, const uint32_t* order, uint32_t n, uint32_t workgroup_table_bits,
                        const FragmentBuffers& B, const FragmentState* states_in, FragmentState* states_out, FragmentResult* results, uint8_t* out) {
  if (workgroup_table_bits > kFragmentWorkgroupTableBitsMax) throw std::runtime_error("brotli_mi355x: a fragment table of this size does not fit workgroup memory");
  const DeviceTables& dt = dev_tables();
  EntropyTables et;
  et.logs_16 = dt.logs_16;
  et.logs_8 = dt.logs_8;
  static thread_local FragmentScratch S;
  static thread_local uint64_t cmd_code_words[kTreeBitsWords];
  static thread_local uint32_t workgroup_table[1u << kFragmentWorkgroupTableBitsMax];
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t j = order ? order[k] : k;
    if (workgroup_table_bits != 0) {
      if (jobs[j].table_bits > workgroup_table_bits) throw std::runtime_error("brotli_mi355x: a fragment's table is larger than its class");
      memset(workgroup_table, 0xa5, (size_t)4 << workgroup_table_bits);  // (whatever the last workgroup left there)
      br_fragment_job(quality, et, input, jobs[j], j, B, FrTableWorkgroup{workgroup_table}, states_in, states_out, results, out, S, cmd_code_words);
    } else {
      memset(fr_table_slab(B, jobs[j], j).p, 0, ((size_t)1 << jobs[j].table_bits) * 4);
      br_fragment_job(quality, et, input, jobs[j], j, B, states_in, states_out, results, out, S, cmd_code_words);
    }
  }
}

void frag_join_bounded(const uint8_t* src, const FragmentPiece* pieces, uint32_t n, uint8_t* dst, uint64_t) { frag_join(src, pieces, n, dst); }

}  // namespace brotli_mi355x
