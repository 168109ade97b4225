// batch_greedy_emu.inc -- host emulation of the batch seam of qualities 5 .. 8 (batch_greedy.h: lz77_batch_parse,
// lz77_batch_gather), compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu; batch_greedy.inc includes it there): the
// same item code (batch_greedy_device.h) on plain memory, one item after the other in the order of the plan, the tables taken in
// turn -- so that a table serves several items, as on the device.
#include <stdexcept>

#include "batch_greedy_device.h"
#include "device_api.h"

namespace brotli_mi355x {

void lz77_batch_parse(const BatchParseJob& J) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  if (J.P.block_bits > 7) throw std::runtime_error("brotli_mi355x: the batch chains do not run the 512-deep rings");
  const DeviceTables& dt = dev_tables();
  ChainTables T;
  T.text = J.text;
  T.info = nullptr;
  T.sorted = nullptr;
  T.rows = nullptr;
  T.run_end = nullptr;
  T.work = nullptr;
  T.search_log = nullptr;
  T.flags_next = J.flags;
  T.cmds = J.slabs;
  T.dict_hash = dt.dict_hash;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  T.dict_size_bits_by_length = dt.dict_size_bits_by_length;
  T.dist_postfix_bits = J.P.dist_postfix_bits;
  T.num_direct_distance_codes = J.P.num_direct_distance_codes;
  T.keys = J.keys;
  T.logs.logs_16 = dt.logs_16;
  T.logs.logs_8 = dt.logs_8;
  static thread_local ChainScratchT<false, false> scratch;
  uint32_t histo[256];
  for (uint32_t place = 0; place < J.n_items; ++place) br_batch_item<false>(J, T, scratch, histo, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

void lz77_batch_gather(const BatchParseJob& J, const uint32_t* offsets, Command* out) {
  for (uint32_t i = 0; i < J.n_items; ++i) {
    const BatchRecord& r = J.records[i];
    if (r.overflow || r.n_cmds > J.items[i].cmd_cap) continue;
    for (uint32_t c = 0; c < r.n_cmds; ++c) out[offsets[i] + c] = br_batch_command(J, J.items[i], r, c);
  }
}

}  // namespace brotli_mi355x
