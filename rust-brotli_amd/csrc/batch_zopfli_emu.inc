// batch_zopfli_emu.inc -- host emulation of the batch seam of quality 11 (batch_zopfli.h: lz77_zopfli_batch_parse),
// compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu; batch_greedy.inc includes it there): the same item code
// (batch_zopfli_device.h) on plain memory, one item after the other in the order of the plan, the tables taken in turn -- so that
// a table serves several items, as on the device.  The gather is lz77_batch_gather (batch_greedy_emu.inc).
#include <stdexcept>

#include "batch_zopfli_device.h"
#include "device_api.h"

namespace brotli_mi355x {

namespace {
void zopfli_batch_emu(const ZopfliBatchJob& J, bool dicts) {
  if (J.n_items == 0) return;
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  const DeviceTables& dt = dev_tables();
  ZopfliTables T;
  T.lut_buckets = dt.dict_lut_buckets;
  T.lut_words = dt.dict_lut_words;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  T.dict_size_bits_by_length = dt.dict_size_bits_by_length;
  T.logs.logs_16 = dt.logs_16;
  T.logs.logs_8 = dt.logs_8;
  uint32_t histo[256];
  for (uint32_t place = 0; place < J.n_items; ++place) {
    if (dicts)
      br_zopfli_batch_item<true>(J, T, histo, ZFast(), J.order[place], place % J.tables);
    else
      br_zopfli_batch_item(J, T, histo, ZFast(), J.order[place], place % J.tables);
  }
  *J.counter = J.n_items;
}
}  // namespace

void lz77_zopfli_batch_parse(const ZopfliBatchJob& J) { zopfli_batch_emu(J, false); }

// (the scalar build of br_zopfli_batch_prepend runs the 64 key classes of the wave-wide partition one after the other)
void lz77_zopfli_batch_parse_dicts(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its dictionary sizes");
  zopfli_batch_emu(J, true);
}

}  // namespace brotli_mi355x
