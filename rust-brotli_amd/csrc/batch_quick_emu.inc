// batch_quick_emu.inc -- host emulation of the batch seam of qualities 2 .. 4 (batch_quick.h: lz77_quick_batch_parse), compiled
// into the emulation build only (BROTLI_HOST_EMU, tests/emu; batch_greedy.inc includes it there): the same item code
// (batch_quick_device.h) on plain memory, one item after the other in the order of the plan, the tables taken in turn -- so that
// a table serves several items, as on the device.  The gather is lz77_batch_gather (batch_greedy_emu.inc).
// lz77_quick_batch_parse_dict: the same loop over the item code behind a shared custom dictionary (the image is the emulation's
// lz77_quick_init + lz77_quick_prepend, i.e. br_quick_prepend).
// lz77_quick_batch_parse_dicts: the same loop behind a dictionary per item; a chain files its dictionary with br_quick_prepend, or
// copies the image lz77_quick_dict_images (br_quick_prepend per image) has made of it.
// lz77_quick_batch_parse_long: the same loop over the item code of the items of several blocks; its gather is lz77_batch_gather_long.
#include <stdexcept>

#include "batch_quick_device.h"
#include "device_api.h"

namespace brotli_mi355x {

// what every entry below starts with: the group has a table, and the tables of the static dictionary and of should_compress
static void quick_batch_emu_tables(const QuickBatchJob& J, QuickTables& T, EntropyTables& logs) {
  if (J.tables == 0) throw std::runtime_error("brotli_mi355x: a batch group without a table");
  const DeviceTables& dt = dev_tables();
  T.dict_hash = dt.dict_hash;
  T.dict_data = dt.dict_data;
  T.dict_offsets_by_length = dt.dict_offsets_by_length;
  logs.logs_16 = dt.logs_16;
  logs.logs_8 = dt.logs_8;
}

void lz77_quick_batch_parse(const QuickBatchJob& J) {
  if (J.n_items == 0) return;
  QuickTables T;
  EntropyTables logs;
  quick_batch_emu_tables(J, T, logs);
  uint32_t histo[256];
  SegExit exit_slot;
  for (uint32_t place = 0; place < J.n_items; ++place) br_quick_batch_item(J, T, logs, histo, &exit_slot, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

void lz77_quick_batch_parse_dict(const QuickBatchJob& J) {
  if (J.n_items == 0) return;
  QuickTables T;
  EntropyTables logs;
  quick_batch_emu_tables(J, T, logs);
  if (J.dict_bytes == 0 || J.image == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its table image");
  uint32_t histo[256];
  SegExit exit_slot;
  for (uint32_t place = 0; place < J.n_items; ++place) br_quick_batch_item<true>(J, T, logs, histo, &exit_slot, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

void lz77_quick_batch_parse_dicts(const QuickBatchJob& J) {
  if (J.n_items == 0) return;
  QuickTables T;
  EntropyTables logs;
  quick_batch_emu_tables(J, T, logs);
  if (J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a batch group with a dictionary per item without their sizes");
  uint32_t histo[256];
  SegExit exit_slot;
  for (uint32_t place = 0; place < J.n_items; ++place) br_quick_batch_item<true, true>(J, T, logs, histo, &exit_slot, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

// the table images of a group: br_quick_prepend per image, on the zeroed table the caller hands over
void lz77_quick_dict_images(const QuickJob& Q, const uint8_t* text, uint32_t n_images, const uint32_t* text_at, const uint32_t* dict_bytes,
                            uint32_t* images) {
  for (uint32_t j = 0; j < n_images; ++j) {
    QuickJob image = Q;
    image.table = images + (size_t)j * quick_table_words(Q);
    br_quick_prepend(image, text + text_at[j], dict_bytes[j]);
  }
}

void lz77_quick_batch_parse_long(const QuickBatchJob& J, BatchLongRecord* records) {
  if (J.n_items == 0) return;
  QuickTables T;
  EntropyTables logs;
  quick_batch_emu_tables(J, T, logs);
  uint32_t histo[256];
  SegExit exit_slot;
  for (uint32_t place = 0; place < J.n_items; ++place) br_quick_batch_item_long(J, records, T, logs, histo, &exit_slot, J.order[place], place % J.tables);
  *J.counter = J.n_items;
}

}  // namespace brotli_mi355x
