// batch_zopfli_emu.inc -- host emulation of the batch seam of quality 11 (batch_zopfli.h: lz77_zopfli_batch_parse),
// compiled into the emulation build only (BROTLI_HOST_EMU, tests/emu; batch_greedy.inc includes it there): the same item code
// (batch_zopfli_device.h) on plain memory, one item after the other in the order of the plan, the tables taken in turn -- so that
// a table serves several items, as on the device.  The gather is lz77_batch_gather (batch_greedy_emu.inc).
#include <stdexcept>

#include "batch_zopfli_device.h"
#include "device_api.h"

namespace brotli_mi355x {

namespace {
void zopfli_batch_emu(const ZopfliBatchJob& J, int dict) {
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
    if (dict == kZBatchSharedDict)
      br_zopfli_batch_item<kZBatchSharedDict>(J, T, histo, ZFast(), J.order[place], place % J.tables);
    else if (dict == kZBatchItemDicts)
      br_zopfli_batch_item<kZBatchItemDicts>(J, T, histo, ZFast(), J.order[place], place % J.tables);
    else
      br_zopfli_batch_item(J, T, histo, ZFast(), J.order[place], place % J.tables);
  }
  *J.counter = J.n_items;
}
}  // namespace

void lz77_zopfli_batch_parse(const ZopfliBatchJob& J) { zopfli_batch_emu(J, kZBatchNoDict); }

// (the scalar build of br_zopfli_batch_prepend runs the 64 key classes of the wave-wide partition one after the other)
void lz77_zopfli_batch_parse_dicts(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && J.item_dict_bytes == nullptr) throw std::runtime_error("brotli_mi355x: a dictionary batch group without its dictionary sizes");
  zopfli_batch_emu(J, kZBatchItemDicts);
}

void lz77_zopfli_batch_parse_dict(const ZopfliBatchJob& J) {
  if (J.n_items != 0 && (J.image_buckets == nullptr || J.image_forest == nullptr || J.dict_bytes < 2))
    throw std::runtime_error("brotli_mi355x: a shared-dictionary batch group without its tree image");
  zopfli_batch_emu(J, kZBatchSharedDict);
}

// the three launches of the product's build, element by element: the fill, the class of every stored position, and the store
// launch class by class -- lane by lane -- each class walking its positions through the same scan of the class entries
void lz77_zopfli_dict_image(const uint8_t* dict, uint32_t D, uint32_t lgwin, uint16_t* classes, uint32_t* buckets, uint32_t* forest) {
  if (lgwin < 10 || lgwin > 24 || D > (1u << lgwin) - 16u) throw std::runtime_error("brotli_mi355x: a dictionary the Zopfli tree image does not take");
  const uint32_t end = zopfli_dict_image_stored(D), entries = zopfli_dict_image_class_entries(D);
  br_zopfli_image_fill(buckets, forest, lgwin, zopfli_dict_image_slots(D, lgwin), 0, 1);
  if (end == 0) return;
  for (uint32_t i = 0; i < entries; ++i) br_zopfli_image_class_entry(dict, end, classes, i);
  const ZopfliParams Z = br_zopfli_image_params(lgwin, D);
  ZopfliBuffers B{};
  B.buckets = buckets;
  B.forest = forest;
  const ZH10 h = z_hasher_of(Z, B);
  for (uint32_t cls = 0; cls < kZImageClasses; ++cls) br_zopfli_image_store_class(h, Z, dict, classes, end, cls);
}

}  // namespace brotli_mi355x
