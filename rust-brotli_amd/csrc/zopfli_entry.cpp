// the introspection entry points of the quality 10 / 11 dictionary search and cost model: see zopfli_entry.inc
#include "zopfli_entry.inc"
