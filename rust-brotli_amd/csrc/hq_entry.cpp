// the introspection entry points of the quality >= 10 meta-block builder: see hq_entry.inc
#include "hq_entry.inc"
