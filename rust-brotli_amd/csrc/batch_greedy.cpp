#include "batch_greedy.inc"
