// lz4_hc_dict_seed.hip -- the seeded rings of the high-compression dictionary
// encoder (lz4_encode_hc_dict.hip), computed on the host by lz4_hc_core.h's own
// host build (the lanes as loops, as in tools/lz4_hc_dict_emul.cpp): one rule
// for what a ring holds, in the kernel, the emulator and here.  Host code only;
// a file of its own because the core is host or device per translation unit.
#include <string.h>

#include "engine.h"

#define LZH_HOST 1
#include "lz4_hc_core.h"

namespace tyche {

size_t lz4_hc_dict_seed_bytes() { return lzh::kTableEntries * sizeof(uint16_t) + lzh::kBuckets; }

// tail: the dictionary's last n = dlen & ~63 bytes; table_out: the rings, then the next-way counters
void lz4_hc_dict_seed_table(const uint8_t *tail, uint32_t n, void *table_out) {
    memset(table_out, 0, lz4_hc_dict_seed_bytes());
    uint16_t *table = (uint16_t *)table_out;
    lzh::seed_window(tail, n, table, (uint8_t *)(table + lzh::kTableEntries));
}

}  // namespace tyche
