// tools/page_order_emul.cpp -- host emulator of the page order of the
// lane-per-page launches (tyche_amd/csrc/page_order_core.h): the bin of a stream
// length, the windowed stable order that page_order.hip computes on the device,
// and the slot map the decoder walks.  TEST INFRASTRUCTURE:
// tests/test_page_order_emul.py checks the rule on the CPU, and
// tests/test_gpu_lz4_order.py holds the device's order array to this one.
//
//   g++ -O2 -shared -fPIC -o tools/bin/libpageorderemul.so tools/page_order_emul.cpp
#include <cstddef>
#include <cstdint>
#include <vector>

#define PO_HOST 1
#include "../tyche_amd/csrc/page_order_core.h"

extern "C" {

void page_order_emul_constants(uint32_t *k3) {
    k3[0] = po::kBins;
    k3[1] = po::kTile;
    k3[2] = po::kLanes;
}

uint32_t page_order_emul_bin(uint32_t length, uint32_t in_cap) { return po::bin_of(length, in_cap, po::bin_shift(in_cap)); }

// order[0 .. count): the counting sort, tile by tile as the device runs it (histograms, the scan
// with keys outside and tiles inside, the scatter in page order).  0, or 1 for a count it refuses.
int page_order_emul(const uint32_t *lengths, uint64_t count, uint32_t in_cap, uint32_t window, uint32_t *order) {
    if (count == 0 || count > 0x7FFFFFFFu || !po::geometry_ok((uint32_t)count, window)) return 1;
    const po::Geo g = po::geometry((uint32_t)count, window);
    const uint32_t shift = po::bin_shift(in_cap);
    std::vector<uint32_t> hist((size_t)g.ntiles * po::kBins, 0u), base((size_t)g.nwin * po::kBins, 0u);
    for (uint32_t t = 0; t < g.ntiles; t++) {
        uint32_t first, end;
        po::tile_bounds(g, t, &first, &end);
        for (uint32_t i = first; i < end; i++) hist[(size_t)t * po::kBins + po::rank_key(lengths[i], in_cap, shift)]++;
    }
    for (uint32_t w = 0; w < g.nwin; w++) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < po::kBins; k++) {
            uint32_t run = 0;
            for (uint32_t j = 0; j < g.tpw; j++) {
                uint32_t &h = hist[((size_t)w * g.tpw + j) * po::kBins + k];
                const uint32_t v = h;
                h = run;
                run += v;
            }
            base[(size_t)w * po::kBins + k] = total;
            total += run;
        }
    }
    for (uint32_t t = 0; t < g.ntiles; t++) {
        uint32_t first, end;
        po::tile_bounds(g, t, &first, &end);
        const uint32_t w = t / g.tpw;
        for (uint32_t i = first; i < end; i++) {
            const uint32_t k = po::rank_key(lengths[i], in_cap, shift);
            const uint32_t pos = po::window_first(g, w) + base[(size_t)w * po::kBins + k] + hist[(size_t)t * po::kBins + k]++;
            if (pos >= count) return 2;
            order[pos] = i;
        }
    }
    return 0;
}

// slots[(k * grid + wave) * 64 + lane] for every generation k < gens: po::slot, `count` where the lane has none
uint64_t page_order_emul_generations(uint32_t grid, uint64_t count) { return po::generations(grid, count); }
void page_order_emul_slots(uint32_t grid, uint64_t count, uint64_t gens, uint64_t *slots) {
    for (uint64_t k = 0; k < gens; k++)
        for (uint32_t w = 0; w < grid; w++)
            for (uint32_t l = 0; l < po::kLanes; l++) slots[(k * grid + w) * po::kLanes + l] = po::slot(k, w, l, grid, count);
}

}  // extern "C"
