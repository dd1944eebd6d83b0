// sim_gather.h -- gather_tiles of kmerutils_amd/csrc/kmu_gather.h over 64 simulated lanes in lockstep, built from the functions of
// kmu_gather_core.h alone: the 64-ary search for a tile's first item with the ballot as a loop, windows of 64 ends, the skip of 64
// empty items, the limit, gather_window_count per lane and the advance.  sim_pile_segments.cpp (k_ext_copy) and sim_unitigs.cpp
// (k_ut_seq_copy) replay their copies with it.  Checked on the way: the first item of every tile equals the single-lane upper index
// and brackets the tile's first byte; no trip is empty and the walk ends; the window never advances past the position; the window
// count equals plain counting and is at most 63; every output byte is delivered exactly once, to an item that holds it.
#pragma once

#include <algorithm>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_gather_core.h"

// ends: n_items + 1 ascending entries, ends[0] = 0.  byte(r, o) is the kernel's callback; fail(what) must not return
template <class Fail, class Byte> inline void gather_replay(const std::vector<uint64_t> &ends, Fail fail, Byte byte) {
    using namespace kmu;
    const uint64_t n_items = ends.size() - 1u, total = ends[n_items], n_tiles = (total + GATHER_TILE - 1u) / GATHER_TILE;
    std::vector<uint32_t> hits(total, 0u);
    for (uint64_t t = 0; t < n_tiles; t++) {
        uint64_t pos = t * GATHER_TILE;
        const uint64_t tile_end = std::min<uint64_t>(pos + GATHER_TILE, total);
        uint64_t r0 = gather_find_64ary(n_items, [&](uint64_t lo, uint64_t step, uint64_t hi) { // the ballot over 64 lanes
            uint32_t n = 0;
            for (uint64_t lane = 0; lane < 64; lane++) n += lo + (lane + 1u) * step < hi && ends[lo + (lane + 1u) * step] <= pos;
            return n;
        });
        if (r0 != gather_upper_index(ends.data(), n_items, pos)) fail("the wave's search differs from one lane's");
        if (ends[r0] > pos || (r0 < n_items && ends[r0 + 1u] <= pos)) fail("the first item of a tile");
        uint32_t guard = 0;
        while (pos < tile_end) {
            if (++guard > 100000u) fail("the walk does not advance");
            uint64_t win[64];
            for (uint32_t lane = 0; lane < 64; lane++) win[lane] = r0 + 1u + lane <= n_items ? ends[r0 + 1u + lane] : ~0ull;
            if (win[63] <= pos) {
                r0 += 64u;
                continue;
            }
            uint64_t limit = std::min<uint64_t>(pos + 64u, tile_end);
            limit = std::min(limit, win[63]);
            if (limit <= pos) fail("an empty trip");
            uint32_t advance = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint64_t o = pos + lane;
                advance += win[lane] <= limit;
                if (o >= limit) continue;
                const uint32_t c = gather_window_count([&](uint32_t j) { return win[j]; }, o);
                uint32_t slow = 0;
                for (uint32_t j = 0; j < 64; j++) slow += win[j] <= o;
                if (c != slow || c > 63u) fail("gather_window_count differs from counting");
                const uint64_t r = r0 + c;
                if (r >= n_items || ends[r] > o || ends[r + 1u] <= o) fail("a byte's item does not hold it");
                hits[o]++;
                byte(r, o);
            }
            r0 += advance;
            if (r0 > n_items || ends[r0] > limit) fail("the window advanced past the position");
            pos = limit;
        }
    }
    for (uint64_t o = 0; o < total; o++)
        if (hits[o] != 1u) fail("an output byte delivered not exactly once");
}
