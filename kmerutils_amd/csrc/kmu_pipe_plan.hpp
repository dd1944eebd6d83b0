// kmu_pipe_plan.hpp -- the chunk plan of kmu_sketch_count's host pipeline (kmu_sketch_pipe.hip): pure host arithmetic, no HIP
// header, so that the host-only sanitizer program (tests/cpp/test_host_san.cpp) compiles it with g++ alone.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace kmu {

// The chunks of a call over n_seq whole reads of `total` bases, h_off[0 .. n_seq] their offsets re-based to 0.
//  cut        chunk c is reads [cut[c], cut[c + 1])
//  pk_bounds  packed uploads only (packed_up and at least one chunk), else empty: the packed form of chunk c is the stream
//             [pk_bounds[c], pk_bounds[c + 1])
// Chunk sizes: the first one is an eighth of chunk_bytes.  growth > 1: each chunk is `growth` times its predecessor; growth 1:
// equal chunks of about chunk_bytes after the first.  (Why: the comment in kmu_sketch_count.)
inline void pipe_chunk_plan(const std::vector<uint64_t> &h_off, uint32_t n_seq, uint64_t total, uint64_t chunk_bytes, uint64_t growth,
                            bool packed_up, std::vector<uint32_t> *cut_out, std::vector<uint64_t> *pk_bounds) {
    std::vector<uint32_t> &cut = *cut_out;
    cut.assign(1, 0u);
    std::vector<uint64_t> plan; // chunk sizes, in order (a chunk ends at the first read boundary at or behind its target)
    if (growth > 1) {
        uint64_t sz = std::min<uint64_t>(std::max<uint64_t>(chunk_bytes / 8, 1), total), left = total;
        while (left) {
            const uint64_t take = left <= sz + sz / 2 ? left : sz; // (a remainder of up to half a chunk more rides with the last one)
            plan.push_back(take);
            left -= take;
            sz *= growth;
        }
    } else {
        const uint64_t first = std::min<uint64_t>(std::max<uint64_t>(chunk_bytes / 8, 1), total);
        plan.push_back(first);
        const uint64_t body = total - first;
        const uint64_t n_body = std::max<uint64_t>(1, (body + chunk_bytes / 2) / chunk_bytes);
        for (uint64_t i = 0; i < n_body && body; i++) plan.push_back(body / n_body + 1);
    }
    {
        uint64_t target = 0;
        uint32_t r = 0;
        for (size_t i = 0; i < plan.size() && r < n_seq; i++) {
            target += plan[i];
            uint32_t e = i + 1 == plan.size() ? n_seq : (uint32_t) (std::lower_bound(h_off.begin() + r + 1, h_off.end(), target) - h_off.begin());
            if (e > n_seq) e = n_seq;
            if (e <= r) continue; // (a read that spans several targets: one chunk)
            cut.push_back(e);
            r = e;
        }
        if (r < n_seq) cut.push_back(n_seq);
    }
    const size_t n_chunks = cut.size() - 1;
    // The packed form of chunk c is the stream from the end of chunk c - 1 rounded up to 16 bases to its own end rounded up
    // likewise (the few bases of its first read before that came with the chunk before).
    pk_bounds->clear();
    if (packed_up && n_chunks > 0) {
        pk_bounds->push_back(0);
        for (size_t c = 0; c < n_chunks; c++) {
            const uint64_t e = c + 1 == n_chunks ? total : std::min<uint64_t>(total, (h_off[cut[c + 1]] + 15) & ~15ull);
            pk_bounds->push_back(std::max(e, pk_bounds->back()));
        }
    }
}

} // namespace kmu
