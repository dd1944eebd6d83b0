// The sub-list rule of k_multiset_long (kmerutils_amd/csrc/kmu_sketch_host.hpp: PMH_LONG_TP, pmh_long_parts, pmh_long_part_of), host side.
// A program of its own: hipcc, host code only (the header sits on HIP's), no device needed:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/cpp/test_long_parts.cpp -o test_long_parts && ./test_long_parts
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_sketch_host.hpp"
#include "../../kmerutils_amd/csrc/kmu_sketch_kernels.h"

using namespace kmu;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

int main() {
    const uint32_t T = PMH_LONG_TP;
    CHECK(T == 16384u);
    // P at the edges
    CHECK(pmh_long_parts(1) == 1u);
    CHECK(pmh_long_parts(T) == 1u);
    CHECK(pmh_long_parts(T + 1) == 2u);
    CHECK(pmh_long_parts(2 * T) == 2u);
    CHECK(pmh_long_parts(2 * T + 1) == 3u);
    CHECK(pmh_long_parts(UQ_KREG * 1024u + 1u) == 2u); // the first read beyond the second uq shape
    // the largest read the per-sequence route keeps, and the largest the kernel keeps
    CHECK(pmh_long_parts(LONG_SEQ_KMERS) == 16u);
    CHECK(pmh_long_parts(LONG_SEQ_KMERS + 1) == 17u);
    CHECK(pmh_long_parts(LONG_SEQ_KMERS) <= DEF_PARTS);
    CHECK(pmh_long_parts(DEF_PARTS * T) == DEF_PARTS);
    CHECK(pmh_long_parts(DEF_PARTS * T + 1) == DEF_PARTS + 1);
    CHECK(pmh_long_parts(0xFFFFFFFFu) == 0xFFFFFFFFu / T + 1u); // (no overflow at the top of the range)
    // an expected sub-list lies well inside a workgroup's registers and a scratch segment
    CHECK(T < UQ_KREG * 1024u && UQ_KREG * 1024u + UQ2_COLL + UQ2_COLL / 2 <= DEF_SEG);
    // the sub-list of a key: always in range, equal keys together (a function of the key), and even over keys that share lo ^ hi
    // (k_multiset_uq's bitmap index and its collision sort's bucket are functions of lo ^ hi)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (uint32_t P = 1; P <= DEF_PARTS; P++) {
        std::vector<uint32_t> hist(P, 0), hist_x(P, 0);
        const uint32_t n = 20000;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t key = next();
            const uint32_t p = pmh_long_part_of(key, P);
            CHECK(p < P);
            CHECK(p == pmh_long_part_of(key, P));
            hist[p]++;
            const uint32_t lo = (uint32_t) next(); // keys with lo ^ hi == 0x12345678
            const uint32_t px = pmh_long_part_of(((uint64_t) (lo ^ 0x12345678u) << 32) | lo, P);
            CHECK(px < P);
            hist_x[px]++;
        }
        for (uint32_t p = 0; p < P; p++) { // within 6 sigma of n / P (binomial)
            const double e = (double) n / P, sd = std::sqrt(e * (1.0 - 1.0 / P)) + 1.0;
            CHECK(std::fabs(hist[p] - e) <= 6.0 * sd);
            CHECK(std::fabs(hist_x[p] - e) <= 6.0 * sd);
        }
    }
    CHECK(pmh_long_part_of(0, 7) == 0u && pmh_long_part_of(~0ull, 1) == 0u);
    if (failures) return 1;
    std::printf("test_long_parts ok\n");
    return 0;
}
