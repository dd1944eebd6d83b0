// rstat_core_check -- kmu_rstat_core.h on the host: a stand-alone program (no GPU, no libkmu) that prints the sweeps
// tests/test_cpp_rstat_core.py compares with the numpy model.  Built with -fsanitize=address,undefined and run as a child.
//   base <256 classes> / qual <256 classes>
//   pct L <pct of h = 0 .. L>                       for every L <= 2000
//   bucket sig len bucket lowest highest            for every len <= 4200 and around every power of two up to 2^62
//   bucketsum sig <sum of bucket(len), len <= 2^21>
//   layout max_len sig n_buckets limit
//   median <class> for a few rows of counts
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_rstat_core.h"

using namespace kmu;

static void bucket_line(int sig, uint64_t len) {
    const uint32_t sub = rs_sub_bits(sig);
    const uint64_t b = rs_len_bucket(len, sub);
    uint64_t lo, hi;
    rs_bucket_range(b, sub, lo, hi);
    std::printf("bucket %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", sig, len, b, lo, hi);
}

int main() {
    std::printf("base");
    for (uint32_t b = 0; b < 256; b++) std::printf(" %u", rs_base_class(b));
    std::printf("\nqual");
    for (uint32_t b = 0; b < 256; b++) std::printf(" %u", rs_qual_class(b));
    std::printf("\n");
    for (uint64_t len = 0; len <= 2000; len++) {
        std::printf("pct %" PRIu64, len);
        for (uint64_t h = 0; h <= len; h++) std::printf(" %u", rs_pct(h, len));
        std::printf("\n");
    }
    std::printf("pct_long %u %u\n", rs_pct(((uint64_t) 1 << 40) / 3, (uint64_t) 1 << 40), rs_pct((uint64_t) 1 << 50, (uint64_t) 1 << 50));
    for (int sig = 0; sig <= 6; sig++) std::printf("sub_bits %d %u\n", sig, rs_sub_bits(sig));
    for (int sig = 1; sig <= 5; sig++) {
        for (uint64_t len = 0; len <= 4200; len++) bucket_line(sig, len);
        for (int k = 12; k <= 62; k++)
            for (int d = -1; d <= 1; d++) bucket_line(sig, ((uint64_t) 1 << k) + (uint64_t) (int64_t) d);
        uint64_t sum = 0;
        const uint32_t sub = rs_sub_bits(sig);
        for (uint64_t len = 0; len <= ((uint64_t) 1 << 21); len++) sum += rs_len_bucket(len, sub);
        std::printf("bucketsum %d %" PRIu64 "\n", sig, sum);
    }
    const uint64_t max_lens[] = {1, 31, 32, 63, 64, 5000, 1000000, (uint64_t) 1 << 40};
    for (int sig = 1; sig <= 5; sig++)
        for (uint64_t max_len : max_lens) {
            uint32_t n_buckets;
            uint64_t limit;
            rs_len_layout(max_len, rs_sub_bits(sig), n_buckets, limit);
            std::printf("layout %" PRIu64 " %d %u %" PRIu64 "\n", max_len, sig, n_buckets, limit);
        }
    const std::vector<std::vector<uint64_t>> rows = {{0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0}, {2, 0, 0, 2, 0, 0, 0, 0},
                                                     {1, 0, 0, 2, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 9}, {3, 1, 1, 1, 1, 1, 1, 2}};
    for (const auto &r : rows) {
        uint64_t len = 0;
        for (uint64_t v : r) len += v;
        std::printf("median %u\n", rs_median_class(r.data(), len));
    }
    return 0;
}
