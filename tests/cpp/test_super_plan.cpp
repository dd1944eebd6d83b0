// The launch plan of k_sketch_super (kmerutils_amd/csrc/kmu_sketch_host.hpp: SuperPlan, super_plan), host side: the plan at every
// sketch size where it changes, pinned number by number, and what must hold at every size the launcher accepts.
// A program of its own: hipcc, host code only (the header sits on HIP's), no device needed:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g tests/cpp/test_super_plan.cpp -o test_super_plan && ./test_super_plan
#include <cstdio>
#include <cstdlib>

#include "../../kmerutils_amd/csrc/kmu_sketch_host.hpp"

using namespace kmu;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

static const uint32_t CHUNK = 512;          // what launch_super stages per chunk
static const size_t LDS_MAX = 160 * 1024;   // what launch_super asks of a gfx950 workgroup

// one row of the table: lds == 0 leaves the byte count to the general checks below
static void pin(int m, int wide, int threads, int ncol, size_t lds, int blocks_per_cu) {
    const SuperPlan sp = super_plan(m, CHUNK, LDS_MAX);
    const bool ok = sp.wide == wide && sp.threads == threads && sp.ncol == ncol && (lds == 0 || sp.lds == lds) && sp.blocks_per_cu == blocks_per_cu;
    if (!ok) {
        std::printf("FAILED m = %d: wide %d threads %d ncol %d lds %zu blocks/CU %d, expected %d %d %d %zu %d\n", m, sp.wide, sp.threads, sp.ncol,
                    sp.lds, sp.blocks_per_cu, wide, threads, ncol, lds, blocks_per_cu);
        failures++;
    }
}

int main() {
    //  m   entry  threads ncol  lds  blocks/CU
    pin(2, 0, 256, 256, 4656, 8);
    pin(3, 0, 256, 256, 4928, 8);
    pin(64, 0, 256, 256, 21520, 7);
    pin(225, 0, 256, 256, 65312, 2);   // the last size under 64 KiB: no attribute call
    pin(226, 0, 256, 256, 65584, 2);   // the first one over
    pin(256, 0, 256, 256, 73744, 2);
    pin(257, 1, 256, 256, 139808, 1);  // two-byte entries
    pin(302, 1, 256, 256, 163568, 1);
    pin(303, 1, 192, 192, 125312, 1);
    pin(399, 1, 192, 192, 163712, 1);
    pin(400, 1, 128, 128, 112912, 1);
    pin(587, 1, 128, 128, 163776, 1);
    pin(588, 1, 64, 64, 88784, 1);
    pin(1109, 1, 64, 64, 163808, 1);
    pin(1110, 1, 64, 63, 0, 1);        // one wave, fewer item lanes than lanes
    pin(2500, 1, 64, 23, 0, 1);
    pin(8872, 1, 64, 1, 0, 1);
    CHECK(super_plan(8873, CHUNK, LDS_MAX).ncol == 0); // refused
    CHECK(super_plan(65536, CHUNK, LDS_MAX).ncol == 0);
    CHECK(super_plan(1110, CHUNK, LDS_MAX).lds <= LDS_MAX);
    // 64 KiB is the limit without the attribute call: 225 and 226 sit on either side of it
    CHECK(super_plan(225, CHUNK, LDS_MAX).lds <= 64 * 1024 && super_plan(226, CHUNK, LDS_MAX).lds > 64 * 1024);

    int last_ncol = 256, last_threads = 256;
    for (int m = 2; m <= 8872; m++) {
        const SuperPlan sp = super_plan(m, CHUNK, LDS_MAX);
        CHECK(sp.wide == (m > 256 ? 1 : 0));
        CHECK(sp.lds <= LDS_MAX && sp.lds % 16 == 0);
        CHECK(sp.threads == 256 || sp.threads == 192 || sp.threads == 128 || sp.threads == 64);
        CHECK(1 <= sp.ncol && sp.ncol <= sp.threads);
        CHECK(sp.ncol == sp.threads || sp.threads == 64);
        // what the kernel carves out: slot minima, staged seeds, index bounds, two words of 8 bytes, the permutation columns
        const size_t carved = (size_t) 16 * m + (size_t) 8 * CHUNK + 16 + (sp.wide ? 2 : 1) * (size_t) m * sp.ncol;
        CHECK(carved <= sp.lds);
        CHECK(sp.lds < carved + 48); // and no more than rounding asks for
        CHECK(sp.blocks_per_cu >= 1 && (size_t) sp.blocks_per_cu * sp.lds <= LDS_MAX && sp.blocks_per_cu * sp.threads <= 2048);
        // a larger sketch never gets more item lanes or threads; within the u8 or the u16 range the plan only shrinks
        if (m != 257) CHECK(sp.ncol <= last_ncol && sp.threads <= last_threads);
        // one more item lane would not fit (the plan leaves no usable column unused)
        if (sp.threads == 64 && sp.ncol < 64) CHECK(carved + (size_t) 2 * m + 16 > LDS_MAX);
        last_ncol = sp.ncol;
        last_threads = sp.threads;
        if (failures > 20) break;
    }
    for (int m = 8873; m <= 65536; m++) CHECK(super_plan(m, CHUNK, LDS_MAX).ncol == 0);
    if (failures) return 1;
    std::printf("test_super_plan ok\n");
    return 0;
}
