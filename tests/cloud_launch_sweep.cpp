// cloud_launch_sweep.cpp -- every launch of the cloud path (csrc/cloud_common.h's kCloudLaunches) at the ends of the
// domain its ABI headers declare, as a stand-alone host program: tests/test_cloud_limits_host.py builds it with the host
// compiler and the address and undefined-behaviour sanitizers and runs the binary.  For every launch and size it asks the
// library's own cloud_blocks and cloud_trips and checks two things: HIP launches the grid (blocks * threads < 2^32), and
// the grid covers the work (blocks * items per block * trips >= work).  It holds no copy of the library's rule; what it
// checks is the table of launches, not the launch sites, which the GPU cases of tests/cloud_limits_check.py run.
//   cloud_launch_sweep             the library's counts; exit status 0 iff nothing is bad
//   cloud_launch_sweep --uncapped  a demonstration that the check can fail: the counts from before there was a cap,
//                                  ceil(work / items per block) in one trip, restated here because no function of the
//                                  library computes them any more; what HIP refuses of those is listed, one
//                                  "REFUSED <launch>" line per launch, exit status 1
#define MVS_CLOUD_GEOMETRY_ONLY
#include "cloud_common.h"

#include <cstdio>
#include <cstring>

using namespace mvs;

int main(int argc, char** argv) {
    const bool uncapped = argc > 1 && !std::strcmp(argv[1], "--uncapped");
    const long long kRows[] = {1, 31, 32, 33, 536870880, 536870881, (1LL << 28) - 1, 1LL << 28, (1LL << 31) - 1};
    const long long kCells[] = {1, 1024, 1025, (1LL << 31) - 1};
    const int kFuse[][3] = {{1, 1, 1}, {(1 << 24) - 1, 1, 1}, {1 << 24, 1, 1}, {2147483647, 1, 1}, {2185, 512, 640}};
    long n_checked = 0, n_bad = 0;
    for (const CloudLaunch& L : kCloudLaunches) {
        long long sizes[16];
        int n = 0;
        if (L.work == kWorkRows) for (const long long v : kRows) sizes[n++] = v;
        if (L.work == kWorkCells) for (const long long v : kCells) sizes[n++] = v;
        if (L.work == kWorkFuseTiles) for (const auto& f : kFuse) sizes[n++] = cloud_fuse_tiles(f[0], f[1], f[2]);
        bool refused = false;
        for (int k = 0; k < n; ++k) {
            const long long work = sizes[k];
            const long long blocks = uncapped ? (work + L.per_block - 1) / L.per_block : cloud_blocks(L, work);
            const long long trips = uncapped ? 1 : cloud_trips(L, work);
            const bool launches = blocks >= 1 && blocks * L.threads < (1LL << 32);
            // blocks <= 2^31, items per block <= 2^10, trips <= 2^31 / blocks + 1: the product stays below 2^63
            const bool covers = blocks * L.per_block * trips >= work;
            // a kernel without a loop must not need one
            const bool one_trip = L.loops || trips == 1;
            ++n_checked;
            if (!launches || !covers || !one_trip) {
                ++n_bad;
                refused = refused || !launches;
                std::printf("BAD %s: work %lld -> %lld blocks of %d threads, %d items per block, %lld trips%s%s%s\n", L.kernels,
                            work, blocks, L.threads, L.per_block, trips, launches ? "" : " [2^32 threads or more]",
                            covers ? "" : " [work left over]", one_trip ? "" : " [no loop in this kernel]");
            }
        }
        if (refused) std::printf("REFUSED %s\n", L.kernels);
    }
    std::printf("cloud_launch_sweep: %ld launches, %ld bad\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
