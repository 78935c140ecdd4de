// The split of one AUTO host-buffer batch between the device and the host cores (csrc/hrx_host_split.hpp): the two parts cover the batch exactly, the device part
// never exceeds it, and batches too small to split take one route.  No device: the split is pure arithmetic.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../halo2_regex_amd/csrc/hrx_host_split.hpp"

using hrx::HostSplit;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d (B=%zu f=%g): %s\n", __LINE__, B, f, #c); ++failures; } } while (0)

int main() {
    const size_t batches[] = {1, 2, 32, 63, 64, 65, 127, 128, 129, 191, 192, 1000, 16384, 16385, (size_t)1 << 32};
    const double shares[] = {0.0, 1.0 / 16, 1.0 / 17, 0.5, 15.0 / 16, 0.99, 1.0, 2.0, -1.0, std::numeric_limits<double>::quiet_NaN()};
    for (size_t B : batches) {
        for (double f : shares) {
            HostSplit p{123, 456};
            const bool split = hrx::host_split(B, f, p);
            CHECK(split == (B >= 128));
            if (!split) {
                CHECK(p.device == 0 && p.host == 0);      // nothing recorded: the caller takes one route
                continue;
            }
            CHECK(p.device + p.host == B);
            CHECK(p.device <= B && p.host <= B);
            CHECK(p.device >= 64 && p.host >= 64);
            CHECK(p.device % 64 == 0);
        }
    }
    {   // the shares clamp at 1/16 and 15/16 of the batch (rounded down to the grain)
        size_t B = 16384; double f = 0.0;
        HostSplit p;
        CHECK(hrx::host_split(B, f, p) && p.device == 1024 && p.host == 15360);
        f = 1.0;
        CHECK(hrx::host_split(B, f, p) && p.device == 15360 && p.host == 1024);
        f = 0.5;
        CHECK(hrx::host_split(B, f, p) && p.device == 8192 && p.host == 8192);
        B = 128; f = 1.0;
        CHECK(hrx::host_split(B, f, p) && p.device == 64 && p.host == 64);
        f = 0.0;
        CHECK(hrx::host_split(B, f, p) && p.device == 64 && p.host == 64);
        B = 32; f = 0.5;      // the batch that once made the host part wrap around
        CHECK(!hrx::host_split(B, f, p));
    }
    if (failures) return 1;
    std::printf("host split: ok\n");
    return 0;
}
