// hrx_host_split.hpp — how hrx_witness_batch_host (hrx_host_api.cpp) divides one AUTO batch between the device and the host cores when it takes both at once.
// Pure arithmetic on the batch size and the device's share, kept apart from the route so that it can be checked on a host without a device
// (tests/host_cpp/test_host_split.cpp).
#pragma once
#include <algorithm>
#include <cstddef>

namespace hrx {

constexpr size_t kSplitGrain = 64;                        // the device part is a multiple of this many strings (one group of the one-wave kernel) ...
constexpr size_t kSplitMinStrings = 2 * kSplitGrain;      // ... and a batch of fewer strings than two grains is not split: one way takes it whole
constexpr double kSplitMinShare = 1.0 / 16, kSplitMaxShare = 15.0 / 16;   // the device's share of a split, clamped

struct HostSplit {
    size_t device = 0;      // strings [0, device) through the device
    size_t host = 0;        // strings [device, device + host) on the host cores; device + host == B
};

// f_dev: the device's share of the batch (from the two parts' rates; clamped to [kSplitMinShare, kSplitMaxShare]).  Returns false when B is too small to split:
// the caller takes one route for the whole batch and records no split figures.  When it returns true, both parts are at least one grain and device is a
// multiple of kSplitGrain.
inline bool host_split(size_t B, double f_dev, HostSplit &out) {
    out = HostSplit{};
    if (B < kSplitMinStrings) return false;
    if (!(f_dev >= kSplitMinShare)) f_dev = kSplitMinShare;      // (NaN included)
    if (f_dev > kSplitMaxShare) f_dev = kSplitMaxShare;
    size_t dev = (size_t)((double)B * f_dev) / kSplitGrain * kSplitGrain;
    dev = std::max(kSplitGrain, std::min(dev, (B - kSplitGrain) / kSplitGrain * kSplitGrain));
    out.device = dev;
    out.host = B - dev;
    return true;
}

}  // namespace hrx
