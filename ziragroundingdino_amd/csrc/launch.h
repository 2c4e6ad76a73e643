// launch.h -- what the launchers share on the host.  Per-device launch state: the dynamic-LDS opt-in and the CU count, both
// kept per device (the current one at the call), so a process that drives several devices opts in and sizes its work on each.
// And the one-liners of the argument checks and workspace layouts: align4, misaligned, tiles_of, max_xty_workspace.
#ifndef ZIRA_LAUNCH_H_
#define ZIRA_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <map>
#include <mutex>
#include <utility>

#include "zira_msda.h"

namespace zira {

// n floats rounded up to whole 16-byte units: what follows in a workspace stays 16-byte aligned
inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// p is not a multiple of a (a power of two; 16 bytes: a float4 access).  A null pointer is aligned
inline bool misaligned(const void *p, uintptr_t a = 16) { return ((uintptr_t)p & (a - 1)) != 0; }

// tiles of `rows` rows that M rows fill, the last one perhaps partly
inline int tiles_of(long long M, int rows) { return (int)((M + rows - 1) / rows); }

// floats of zira_xty_f32's scratch that serve each of the products [M, a]^T [M, b] of `shapes` = {{a, b}, ...} in turn
inline size_t max_xty_workspace(long long M, std::initializer_list<std::pair<int, int>> shapes)
{
    size_t n = 0;
    for (const auto &s : shapes) {
        const size_t w = zira_xty_workspace_floats(1, (int)M, s.first, s.second);
        n = w > n ? w : n;
    }
    return n;
}

// Lets `kernel` launch with `bytes` of dynamic LDS on the current device.  48 KB or less needs no opt-in; above that,
// hipFuncSetAttribute is called only when the launch needs more than the largest size opted in before for this (device,
// kernel).  Thread-safe.  Returns the runtime's error, if any; the size is then not recorded.
inline hipError_t lds_opt_in(const void *kernel, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> opted;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = opted[{dev, kernel}];
    if (bytes <= have) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

template <typename F>
inline hipError_t lds_opt_in(F *kernel, size_t bytes)
{
    return lds_opt_in(reinterpret_cast<const void *>(kernel), bytes);
}

// The current device's number of CUs, cached per device (256, an MI355X's, where the runtime gives no answer).
inline int cu_count()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    static std::mutex mu;
    static std::map<int, int> cus;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
    return n;
}

}  // namespace zira

#endif  // ZIRA_LAUNCH_H_
