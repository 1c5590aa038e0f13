/*
 * ddc_host.h -- host plumbing shared by the library's translation units: the error macro, the device check, the
 * arithmetic every windowed object repeats, and the one way a launcher raises a kernel's dynamic LDS cap.  Internal
 * (not part of the public ABI, that is include/perseus_ddc.h); nothing here is exported.
 */
#ifndef PDDC_DDC_HOST_H
#define PDDC_DDC_HOST_H

#include "../../include/perseus_ddc.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

/* sets pddc_last_error() of this thread and returns `code` (ddc_pipeline.cpp) */
extern "C" __attribute__((visibility("hidden"))) int pddc_set_error_(int code, const char *fmt, ...);
/* PDDC_OK, or PDDC_ENODEV with its message: no device at all / `device` is not one of them (ddc_pipeline.cpp) */
extern "C" __attribute__((visibility("hidden"))) int pddc_check_device_(int device);

#define PDDC_HIP_TRY(expr)                                                                                      \
    do {                                                                                                        \
        hipError_t e__ = (expr);                                                                                \
        if (e__ != hipSuccess)                                                                                  \
            return pddc_set_error_(e__ == hipErrorOutOfMemory ? PDDC_ENOMEM                                     \
                                   : (e__ == hipErrorNoDevice || e__ == hipErrorInvalidDevice) ? PDDC_ENODEV    \
                                                                                               : PDDC_EHIP,     \
                                   "%s: %s", #expr, hipGetErrorString(e__));                                    \
    } while (0)

namespace pddc {

/* windows of `window` items, `hop` apart, that lie completely inside the first `len` items of a stream */
inline uint64_t windows_complete(int window, int hop, uint64_t len)
{
    return len >= (uint64_t)window ? (len - (uint64_t)window) / (uint64_t)hop + 1 : 0;
}

/* the channels (first + i) mod nchan, i < count */
inline bool channel_range_ok(int nchan, int first, int count)
{
    return first >= 0 && first < nchan && count >= 1 && count <= nchan;
}

/* a channel list: channels[0 .. n), 1 <= n <= kChannelListMax, each in [0, nchan), pairwise distinct, any order */
static constexpr int kChannelListMax = 1024;
inline bool channel_list_ok(int nchan, const int *channels, int n)
{
    if (!channels || n < 1 || n > kChannelListMax || nchan < 1 || nchan > 4096)
        return false;
    bool seen[4096] = {};
    for (int i = 0; i < n; ++i) {
        if (channels[i] < 0 || channels[i] >= nchan || seen[channels[i]])
            return false;
        seen[channels[i]] = true;
    }
    return true;
}

/* hipFuncAttributeMaxDynamicSharedMemorySize of Kernel, once per device (the attribute is per device): every kernel
 * instantiation has flags of its own, so a kernel asks for ONE size wherever it is launched from.  (Two threads may
 * both set the attribute: the same value, harmless.) */
template <auto Kernel> hipError_t raise_dynamic_lds_once(size_t bytes)
{
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    if (!raised[dev & 63]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bytes);
        if (e != hipSuccess)
            return e;
        raised[dev & 63] = true;
    }
    return hipSuccess;
}

/* ... and then the launch: Kernel<<<grid, block, lds, s>>>(args...) under a cap of `lds_cap` bytes (>= lds) */
template <auto Kernel, class... Args>
hipError_t launch_dynamic_lds(size_t lds_cap, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args)
{
    const hipError_t e = raise_dynamic_lds_once<Kernel>(lds_cap);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

} // namespace pddc
#endif
