// pnx_launch.hpp -- what the host code of the HIP translation units shares in front of a launch: the check of a HIP call and the
// big-LDS attribute of a kernel.  (The NNLS units keep their own copy of the check, PNX_HIPN in pnx_nnls.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "pnx_internal.hpp"

// a failed HIP call becomes PNX_ERR_HIP with the call's text; for functions that return a pnx error code
#define PNX_HIP(call)                                                                                       \
    do {                                                                                                    \
        hipError_t e__ = (call);                                                                            \
        if (e__ != hipSuccess) return ::pnx::set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

namespace pnx {
// Allows Kernel 160 KB of dynamic LDS on the current device, once per device: function attributes are per device.  Host threads
// may come here at once.  A thread that reads true (acquire) has the release store in front of it and with it the call that set
// the attribute; threads that read false each set the same value again, which is harmless, and then store true.
template <auto Kernel> hipError_t allow_big_lds() {
    static std::atomic<bool> done[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<bool> &d = done[dev & 63];
    if (!d.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        d.store(true, std::memory_order_release);
    }
    return hipSuccess;
}
}  // namespace pnx

// allow_big_lds of the kernel as the launcher names it; a failure carries the text of the call it stands for
#define PNX_ALLOW_BIG_LDS(...)                                                                                                       \
    do {                                                                                                                             \
        hipError_t e__ = ::pnx::allow_big_lds<__VA_ARGS__>();                                                                        \
        if (e__ != hipSuccess)                                                                                                       \
            return ::pnx::set_error(PNX_ERR_HIP, "%s: %s",                                                                           \
                                    "hipFuncSetAttribute((const void *)" #__VA_ARGS__ ", hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)", \
                                    hipGetErrorString(e__));                                                                         \
    } while (0)
