// policy_host.h -- the host side every policy launcher starts with (policy.hip and the three policy_*_f32.hip; internal, not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

namespace magent_amd {

// The stream's device made current for the life of the object (launches and function attributes are per device; a null stream: the
// caller's device).  The caller's current device is put back when the scope ends: a C-ABI call must not leave a side effect in a
// multi-GPU process.  !ok: the runtime refused -- the launcher returns 2, and nothing is put back.
struct StreamDevice {
    int dev = 0, caller = -1;
    bool ok = false;
    explicit StreamDevice(hipStream_t st) {
        if (hipGetDevice(&caller) != hipSuccess) return;
        if (st) { if (hipStreamGetDevice(st, &dev) != hipSuccess || hipSetDevice(dev) != hipSuccess) return; }
        else dev = caller;
        ok = true;
    }
    ~StreamDevice() { if (ok && dev != caller) (void)hipSetDevice(caller); }
    StreamDevice(const StreamDevice &) = delete;
    StreamDevice &operator=(const StreamDevice &) = delete;
};

// The dynamic-LDS allowance of a launcher's kernels, granted once per DEVICE (not once per process); one static object per launcher.
struct LdsAllowance {
    static constexpr int MAX_DEV = 64;
    bool done[MAX_DEV] = {};
    struct Kernel { const void *f; int bytes; };
    // false: a device index outside the table, or the runtime refused (the launcher returns 2; the next call tries again)
    bool grant(int dev, std::initializer_list<Kernel> kernels) {
        if (dev < 0 || dev >= MAX_DEV) return false;
        if (done[dev]) return true;
        for (const Kernel &k : kernels)
            if (hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes) != hipSuccess) return false;
        return done[dev] = true;
    }
};

}  // namespace magent_amd
