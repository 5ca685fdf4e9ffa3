// policy_host.h -- the host side of the policy launchers (policy.hip, policy_f32.hip and the four policy_drqn_* / policy_a2c_* files;
// internal, not part of the C-ABI): StreamDevice and LdsAllowance, which every launcher starts with, the DRQN's and the A2C's workspace
// layouts, each taking what differs between float32 and bf16 (the trunk's act-bytes function; the size of a row element).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>

#include "../../include/magent_policy.h"

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

// The DRQN's workspace: the trunk's own (act_bytes: policy_dqn_act_bytes or policy_dqn_f32_act_bytes), then x from the next 256 bytes on
inline size_t drqn_x_offset(int (*act_bytes)(const PolicyDqnShape *, int, size_t *), const PolicyDqnShape *s, int n) {
    size_t act = 0;
    act_bytes(s, n, &act);
    return (act + 255) / 256 * 256;
}

// The A2C's workspace, rows of A2C_HID elements of `elem` bytes: x and h0; with CommNet h1, the column sums' partial sums (float32, one
// row per block of A2C_CS_BLOCK agents) and the sums.  Every part starts on a multiple of 256 bytes.
constexpr int A2C_HID = 512, A2C_CS_BLOCK = 256;
struct A2cLayout { size_t x, h0, h1, part, sum, bytes; int n_blocks; };
inline A2cLayout a2c_layout(int n, bool comm, size_t elem) {
    auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
    A2cLayout L{};
    const size_t rows = up256((size_t)n * A2C_HID * elem);
    L.n_blocks = (n + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    L.x = 0; L.h0 = rows; L.bytes = 2 * rows;
    if (comm) {
        L.h1 = L.bytes; L.part = L.h1 + rows; L.sum = L.part + up256((size_t)L.n_blocks * A2C_HID * sizeof(float));
        L.bytes = L.sum + A2C_HID * sizeof(float);
    }
    return L;
}

}  // namespace magent_amd
