// policy_host.h -- the host side of the policy launchers (policy.hip, policy_f32.hip and the four policy_drqn_* / policy_a2c_* files;
// internal, not part of the C-ABI): StreamDevice and LdsAllowance, which every launcher starts with, the DRQN's and the A2C's workspace
// layouts, each taking what differs between float32 and bf16 (the trunk's act-bytes function; the size of a row element), and the
// segmented A2C call's table, its validation and its workspace layout.
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

// ---- the segmented A2C call (policy_a2c_infer*_seg): n packed rows and a table of segments (begin, count); every CommNet mean runs over
// the rows of the agent's own segment.  The table travels to the device by value, as the argument of k_a2c_segmap_* (seg_map in
// policy_f32_dev.h), which writes what the other kernels read into the workspace: no allocation, no copy, no host wait.
constexpr int A2C_MAX_SEGMENTS = POLICY_A2C_MAX_SEGMENTS;
struct A2cSegTable { int n_seg; int begin[A2C_MAX_SEGMENTS]; int count[A2C_MAX_SEGMENTS]; };

// The table as the C-ABI states it: 0 <= n_seg <= the cap, begin and count >= 0, begin + count <= n, ascending and disjoint.
inline bool a2c_seg_table(const int *seg_begin, const int *seg_count, int n_seg, int n, A2cSegTable *out) {
    if (n_seg < 0 || n_seg > A2C_MAX_SEGMENTS || (n_seg > 0 && (!seg_begin || !seg_count))) return false;
    long long at = 0;                                            // the first row behind the segments so far
    for (int s = 0; s < n_seg; s++) {
        const long long b = seg_begin[s], c = seg_count[s];
        if (b < 0 || c < 0 || b < at || b + c > (long long)(n < 0 ? 0 : n)) return false;
        at = b + c;
        out->begin[s] = (int)b; out->count[s] = (int)c;
    }
    out->n_seg = n_seg;
    return true;
}

// The segmented call's workspace: a2c_layout's rows; then (CommNet) one partial row per block of A2C_CS_BLOCK agents counted from each
// segment's own first row -- at most n / A2C_CS_BLOCK + n_seg of them --, one sum row per segment, and seg_map's tables:
//   row_seg int[n]                 the segment of every row, -1 for a row in none (a pad row, a stale row: a segment of one)
//   seg_tab int[n_seg][4]          begin, count, first partial row, partial rows
//   blk_map int[part rows][2]      the (segment, block in the segment) of every partial row
struct A2cSegLayout { size_t x, h0, h1, part, sum, row_seg, seg_tab, blk_map, bytes; int max_blocks; };
inline A2cSegLayout a2c_seg_layout(int n, bool comm, size_t elem, int n_seg) {
    auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
    const A2cLayout P = a2c_layout(n, false, elem);
    A2cSegLayout L{};
    L.x = P.x; L.h0 = P.h0; L.bytes = P.bytes;
    if (comm) {
        const size_t rows = L.h0;
        L.max_blocks = n / A2C_CS_BLOCK + n_seg;
        L.h1 = L.bytes; L.part = L.h1 + rows;
        L.sum = L.part + up256((size_t)L.max_blocks * A2C_HID * sizeof(float));
        L.row_seg = L.sum + (size_t)(n_seg > 0 ? n_seg : 1) * A2C_HID * sizeof(float);
        L.seg_tab = L.row_seg + up256((size_t)n * sizeof(int));
        L.blk_map = L.seg_tab + up256((size_t)n_seg * 4 * sizeof(int));
        L.bytes = L.blk_map + up256((size_t)L.max_blocks * 2 * sizeof(int));
    }
    return L;
}
// the partial rows the table takes: sum over the segments of ceil(count / A2C_CS_BLOCK)
inline int a2c_seg_blocks(const A2cSegTable &t) {
    int nb = 0;
    for (int s = 0; s < t.n_seg; s++) nb += (t.count[s] + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    return nb;
}

}  // namespace magent_amd
