// policy_host.h -- the host side of the policy launchers (policy.hip, policy_f32.hip and the four policy_drqn_* / policy_a2c_* files;
// internal, not part of the C-ABI): StreamDevice and LdsAllowance, which every launcher starts with, and the DRQN's workspace layout,
// taking what differs between float32 and bf16 (the trunk's act-bytes function), and what policy_a2c_f32.hip and policy_a2c_bf16.hip share
// below their GEMM kernels: the workspace layout, the segmented call's table check, the five small kernels that do not depend on the
// precision beyond the type of a row element (the segment maps and the CommNet column sums), and a2c_infer, the one driver of all six
// inference entries.  An A2C file holds its trunk, layer and head kernels and a trait that launches them; everything between those
// launches is here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/magent_policy.h"
#include "policy_f32_dev.h"

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

inline bool a2c_seg_table(const int *seg_begin, const int *seg_count, int n_seg, int n, A2cSegTable *out);      // (below, with the A2C's segmented call)

// ---- the segmented DRQN step (policy_drqn_lookup_seg*, then policy_drqn_infer*_rows): the state table is keyed by (segment, id)
// (policy_f32_dev.h: drqn_key).  The look-up is a divergent binary search per lane; it runs in ONE small launch of its own over all rows
// of the call, whatever the chunks the GRU steps are cut into afterwards, and the GRU kernels read the row it found.  The kernel is a
// template of the file family's tag as the A2C's small kernels are of their row type: only a translation unit that launches it holds it.
constexpr int DRQN_LK_THREADS = 256;
template <class Tag>
static __global__ void __launch_bounds__(DRQN_LK_THREADS) k_drqn_lookup_seg(A2cSegTable t, int n, const int *ids, int seg_first, const long long *prev_keys,
                                                                           const int *rows, int count, int *from_row, long long *keys) {
    const int r = blockIdx.x * DRQN_LK_THREADS + threadIdx.x;
    if (r < n) f32::drqn_lookup_row(r, ids, t, seg_first, prev_keys, rows, count, from_row, keys);
}
// Both exported look-ups.  The table as the segmented A2C entries state it (a2c_seg_table: its format, validation and cap); 0; 1: a
// refused argument (nothing is written); 2: the runtime refused the device; 3: the launch failed.
template <class Tag>
int drqn_lookup_seg(const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, int seg_first, const long long *prev_sorted_keys,
                    const int *rows, int count, int *from_row, long long *keys, void *stream) {
    A2cSegTable table;
    if (!a2c_seg_table(seg_begin, seg_count, n_seg, n, &table)) return 1;
    if (seg_first < 0 || seg_first > 0x7FFFFFFF - A2C_MAX_SEGMENTS - 1 || count < 0 || (count > 0 && !(prev_sorted_keys && rows))) return 1;
    if (n <= 0) return 0;
    if (!ids || !from_row || !keys) return 1;
    hipStream_t st = (hipStream_t)stream;
    StreamDevice on(st);
    if (!on.ok) return 2;
    hipLaunchKernelGGL(k_drqn_lookup_seg<Tag>, dim3((n + DRQN_LK_THREADS - 1) / DRQN_LK_THREADS), dim3(DRQN_LK_THREADS), 0, st, table, n, ids, seg_first,
                       prev_sorted_keys, rows, count, from_row, keys);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// ---- the segmented A2C call (policy_a2c_infer*_seg): every CommNet mean runs over the rows of the agent's own segment.  k_a2c_segmap
// writes what the other kernels read of the table (policy_f32_dev.h: A2cSegTable) into the workspace: no allocation, no copy, no host wait.
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
// the partial rows the table takes: sum over the segments of ceil(count / A2C_CS_BLOCK)
inline int a2c_seg_blocks(const A2cSegTable &t) {
    int nb = 0;
    for (int s = 0; s < t.n_seg; s++) nb += (t.count[s] + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    return nb;
}

// The workspace, rows of A2C_HID elements of `elem` bytes: x and h0; with CommNet h1, the column sums' partial rows (float32) and the sum
// rows.  Every part starts on a multiple of 256 bytes.  n_seg < 0, the plain call: one partial row per block of A2C_CS_BLOCK agents of
// the call and one sum row.  n_seg >= 0, the segmented call: one partial row per block of A2C_CS_BLOCK agents counted from each segment's
// own first row -- at most n / A2C_CS_BLOCK + n_seg of them --, one sum row per segment, and k_a2c_segmap's tables:
//   row_seg int[n]                 the segment of every row, -1 for a row in none (a pad row, a stale row: a segment of one)
//   seg_tab int[n_seg][4]          begin, count, first partial row, partial rows
//   blk_map int[part rows][2]      the (segment, block in the segment) of every partial row
struct A2cLayout { size_t x, h0, h1, part, sum, row_seg, seg_tab, blk_map, bytes; int part_rows; };
inline A2cLayout a2c_layout(int n, bool comm, size_t elem, int n_seg) {
    auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
    const bool seg = n_seg >= 0;
    A2cLayout L{};
    const size_t rows = up256((size_t)n * A2C_HID * elem);
    L.part_rows = seg ? n / A2C_CS_BLOCK + n_seg : (n + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    L.x = 0; L.h0 = rows; L.bytes = 2 * rows;
    if (comm) {
        L.h1 = L.bytes; L.part = L.h1 + rows; L.sum = L.part + up256((size_t)L.part_rows * A2C_HID * sizeof(float));
        L.bytes = L.sum + (size_t)(n_seg > 0 ? n_seg : 1) * A2C_HID * sizeof(float);
        if (seg) {
            L.row_seg = L.bytes;
            L.seg_tab = L.row_seg + up256((size_t)n * sizeof(int));
            L.blk_map = L.seg_tab + up256((size_t)n_seg * 4 * sizeof(int));
            L.bytes = L.blk_map + up256((size_t)L.part_rows * 2 * sizeof(int));
        }
    }
    return L;
}
// the four *_workspace_bytes* entries: negative counts are none (the plain entries pass n_seg = -1, the segmented ones max(n_seg, 0))
inline size_t a2c_workspace_bytes(int n, int use_comm, size_t elem, int n_seg) { return a2c_layout(n < 0 ? 0 : n, use_comm != 0, elem, n_seg).bytes; }

// ---------------------------------------------------------------------------------------------------- the small kernels
// The CommNet column sums and the segment maps: the bodies are policy_f32_dev.h's, written for rows of either type.  All five are
// templates of the row type, also the three that read no row: only a translation unit that launches them holds them, one copy each.
constexpr int A2C_SM_THREADS = 256;
template <class Row>
static __global__ void __launch_bounds__(A2C_HID) k_a2c_colsum_part(const Row *h, int n, float *part) {
    const int beg = blockIdx.x * A2C_CS_BLOCK;
    f32::colsum_rows(h, beg, min(beg + A2C_CS_BLOCK, n), part, blockIdx.x);
}
template <class Row>
static __global__ void __launch_bounds__(A2C_HID) k_a2c_colsum(const float *part, int n_blocks, float *sum) { f32::colsum_blocks(part, n_blocks, sum); }
template <class Row>
static __global__ void __launch_bounds__(A2C_SM_THREADS) k_a2c_segmap(A2cSegTable t, int n, int *row_seg, int *seg_tab, int *blk_map) {
    f32::seg_map(t, n, row_seg, seg_tab, blk_map);
}
template <class Row>
static __global__ void __launch_bounds__(A2C_HID) k_a2c_colsum_part_seg(const Row *h, const int *seg_tab, const int *blk_map, float *part) {
    f32::colsum_part_seg(h, seg_tab, blk_map, part);
}
template <class Row>
static __global__ void __launch_bounds__(A2C_HID) k_a2c_colsum_seg(const float *part, const int *seg_tab, float *sum) { f32::colsum_blocks_seg(part, seg_tab, sum); }

// ---------------------------------------------------------------------------------------------------- the driver
// One [n] x [A2C_HID] layer as the driver hands it to a trait: the dense layer (in, w, bias, out) or a CommNet step (in, sum, skip, w,
// out; the segmented step also row_seg and seg_tab, and `sum` is then [n_seg][A2C_HID]).  What a form does not read is null.
enum A2cLayerKind { A2C_DENSE, A2C_COMM, A2C_COMM_SEG };
template <class Row>
struct A2cLayerIo { const Row *in; const void *w; const float *bias; Row *out; const float *sum; const Row *skip; const int *row_seg, *seg_tab; };
// the table arguments of a *_seg entry as the caller gave them; {} (on == false): a plain entry
struct A2cSegArgs { bool on; const int *begin, *count; int n_seg; };

// All six policy_a2c_infer* entries.  The precision's trait `p` gives
//   Row, Weights                          the type of a row element of the workspace; the C-ABI's weight struct
//   supported(s), view_weights(w)         the shape region of the entry; its dense_view packing (null: not packed)
//   view_ok(view)                         the alignment the entry's view loads need
//   device_ready(dev)                     what the kernels need granted once per device (false: return 2)
//   trunk(st, s, w, view, feat, n, x)     the launches: the input layers,
//   layer(st, kind, n, io)                one layer,
//   head(st, s, w, h, u, n, actions, policy, value)       the heads and the draw
// 0; 1: a refused argument (a refused table before anything else is looked at); 2: the runtime refused the device; 3: a launch failed.
template <class P>
int a2c_infer(const P &p, const PolicyDqnShape *s, const typename P::Weights *w, const void *view, const float *feat, int n, const float *u,
              void *workspace, int *actions, float *policy, float *value, void *stream, const A2cSegArgs &seg) {
    typedef typename P::Row Row;
    A2cSegTable table;
    if (seg.on && !a2c_seg_table(seg.begin, seg.count, seg.n_seg, n, &table)) return 1;
    if (!s || !w || !p.supported(s)) return 1;
    const bool comm = w->use_comm != 0;
    if (!p.view_weights(w) || !w->dense_emb || !w->dense || !w->head || !w->dense_view_bias || !w->dense_emb_bias || !w->dense_bias || !w->head_bias) return 1;
    if (comm && !(w->comm[0] && w->comm[1])) return 1;
    if (n <= 0) return 0;
    if (!view || !feat || !u || !actions || !workspace) return 1;
    if (((uintptr_t)workspace & 15) || !p.view_ok(view)) return 1;              // (rows are read and written as 16-byte units)
    const A2cSegTable *t = seg.on && comm ? &table : nullptr;                   // (without CommNet every row is its own: the plain call)
    hipStream_t st = (hipStream_t)stream;
    StreamDevice on(st);
    if (!on.ok || !p.device_ready(on.dev)) return 2;
    const A2cLayout L = a2c_layout(n, comm, sizeof(Row), t ? t->n_seg : -1);
    char *ws = (char *)workspace;
    Row *x = (Row *)(ws + L.x), *h0 = (Row *)(ws + L.h0);
    p.trunk(st, s, w, view, feat, n, x);
    A2cLayerIo<Row> D{};
    D.in = x; D.w = w->dense; D.bias = w->dense_bias; D.out = h0;
    p.layer(st, A2C_DENSE, n, D);
    const Row *h = h0;
    if (comm) {
        float *part = (float *)(ws + L.part), *sum = (float *)(ws + L.sum);
        Row *outs[2] = {x, (Row *)(ws + L.h1)};                  // (x is free once the dense layer has read it)
        int *row_seg = (int *)(ws + L.row_seg), *seg_tab = (int *)(ws + L.seg_tab), *blk_map = (int *)(ws + L.blk_map);      // (t only)
        const int seg_blocks = t ? a2c_seg_blocks(*t) : 0;
        if (t) hipLaunchKernelGGL(k_a2c_segmap<Row>, dim3(t->n_seg > 0 ? t->n_seg : 1), dim3(A2C_SM_THREADS), 0, st, *t, n, row_seg, seg_tab, blk_map);
        for (int step = 0; step < 2; step++) {
            A2cLayerIo<Row> C{};
            C.in = h; C.sum = sum; C.skip = h0; C.w = w->comm[step]; C.out = outs[step];
            if (t) {
                if (seg_blocks > 0) {                            // (no agent in any segment: no sum is read)
                    hipLaunchKernelGGL(k_a2c_colsum_part_seg<Row>, dim3(seg_blocks), dim3(A2C_HID), 0, st, h, (const int *)seg_tab, (const int *)blk_map, part);
                    hipLaunchKernelGGL(k_a2c_colsum_seg<Row>, dim3(t->n_seg), dim3(A2C_HID), 0, st, (const float *)part, (const int *)seg_tab, sum);
                }
                C.row_seg = row_seg; C.seg_tab = seg_tab;
            } else {
                hipLaunchKernelGGL(k_a2c_colsum_part<Row>, dim3(L.part_rows), dim3(A2C_HID), 0, st, h, n, part);
                hipLaunchKernelGGL(k_a2c_colsum<Row>, dim3(1), dim3(A2C_HID), 0, st, (const float *)part, L.part_rows, sum);
            }
            p.layer(st, t ? A2C_COMM_SEG : A2C_COMM, n, C);
            h = outs[step];
        }
    }
    p.head(st, s, w, h, u, n, actions, policy, value);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace magent_amd
