// actors.hip -- the reference's rule-based actors (src/temp_c_booster.cc): its three C symbols on the host, and one device
// entry that runs the same policies as scans of device observations (include/magent_runtime_api.h PART 3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/magent_runtime_api.h"
#include "actors_dev.h"

using namespace magent_amd::actors;

[[noreturn]] static void actor_fatal(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "magent-amd FATAL: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    abort();
}

// ------------------------------------------------------------------------------------------------ host: the reference's loops
// temp_c_booster.cc:14-37
extern "C" void runaway_infer_action(float *obs_buf, float *, int n, int height, int width, int n_channel, int, int *act_buf,
                                     int away_channel, int move_back) {
    const size_t stride = (size_t)height * width * n_channel;
    for (int i = 0; i < n; i++)
        act_buf[i] = runaway_sees(obs_buf + i * stride, height, width, n_channel, away_channel) ? move_back : move_back + 1;
}

// temp_c_booster.cc:39-83
extern "C" void rush_prey_infer_action(float *obs_buf, float *feature_buf, int n, int height, int width, int n_channel, int *act_buf,
                                       int attack_channel, int attack_base, int *view2attack_buf, float threshold) {
    const size_t stride = (size_t)height * width * n_channel;
    const int cells = height * width;
    for (int i = 0; i < n; i++) {
        if (!(feature_buf[i] < threshold)) {            // (the i-th float of the flattened feature array, as there)
            act_buf[i] = (int)(random() % attack_base);
            continue;
        }
        const float *obs = obs_buf + i * stride;
        int action = -1;
        bool found = false;
        for (int c = 0; c < cells; c++) {
            if (rush_hit(obs + (size_t)c * n_channel, attack_channel)) {
                found = true;
                if (view2attack_buf[c] != -1) {
                    action = view2attack_buf[c];
                    break;
                }
            }
        }
        if (action != -1)
            act_buf[i] = attack_base + action;
        else if (found && rush_forward_free(obs, height, width, n_channel))
            act_buf[i] = 0;
        else
            act_buf[i] = (int)(random() % attack_base);
    }
}

// temp_c_booster.cc:115-181
extern "C" void gather_infer_action(float *obs_buf, float *, int n, int height, int width, int n_channel, int *act_buf,
                                    int attack_base, int *view2attack_buf) {
    const size_t stride = (size_t)height * width * n_channel;
    std::vector<int> att;
    std::vector<std::pair<int, int>> disp;
    std::vector<std::pair<float, std::pair<int, int>>> minimap;
    for (int i = 0; i < n; i++) {
        const float *obs = obs_buf + i * stride;
        auto at = [&](int row, int col, int ch) { return obs[((size_t)row * width + col) * n_channel + ch]; };
        int action = -1;

        // food in view
        att.clear();
        disp.clear();
        for (int row = 0; row < height; row++)
            for (int col = 0; col < width; col++) {
                if (!gather_food(at(row, col, 4))) continue;
                int v2a = view2attack_buf[row * width + col];
                if (v2a != -1) {
                    att.push_back(v2a + attack_base);
                } else {
                    int d_row = row - height / 2, d_col = col - width / 2;
                    if (d_row == d_col && abs(d_col) == 1) {    // (a draw for every such cell, as there)
                        if (rand() & 1)
                            d_row = 0;
                        else
                            d_col = 0;
                    }
                    disp.push_back(std::make_pair(d_row, d_col));
                }
            }
        if (!att.empty())
            action = att[rand() % att.size()];
        else if (!disp.empty())
            action = get_action(disp[0].first, disp[0].second, false);

        // minimap navigation
        if (action == -1) {
            std::pair<int, int> mypos = std::make_pair(-1, -1);
            for (int row = 0; row < height; row++)
                for (int col = 0; col < width; col++)
                    if (at(row, col, 3) > 1.0f) mypos = std::make_pair(row, col);
            minimap.clear();
            for (int row = 0; row < height; row++)
                for (int col = 0; col < width; col++)
                    if (at(row, col, 6) > 0.0f)
                        minimap.push_back(std::make_pair(at(row, col, 6), std::make_pair(row - mypos.first, col - mypos.second)));
            if (minimap.empty()) {
                action = rand() % attack_base;          // (the reference divides by zero here)
            } else {
                std::sort(minimap.rbegin(), minimap.rend());
                const std::pair<int, int> &d = minimap[rand() % minimap.size()].second;
                action = get_action(d.first, d.second, true);
                if (action == 6) action = rand() % attack_base;
            }
        }
        act_buf[i] = action;
    }
}

// ------------------------------------------------------------------------------------------------ device
// runaway: one lane per agent; it touches the 9 cells' cache lines of its own view, nothing else
__global__ __launch_bounds__(256) void k_actor_runaway(const float *__restrict__ view, int n, int H, int W, int C, int ch, int move_back,
                                                       int *__restrict__ actions, unsigned char *__restrict__ drew) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    actions[i] = runaway_sees(view + (size_t)i * H * W * C, H, W, C, ch) ? move_back : move_back + 1;
    if (drew) drew[i] = 0;
}

// The scanning kernels: one wave per agent, four agents per workgroup.  The wave's lanes take the view's cells 64 at a time
// in row-major order; a first hit is the lowest set lane of a ballot, "any" a non-zero ballot, the k-th element of a set the
// lane whose prefix popcount is k.  view2attack is copied to LDS once per workgroup; the four actions leave in one 16-byte store.
constexpr int ACTOR_WAVES = 4;

// the cell of the k-th (0-based, row-major) cell of the view for which pred(c) holds; k < the set's size
template <typename Pred>
__device__ inline int kth_cell(int cells, int lane, int k, Pred pred) {
    int before = 0;
    for (int base = 0; base < cells; base += 64) {
        int c = base + lane;
        bool in = c < cells && pred(c);
        unsigned long long m = __ballot(in);
        int cnt = __popcll(m);
        if (k < before + cnt) {
            int rank = __popcll(m & ((1ull << lane) - 1ull));
            unsigned long long sel = __ballot(in && rank == k - before);
            return base + __ffsll(sel) - 1;
        }
        before += cnt;
    }
    return -1;   // (not reached for k below the set's size)
}

__global__ __launch_bounds__(256) void k_actor_rush(const float *__restrict__ view, const float *__restrict__ feature,
                                                    const int *__restrict__ view2attack, MagentActorArgs a,
                                                    int *__restrict__ actions, unsigned char *__restrict__ drew) {
    extern __shared__ int s_v2a[];
    __shared__ int s_act[ACTOR_WAVES];
    __shared__ unsigned char s_drew[ACTOR_WAVES];
    const int cells = a.height * a.width, C = a.n_channel;
    for (int c = threadIdx.x; c < cells; c += blockDim.x) s_v2a[c] = view2attack[c];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * ACTOR_WAVES + wave;
    if (i < a.n) {                                       // (wave-uniform)
        const float *obs = view + (size_t)i * cells * C;
        int act = -1;
        bool drawn = false;
        if (feature[i] < a.threshold) {
            bool found = false;
            int first = -1;
            for (int base = 0; base < cells; base += 64) {
                int c = base + lane;
                bool hit = c < cells && rush_hit(obs + (size_t)c * C, a.channel);
                unsigned long long m_hit = __ballot(hit);
                unsigned long long m_att = __ballot(hit && s_v2a[c] != -1);
                found |= m_hit != 0;
                if (m_att) {
                    first = base + __ffsll(m_att) - 1;
                    break;
                }
            }
            if (first >= 0)
                act = a.attack_base + s_v2a[first];
            else if (found && rush_forward_free(obs, a.height, a.width, C))
                act = 0;
        }
        if (act < 0) {
            act = (int)draw(a.seed, a.counter, (uint32_t)i, 0, (uint32_t)a.attack_base);
            drawn = true;
        }
        if (lane == 0) s_act[wave] = act, s_drew[wave] = drawn;
    }
    __syncthreads();
    int j = blockIdx.x * ACTOR_WAVES + threadIdx.x;
    if (threadIdx.x < ACTOR_WAVES && j < a.n) {
        actions[j] = s_act[threadIdx.x];
        if (drew) drew[j] = s_drew[threadIdx.x];
    }
}

__global__ __launch_bounds__(256) void k_actor_gather(const float *__restrict__ view, const int *__restrict__ view2attack,
                                                      MagentActorArgs a, int *__restrict__ actions, unsigned char *__restrict__ drew) {
    extern __shared__ int s_v2a[];
    __shared__ int s_act[ACTOR_WAVES];
    __shared__ unsigned char s_drew[ACTOR_WAVES];
    const int H = a.height, W = a.width, cells = H * W, C = a.n_channel;
    for (int c = threadIdx.x; c < cells; c += blockDim.x) s_v2a[c] = view2attack[c];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * ACTOR_WAVES + wave;
    if (i < a.n) {                                       // (wave-uniform)
        const float *obs = view + (size_t)i * cells * C;
        // one pass: food that can be attacked (count), the first food that cannot, my position (the last cell with
        // channel 3 > 1), minimap cells (count)
        int n_att = 0, first_disp = -1, mypos = -1, n_map = 0;
        for (int base = 0; base < cells; base += 64) {
            int c = base + lane;
            bool in = c < cells;
            const float *cell = obs + (size_t)(in ? c : 0) * C;
            float f3 = cell[3], f4 = cell[4], f6 = cell[6];
            bool food = in && gather_food(f4);
            bool att = food && s_v2a[c] != -1;
            unsigned long long m_att = __ballot(att);
            unsigned long long m_disp = __ballot(food && !att);
            unsigned long long m_me = __ballot(in && f3 > 1.0f);
            unsigned long long m_map = __ballot(in && f6 > 0.0f);
            n_att += __popcll(m_att);
            if (first_disp < 0 && m_disp) first_disp = base + __ffsll(m_disp) - 1;
            if (m_me) mypos = base + 63 - __clzll(m_me);
            n_map += __popcll(m_map);
        }
        int act;
        bool drawn = true;
        if (n_att > 0) {
            int k = (int)draw(a.seed, a.counter, (uint32_t)i, 0, (uint32_t)n_att);
            int c = kth_cell(cells, lane, k, [&](int c) { return gather_food(obs[(size_t)c * C + 4]) && s_v2a[c] != -1; });
            act = s_v2a[c] + a.attack_base;
        } else if (first_disp >= 0) {
            int d_row = first_disp / W - H / 2, d_col = first_disp % W - W / 2;
            drawn = d_row == d_col && abs(d_col) == 1;
            if (drawn) {
                if (draw(a.seed, a.counter, (uint32_t)i, 0, 2))
                    d_row = 0;
                else
                    d_col = 0;
            }
            act = get_action(d_row, d_col, false);
        } else if (n_map == 0) {
            act = (int)draw(a.seed, a.counter, (uint32_t)i, 0, (uint32_t)a.attack_base);
        } else {
            int k = (int)draw(a.seed, a.counter, (uint32_t)i, 0, (uint32_t)n_map);
            int c = kth_cell(cells, lane, k, [&](int c) { return obs[(size_t)c * C + 6] > 0.0f; });
            int my_row = mypos < 0 ? -1 : mypos / W, my_col = mypos < 0 ? -1 : mypos % W;
            act = get_action(c / W - my_row, c % W - my_col, true);
            if (act == 6) act = (int)draw(a.seed, a.counter, (uint32_t)i, 1, (uint32_t)a.attack_base);
        }
        if (lane == 0) s_act[wave] = act, s_drew[wave] = drawn;
    }
    __syncthreads();
    int j = blockIdx.x * ACTOR_WAVES + threadIdx.x;
    if (threadIdx.x < ACTOR_WAVES && j < a.n) {
        actions[j] = s_act[threadIdx.x];
        if (drew) drew[j] = s_drew[threadIdx.x];
    }
}

// view2attack lives in LDS: 64 KiB of it at most
constexpr int ACTOR_MAX_CELLS = 16384;

extern "C" int actor_infer_action_device(const MagentActorArgs *args, const float *view, const float *feature, const int *view2attack,
                                         int *actions, unsigned char *drew, void *stream) {
    if (!args) actor_fatal("actor_infer_action_device: null args");
    const MagentActorArgs a = *args;
    if (a.n < 0) actor_fatal("actor_infer_action_device: n = %d", a.n);
    if (a.n == 0) return 0;
    if (a.height < 1 || a.width < 1 || a.n_channel < 1 || (long long)a.height * a.width > ACTOR_MAX_CELLS)
        actor_fatal("actor_infer_action_device: view %d x %d x %d (at most %d cells)", a.height, a.width, a.n_channel, ACTOR_MAX_CELLS);
    if (!view || !actions) actor_fatal("actor_infer_action_device: null view or actions");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)a.height * a.width * sizeof(int);
    const int blocks = (a.n + ACTOR_WAVES - 1) / ACTOR_WAVES;
    switch (a.kind) {
    case MAGENT_ACTOR_RUNAWAY:
        if (a.channel < 0 || a.channel >= a.n_channel) actor_fatal("actor_infer_action_device: runaway channel %d of %d", a.channel, a.n_channel);
        hipLaunchKernelGGL(k_actor_runaway, dim3((a.n + 255) / 256), dim3(256), 0, st, view, a.n, a.height, a.width, a.n_channel,
                           a.channel, a.move_back, actions, drew);
        break;
    case MAGENT_ACTOR_RUSH_PREY:
        if (a.channel < 0 || a.channel >= a.n_channel || a.n_channel < 2 || a.attack_base < 1 || !feature || !view2attack)
            actor_fatal("actor_infer_action_device: rush_prey needs channels 1 and %d of %d, attack_base >= 1 (%d), feature and view2attack",
                        a.channel, a.n_channel, a.attack_base);
        hipLaunchKernelGGL(k_actor_rush, dim3(blocks), dim3(64 * ACTOR_WAVES), lds, st, view, feature, view2attack, a, actions, drew);
        break;
    case MAGENT_ACTOR_GATHER:
        if (a.n_channel < 7 || a.attack_base < 1 || !view2attack)
            actor_fatal("actor_infer_action_device: gather needs channels 3, 4 and 6 (%d), attack_base >= 1 (%d) and view2attack",
                        a.n_channel, a.attack_base);
        hipLaunchKernelGGL(k_actor_gather, dim3(blocks), dim3(64 * ACTOR_WAVES), lds, st, view, view2attack, a, actions, drew);
        break;
    default:
        actor_fatal("actor_infer_action_device: unknown kind %d", a.kind);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) actor_fatal("actor_infer_action_device: launch failed: %s", hipGetErrorString(e));
    return 0;
}
