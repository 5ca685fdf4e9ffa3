// actors_dev.h -- per-agent decision logic of the rule-based actors (reference src/temp_c_booster.cc), written once for the
// host loops of actors.hip (the reference's three C symbols, byte-exact) and for its device kernels.
//
// An observation is float32 [H][W][C]; cell (row, col) starts at obs + (row * W + col) * C.  Every comparison is the
// reference's own, including its float -> double promotions (`x + 0.5`, `fabs(x - 1.0) < 1e-10`).
#pragma once
#include <stdint.h>

namespace magent_amd {
namespace actors {

// temp_c_booster.cc:85-113
__host__ __device__ inline int get_action(int d_row, int d_col, bool stride) {
    if (d_row < 0) return d_col < 0 ? 1 : (d_col == 0 ? (stride ? 0 : 2) : 3);
    if (d_row == 0) return d_col < 0 ? (stride ? 4 : 5) : (d_col == 0 ? 6 : (stride ? 8 : 7));
    return d_col < 0 ? 9 : (d_col == 0 ? (stride ? 12 : 10) : 11);
}

// runaway (temp_c_booster.cc:22-30): any of rows H-3 .. H-1, columns W/2-1 .. W/2+1 shows the away channel.
// (Cells outside the view -- a view narrower or shorter than 3 -- are skipped.)
__host__ __device__ inline bool runaway_sees(const float *obs, int H, int W, int C, int ch) {
    bool found = false;
    for (int row = H - 3; row <= H - 1; row++)
        for (int col = W / 2 - 1; col <= W / 2 + 1; col++)
            if (row >= 0 && col >= 0 && col < W && obs[((long long)row * W + col) * C + ch] > 0.5f) found = true;
    return found;
}

// rush_prey (temp_c_booster.cc:57): the cell holds the enemy or "food" (channel 1)
__host__ __device__ inline bool rush_hit(const float *cell, int enemy) { return cell[enemy] > 0.5f || cell[1] > 0.5f; }

// rush_prey (temp_c_booster.cc:74): the cell in front (last row, middle column) is not a wall
__host__ __device__ inline bool rush_forward_free(const float *obs, int H, int W, int C) {
    return (int)((double)obs[((long long)(H - 1) * W + W / 2) * C] + 0.5) != 1;
}

// gather (temp_c_booster.cc:128): food presence, compared in double as there (in float32: the value is exactly 1.0)
__host__ __device__ inline bool gather_food(float x) {
    double d = (double)x - 1.0;
    return (d < 0 ? -d : d) < 1e-10;
}

// The device's draws: a stateless counter-based stream.  Draw `slot` of agent `row` in the call numbered
// `counter` of a stream seeded with `seed` is the splitmix64 finaliser applied twice; a value in [0, m) is its high word % m.
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t draw(uint64_t seed, uint64_t counter, uint32_t row, uint32_t slot, uint32_t m) {
    uint64_t key = mix64(seed ^ mix64(counter + 0x9E3779B97F4A7C15ull));
    uint64_t h = mix64(key + 0x9E3779B97F4A7C15ull * ((uint64_t)row * 4u + slot + 1u));
    return (uint32_t)(h >> 32) % m;
}

}  // namespace actors
}  // namespace magent_amd
