// Monte-Carlo playouts (include/g2048.h, "Monte-Carlo playouts"): the playout kernel and the reduction to Q(s, .).
//
//   playout  persistent, one lane per playout: the board stays in four VGPRs across the launch's n_steps steps, the step
//            sub-keys ride in the kernarg (wave-uniform -> SGPRs), no trajectory is written.  HBM traffic: the lane state,
//            26 B per lane each way (16 B board + mask + done + ret + disc); at t0 == 0 the read side is the 16 B root of
//            the lane's pair instead (R consecutive lanes read the same root: one cache line per 4 R lanes).
//            A wave leaves the loop when all of its lanes are done.  LDS: the live counter's four words only.
//   reduce   one lane per (board, action) pair walks its R consecutive lanes in ascending order: no atomics, no cross-lane
//            combine, so q does not depend on scheduling.
//
// The per-lane code is g2048_mc.h, shared with the host build the CPU tests compare against the numpy restatement.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_mc.h"

using namespace g2048;
using namespace g2048_host;

static_assert(MC_POLICY_DRUL == G2048_POLICY_DRUL && MC_POLICY_RANDOM == G2048_POLICY_RANDOM, "g2048_mc.h restates the policy ids");

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPlayouts = 1024;

struct McKeyTable {
    u32 k[G2048_MAX_FUSED_STEPS][4];  // act sub-key, step sub-key per step (wave-uniform -> SGPRs)
};

// *live_count += lanes of this workgroup that are still running: ONE atomic per workgroup, none for a workgroup without live
// lanes (the fused engine's counter, under a name of its own).  All lanes of the workgroup reach this call.
__device__ __forceinline__ void mc_count_live(bool lane_live, u32 *live_count) {
    if (!live_count) return;  // (uniform)
    __shared__ u32 wave_live[kBlock / 64];
    const unsigned long long b = __ballot(lane_live);
    if ((threadIdx.x & 63) == 0) wave_live[threadIdx.x >> 6] = (u32)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 n = 0;
        for (int w = 0; w < kBlock / 64; ++w) n += wave_live[w];
        if (n) atomicAdd(live_count, n);
    }
}

template <int MODE, int POLICY>
__global__ void __launch_bounds__(kBlock) k_mc_playout(const McKeyTable keys, int n_steps, int seed, const uint8_t *roots, u32 R,
                                                       u32 n, u32 lane0, u32 n_total, float gamma, uint8_t *lane_boards,
                                                       uint8_t *lane_masks, uint8_t *lane_done, float *lane_ret, float *lane_disc,
                                                       u32 *live_count) {
    const u32 j = blockIdx.x * (u32)kBlock + threadIdx.x;  // (n < 2^31: no wrap)
    const bool in_range = j < n;
    McLane L;
    u32 a_root = 0;
    L.bd.r[0] = L.bd.r[1] = L.bd.r[2] = L.bd.r[3] = 0;
    L.mask = 0xF;
    L.done = 1;
    L.ret = 0.0f;
    L.disc = 1.0f;
    if (in_range) {
        if (seed) {
            const u32 pair = j / R;
            a_root = pair & 3u;
            mc_seed(L, load_board(roots, (int64_t)(pair >> 2)), a_root);
        } else {
            L.bd = load_board(lane_boards, j);
            L.mask = lane_masks[j];
            L.done = lane_done[j];
            L.ret = lane_ret[j];
            L.disc = lane_disc[j];
        }
    }
    const u32 g = lane0 + j;
    for (int s = 0; s < n_steps; ++s) {
        if (__all(L.done != 0)) break;  // every playout of this wave has ended
        mc_step<MODE, POLICY>(L, seed && s == 0, a_root, keys.k[s][0], keys.k[s][1], keys.k[s][2], keys.k[s][3], n_total, g, gamma);
    }
    if (in_range) {
        store_board(lane_boards, j, L.bd);
        lane_masks[j] = (uint8_t)L.mask;
        lane_done[j] = (uint8_t)L.done;
        lane_ret[j] = L.ret;
        lane_disc[j] = L.disc;
    }
    mc_count_live(in_range && L.done == 0, live_count);
}

__global__ void __launch_bounds__(kBlock) k_mc_reduce(const float *lane_ret, const float *lane_disc, const uint8_t *lane_done,
                                                      const float *leaf_values, int64_t pairs, int R, float *q) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= pairs) return;
    q[p] = mc_reduce_pair(lane_ret, lane_disc, lane_done, leaf_values, p * R, R);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }

}  // namespace

extern "C" {

int g2048_mc_playout(const uint32_t *step_subs, int n_steps, int64_t t0, const uint8_t *roots, int64_t B, int R, int64_t lane0,
                     int64_t n_total, int policy, double gamma, uint8_t *lane_boards, uint8_t *lane_masks, uint8_t *lane_done,
                     float *lane_ret, float *lane_disc, int rng_mode, uint32_t *live_count, void *stream) {
    if (!step_subs || n_steps <= 0 || n_steps > G2048_MAX_FUSED_STEPS || t0 < 0 || (t0 == 0 && !roots) || !lane_boards ||
        !lane_masks || !lane_done || !lane_ret || !lane_disc)
        return G2048_EINVAL;
    if (R < 1 || R > kMaxPlayouts || B <= 0 || lane0 < 0 || n_total <= 0 || n_total >= ((int64_t)1 << 31) || B > n_total ||
        lane0 > n_total || lane0 + 4 * B * R > n_total)
        return G2048_EINVAL;
    if ((policy != G2048_POLICY_DRUL && policy != G2048_POLICY_RANDOM) || !(gamma > 0.0 && gamma <= 1.0) ||
        (rng_mode != G2048_RNG_LEGACY && rng_mode != G2048_RNG_PARTITIONABLE))
        return G2048_EINVAL;
    if (!aligned16(roots, lane_boards) || !aligned4(lane_ret) || !aligned4(lane_disc) || !aligned4(live_count)) return G2048_EINVAL;
    McKeyTable tab;
    for (int s = 0; s < n_steps; ++s)
        for (int c = 0; c < 4; ++c) tab.k[s][c] = step_subs[4 * s + c];
    const int64_t n = 4 * B * R;
#define G2048_MC(M, P)                                                                                                          \
    hipLaunchKernelGGL((k_mc_playout<M, P>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, tab, n_steps,           \
                       (int)(t0 == 0), roots, (u32)R, (u32)n, (u32)lane0, (u32)n_total, (float)gamma, lane_boards, lane_masks, \
                       lane_done, lane_ret, lane_disc, live_count)
    if (rng_mode) {
        if (policy == G2048_POLICY_RANDOM) G2048_MC(1, G2048_POLICY_RANDOM);
        else G2048_MC(1, G2048_POLICY_DRUL);
    } else {
        if (policy == G2048_POLICY_RANDOM) G2048_MC(0, G2048_POLICY_RANDOM);
        else G2048_MC(0, G2048_POLICY_DRUL);
    }
#undef G2048_MC
    return launch_status();
}

int g2048_mc_reduce(const float *lane_ret, const float *lane_disc, const uint8_t *lane_done, const float *leaf_values, int64_t B,
                    int R, float *q, void *stream) {
    if (!lane_ret || !lane_disc || !lane_done || !q || R < 1 || R > kMaxPlayouts || B <= 0 || B > ((int64_t)1 << 29) ||
        4 * B * R >= ((int64_t)1 << 31))
        return G2048_EINVAL;
    if (!aligned4(lane_ret) || !aligned4(lane_disc) || !aligned4(leaf_values) || !aligned4(q)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_mc_reduce, dim3(blocks_for(4 * B)), dim3(kBlock), 0, (hipStream_t)stream, lane_ret, lane_disc, lane_done,
                       leaf_values, 4 * B, R, q);
    return launch_status();
}

}  // extern "C"
