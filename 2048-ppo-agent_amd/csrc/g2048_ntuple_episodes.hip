// N-tuple episodes (include/g2048.h, "n-tuple episodes"): a whole greedy evaluation, every batch of the protocol at once and
// every game to its end, in a handful of launches.
//
//   episodes  persistent, one quad per game (16 games per wave): the board, mask, done flag, length, score and the head of the
//             game's key chain stay in registers across the launch's n_steps steps.  Per step lane a of the quad moves the board
//             in direction a, gathers the afterstate's 8 m entries (a lane whose move changes nothing gathers nothing) and the
//             quad takes the engine's masked argmax with two quad-permute DPP moves that carry the action index; then the four
//             lanes run the same env_step on the same keys, which the lane derives itself (two chain steps and one split per
//             step: no host key table, games of different batches share a wave).  A wave leaves the loop when all of its games
//             are done.  HBM traffic per launch: the game state, 38 B per game each way (16 B board + mask + done + 4 B length +
//             8 B score + 8 B chain; at start only the 8 B chain is read); per game-step nothing but the gathers.  Lane 0 of the
//             quad owns the stores.  LDS: the live counter's four words only.  No spinning, no cross-workgroup communication.
//
// The per-lane code is g2048_ntuple_episodes.h, shared with the host build the CPU tests compare against the numpy restatement.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_episodes.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxGames = (int64_t)1 << 24;  // 4 lanes per game stay far below 2^31
constexpr int64_t kMaxBatch = (int64_t)1 << 20;
constexpr int kMaxSteps = 65536;

// *live_count += games of this workgroup that are still running: ONE atomic per workgroup, none for a workgroup without live
// games (the fused engine's counter, under a name of its own).  All lanes of the workgroup reach this call.
__device__ __forceinline__ void nte_count_live(bool lane_live, u32 *live_count) {
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

// x of the lane whose index differs in bit 0 (0xB1 = quad_perm [1,0,3,2]) / bit 1 (0x4E = quad_perm [2,3,0,1])
template <int CTRL>
__device__ __forceinline__ u32 quad_swap(u32 x) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}

// one round of the quad's argmax: (x, a) against the partner's pair
template <int CTRL>
__device__ __forceinline__ void quad_argmax_round(float &x, u32 &a) {
    const float xo = __uint_as_float(quad_swap<CTRL>(__float_as_uint(x)));
    const u32 ao = quad_swap<CTRL>(a);
    const bool take = nte_beats(xo, ao, x, a);
    x = take ? xo : x;
    a = take ? ao : a;
}

template <int MODE, int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_episodes(int start, int n_steps, u32 N, u32 bs, const int32_t *weights,
                                                         const NtNet net_arg, float scale, u32 *chain, uint8_t *boards,
                                                         uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score,
                                                         u32 *live_count) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    // every lane stays to the end: the quad moves below want whole quads (4 N lanes: the last quad in range is whole too)
    const u32 t = blockIdx.x * (u32)kBlock + threadIdx.x;  // (4 N <= 2^26: no wrap)
    const u32 i = t >> 2, a = t & 3u;
    const bool in_range = i < N;
    NteGame G;
    G.bd.r[0] = G.bd.r[1] = G.bd.r[2] = G.bd.r[3] = 0;
    G.mask = 0xF;
    G.done = 1;
    G.len = 0;
    G.score = 0;
    G.c0 = G.c1 = 0;
    u32 g = 0, B_total = 1;
    if (in_range) {
        nte_place(i, N, bs, g, B_total);
        const u32 c0 = chain[2 * i], c1 = chain[2 * i + 1];  // (4-byte aligned: two loads)
        if (start) {
            nte_seed<MODE>(G, c0, c1, B_total, g);
        } else {
            G.bd = load_board(boards, i);
            G.mask = masks[i];
            G.done = done[i];
            G.len = (u32)ep_len[i];
            G.score = score[i];
            G.c0 = c0;
            G.c1 = c1;
        }
    }
    for (int s = 0; s < n_steps; ++s) {
        if (__all(G.done != 0)) break;  // every game of this wave has ended
        float x = -3.40282347e38f;
        if (!G.done) x = nte_logit<M>(weights, net, scale, G, a);  // (quad-uniform: a finished game gathers nothing)
        u32 act = a;
        quad_argmax_round<0xB1>(x, act);
        quad_argmax_round<0x4E>(x, act);
        nte_step<MODE>(G, act, B_total, g);
    }
    if (in_range && a == 0) {
        chain[2 * i] = G.c0;
        chain[2 * i + 1] = G.c1;
        store_board(boards, i, G.bd);
        masks[i] = (uint8_t)G.mask;
        done[i] = (uint8_t)G.done;
        ep_len[i] = (int32_t)G.len;
        score[i] = G.score;
    }
    nte_count_live(in_range && a == 0 && G.done == 0, live_count);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NTE_LAUNCH_M(MODE, STAGED, m, n, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((k_nt_episodes<MODE, 1, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((k_nt_episodes<MODE, 2, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((k_nt_episodes<MODE, 3, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((k_nt_episodes<MODE, 4, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((k_nt_episodes<MODE, 5, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((k_nt_episodes<MODE, 6, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((k_nt_episodes<MODE, 7, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((k_nt_episodes<MODE, 8, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read: a single stage launches the kernel without stage work
#define G2048_NTE_LAUNCH(MODE, m, n, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NTE_LAUNCH_M(MODE, true, m, n, stream, __VA_ARGS__) \
    } else { \
        G2048_NTE_LAUNCH_M(MODE, false, m, n, stream, __VA_ARGS__) \
    }

extern "C" {

int g2048_ntuple_staged_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights, const uint8_t *tuple_cells,
                                 int m, int L, const uint8_t *stage_tiles, int n_stages, int frac_bits, uint32_t *chain,
                                 uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score, int rng_mode,
                                 uint32_t *live_count, void *stream) {
    NtNet net;
    if (!weights || !chain || !boards || !masks || !done || !ep_len || !score || N < 1 || N > kMaxGames || bs < 1 || bs > kMaxBatch ||
        n_steps < 1 || n_steps > kMaxSteps || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) ||
        (rng_mode != G2048_RNG_LEGACY && rng_mode != G2048_RNG_PARTITIONABLE))
        return G2048_EINVAL;
    if (!aligned16(boards) || !aligned8(score) || !aligned4(chain) || !aligned4(ep_len) || !aligned4(weights) || !aligned4(live_count))
        return G2048_EINVAL;
    const int st = start != 0;
    const float scale = nt_scale(frac_bits);
    if (rng_mode) {
        G2048_NTE_LAUNCH(1, m, 4 * N, stream, st, n_steps, (u32)N, (u32)bs, weights, net, scale, chain, boards, masks, done, ep_len, score,
                         live_count);
    } else {
        G2048_NTE_LAUNCH(0, m, 4 * N, stream, st, n_steps, (u32)N, (u32)bs, weights, net, scale, chain, boards, masks, done, ep_len, score,
                         live_count);
    }
    return launch_status();
}

int g2048_ntuple_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights, const uint8_t *tuple_cells, int m,
                          int L, int frac_bits, uint32_t *chain, uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len,
                          int64_t *score, int rng_mode, uint32_t *live_count, void *stream) {
    return g2048_ntuple_staged_episodes(start, n_steps, N, bs, weights, tuple_cells, m, L, nullptr, 1, frac_bits, chain, boards, masks,
                                        done, ep_len, score, rng_mode, live_count, stream);
}

}  // extern "C"
