// N-tuple searched episodes (include/g2048.h, "n-tuple searched episodes"): a whole one-ply expectimax evaluation, every batch of
// the protocol at once and every game to its end, in a handful of launches.
//
//   search_episodes  persistent, one wavefront per game in one-wave workgroups.  The game (board, mask, done flag, length, score,
//                    chain head) is REPLICATED in all 64 lanes: every lane runs the same nte_step on the same keys, so `done`, the
//                    loop exit and every barrier are workgroup-uniform by construction.  Per step:
//                      1 existence  lane l tests slots l and l + 64; two ballots give the 128-bit set of existing slots and each
//                                   existing slot writes itself to the LDS list at its rank
//                      2 leaf       ceil(4 n_live / 64) rounds of 64 (child, action) pairs, a child per quad: the lane builds the
//                                   child in registers and scores one move on it (8 m gathers), the quad takes the max with two
//                                   quad-permute DPP moves, lane 0 of the quad writes V0(child) to leaf[slot]
//                      3 choose     lanes 0 .. 3 run the serial reduction of their action over leaf, build the engine's logit
//                                   under the game's mask and take the first maximum; the action is broadcast to the wave
//                      4 step       all lanes run nte_step
//                    HBM traffic per launch: the game state, 38 B per game each way (at start only the 8 B chain is read); per
//                    game-step nothing but the gathers.  Lane 0 owns the stores and the one atomic of a live game per launch.
//                    LDS: 128 B list + 512 B leaf.  No spinning, no cross-workgroup communication.
//
// The per-lane and per-wave code is g2048_ntuple_search_episodes.h, shared with the host build the CPU tests compare against the
// numpy restatement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_search_episodes.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = NTSE_WAVE;
constexpr int64_t kMaxGames = (int64_t)1 << 24;  // one workgroup per game
constexpr int64_t kMaxBatch = (int64_t)1 << 20;
constexpr int kMaxSteps = 65536;

// x of the lane whose index differs in bit 0 (0xB1 = quad_perm [1,0,3,2]) / bit 1 (0x4E = quad_perm [2,3,0,1])
template <int CTRL>
__device__ __forceinline__ u32 quad_swap(u32 x) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float quad_swap_f(float x) {
    return __uint_as_float(quad_swap<CTRL>(__float_as_uint(x)));
}

// the max over the legal lanes of a quad, +0 if there is none (every lane of the quad must be active)
__device__ __forceinline__ float quad_best(float q, bool legal) {
    float x = legal ? q : nt_neg_inf();
    x = nt_vmax(x, quad_swap_f<0xB1>(x));
    x = nt_vmax(x, quad_swap_f<0x4E>(x));
    return x == nt_neg_inf() ? 0.0f : x;
}

// one round of the quad's argmax: (x, a) against the partner's pair
template <int CTRL>
__device__ __forceinline__ void quad_argmax_round(float &x, u32 &a) {
    const float xo = quad_swap_f<CTRL>(x);
    const u32 ao = quad_swap<CTRL>(a);
    const bool take = nte_beats(xo, ao, x, a);
    x = take ? xo : x;
    a = take ? ao : a;
}

template <int MODE, int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_search_episodes(int start, int n_steps, u32 N, u32 bs, const int32_t *weights,
                                                                const NtNet net_arg, float scale, float gamma, u32 *chain,
                                                                uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len,
                                                                int64_t *score, u32 *live_count) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    __shared__ __align__(8) float leaf[NTS_SLOTS];  // V0 of the children, by slot
    __shared__ uint8_t list[NTS_SLOTS];             // the existing slots, ascending
    const u32 lane = threadIdx.x;
    const u32 i = blockIdx.x;  // the grid is N workgroups: every workgroup has a game
    u32 g, B_total;
    nte_place(i, N, bs, g, B_total);
    NteGame G;  // the same in all 64 lanes
    {
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
#pragma unroll 1
    for (int s = 0; s < n_steps; ++s) {
        if (__builtin_amdgcn_readfirstlane((int)G.done)) break;  // the game is replicated: all lanes hold lane 0's flag
        // 1 existence
        Board child;
        const bool e0 = nts_child(G.bd, lane, child), e1 = nts_child(G.bd, lane + NTSE_WAVE, child);
        const uint64_t lo = __ballot(e0), hi = __ballot(e1);
        const u32 n_live = ntse_popc64(lo) + ntse_popc64(hi);  // (scalar)
        if (e0) list[ntse_rank(lo, hi, lane)] = (uint8_t)lane;
        if (e1) list[ntse_rank(lo, hi, lane + NTSE_WAVE)] = (uint8_t)(lane + NTSE_WAVE);
        // workgroup-uniform: the workgroup is this one wave, and the loop exit above is taken by all of its lanes or by none
        __syncthreads();
        // 2 leaf
        const u32 rounds = ntse_rounds(n_live);  // (scalar)
#pragma unroll 1
        for (u32 round = 0; round < rounds; ++round) {
            const u32 p = round * NTSE_WAVE + lane;
            u32 slot;
            bool legal;
            const float q = ntse_leaf_pair<M>(weights, net, scale, G.bd, list, n_live, p, slot, legal);
            const float v0 = quad_best(q, legal);  // every lane of the wave gets here: the trip count is scalar
            if ((p & 3u) == 0 && (p >> 2) < n_live) leaf[slot] = v0;
        }
        // workgroup-uniform, as above: `rounds` comes from the ballots, the same number in every lane
        __syncthreads();
        // 3 choose
        float x = -3.40282347e38f;
        if (lane < 4) {  // one whole quad
            bool legal;
            x = ntse_logit(nts_reduce_lane(G.bd, lane, leaf, gamma, legal), G.mask, lane);
        }
        u32 act = lane & 3u;
        quad_argmax_round<0xB1>(x, act);
        quad_argmax_round<0x4E>(x, act);
        act = (u32)__builtin_amdgcn_readfirstlane((int)act);  // quad 0's choice to the wave
        // 4 step.  The next step's list writes follow this step's last list read by a barrier, its leaf writes follow this step's
        // leaf reads by the next step's first barrier.
        nte_step<MODE>(G, act, B_total, g);
    }
    if (lane == 0) {
        chain[2 * i] = G.c0;
        chain[2 * i + 1] = G.c1;
        store_board(boards, i, G.bd);
        masks[i] = (uint8_t)G.mask;
        done[i] = (uint8_t)G.done;
        ep_len[i] = (int32_t)G.len;
        score[i] = G.score;
        if (live_count && G.done == 0) atomicAdd(live_count, 1u);  // once per live game per launch
    }
}

inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NTSE_LAUNCH_M(MODE, STAGED, m, n, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 1, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 2, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 3, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 4, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 5, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 6, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 7, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((k_nt_search_episodes<MODE, 8, STAGED>), dim3((unsigned)(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read: a single stage launches the kernel without stage work
#define G2048_NTSE_LAUNCH(MODE, m, n, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NTSE_LAUNCH_M(MODE, true, m, n, stream, __VA_ARGS__) \
    } else { \
        G2048_NTSE_LAUNCH_M(MODE, false, m, n, stream, __VA_ARGS__) \
    }

extern "C" {

int g2048_ntuple_staged_search_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights,
                                        const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles, int n_stages, int frac_bits,
                                        int plies, float gamma, uint32_t *chain, uint8_t *boards, uint8_t *masks, uint8_t *done,
                                        int32_t *ep_len, int64_t *score, int rng_mode, uint32_t *live_count, void *stream) {
    NtNet net;
    if (!weights || !chain || !boards || !masks || !done || !ep_len || !score || N < 1 || N > kMaxGames || bs < 1 || bs > kMaxBatch ||
        n_steps < 1 || n_steps > kMaxSteps || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) ||
        plies != 1 || !(gamma >= 0.0f) || !isfinite(gamma) || (rng_mode != G2048_RNG_LEGACY && rng_mode != G2048_RNG_PARTITIONABLE))
        return G2048_EINVAL;
    if (!aligned16(boards) || !aligned8(score) || !aligned4(chain) || !aligned4(ep_len) || !aligned4(weights) || !aligned4(live_count))
        return G2048_EINVAL;
    const int st = start != 0;
    const float scale = nt_scale(frac_bits);
    if (rng_mode) {
        G2048_NTSE_LAUNCH(1, m, N, stream, st, n_steps, (u32)N, (u32)bs, weights, net, scale, gamma, chain, boards, masks, done, ep_len,
                          score, live_count);
    } else {
        G2048_NTSE_LAUNCH(0, m, N, stream, st, n_steps, (u32)N, (u32)bs, weights, net, scale, gamma, chain, boards, masks, done, ep_len,
                          score, live_count);
    }
    return launch_status();
}

int g2048_ntuple_search_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights, const uint8_t *tuple_cells, int m,
                                 int L, int frac_bits, int plies, float gamma, uint32_t *chain, uint8_t *boards, uint8_t *masks,
                                 uint8_t *done, int32_t *ep_len, int64_t *score, int rng_mode, uint32_t *live_count, void *stream) {
    return g2048_ntuple_staged_search_episodes(start, n_steps, N, bs, weights, tuple_cells, m, L, nullptr, 1, frac_bits, plies, gamma,
                                               chain, boards, masks, done, ep_len, score, rng_mode, live_count, stream);
}

}  // extern "C"
