// Micro-benchmark: the two leaf mappings of the searched n-tuple episode player on the same wave code
// (csrc/g2048_ntuple_search_episodes.h) and the same games, one wavefront per game either way: the PACKED list of existing children
// (what k_nt_search_episodes ships: an existence pass, then ceil(4 n_live / 64) rounds) against the FIXED slots of k_nt_q1 (no
// existence pass, no list, always 8 rounds of 64 (slot, action) pairs).  Default tuples, random weights, partitionable RNG, batches
// of 100, gamma 1.  Times one seeding launch of n_steps steps (argv[1], default 32: short enough that almost every game is still
// live) at 1 000 and 100 000 games: HIP events, 3 warm-up launches, median of 5 [min, max]; prints one JSON line per (size, variant)
// and whether the scores equal the packed mapping's.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/ubench/nt_search_packed_vs_fixed tools/ubench/nt_search_packed_vs_fixed.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>

#include "../../2048-ppo-agent_amd/csrc/g2048_ntuple_search_episodes.h"
using namespace g2048;

constexpr int kBlock = NTSE_WAVE;
constexpr int M = 4;

template <int CTRL>
__device__ __forceinline__ u32 quad_swap(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ float quad_swap_f(float x) { return __uint_as_float(quad_swap<CTRL>(__float_as_uint(x))); }
__device__ __forceinline__ float quad_best(float q, bool legal) {
    float x = legal ? q : nt_neg_inf();
    x = nt_vmax(x, quad_swap_f<0xB1>(x));
    x = nt_vmax(x, quad_swap_f<0x4E>(x));
    return x == nt_neg_inf() ? 0.0f : x;
}
template <int CTRL>
__device__ __forceinline__ void quad_round(float &x, u32 &a) {
    const float xo = quad_swap_f<CTRL>(x);
    const u32 ao = quad_swap<CTRL>(a);
    const bool take = nte_beats(xo, ao, x, a);
    x = take ? xo : x;
    a = take ? ao : a;
}

template <bool PACKED>
__global__ void __launch_bounds__(kBlock) k_search(int n_steps, u32 N, u32 bs, const int32_t *w, const NtNet net, float scale, float gamma,
                                                   u32 *chain, uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len,
                                                   int64_t *score) {
    __shared__ __align__(8) float leaf[NTS_SLOTS];
    __shared__ uint8_t list[NTS_SLOTS];
    const u32 lane = threadIdx.x, i = blockIdx.x;  // the grid is N workgroups of one wave
    u32 g, B_total;
    nte_place(i, N, bs, g, B_total);
    NteGame G;  // the same in all 64 lanes: every branch and barrier below is workgroup-uniform
    nte_seed<1>(G, chain[2 * i], chain[2 * i + 1], B_total, g);
#pragma unroll 1
    for (int s = 0; s < n_steps; ++s) {
        if (__builtin_amdgcn_readfirstlane((int)G.done)) break;
        if (PACKED) {
            Board child;
            const bool e0 = nts_child(G.bd, lane, child), e1 = nts_child(G.bd, lane + NTSE_WAVE, child);
            const uint64_t lo = __ballot(e0), hi = __ballot(e1);
            const u32 n_live = ntse_popc64(lo) + ntse_popc64(hi);
            if (e0) list[ntse_rank(lo, hi, lane)] = (uint8_t)lane;
            if (e1) list[ntse_rank(lo, hi, lane + NTSE_WAVE)] = (uint8_t)(lane + NTSE_WAVE);
            __syncthreads();  // (uniform: one wave, the game replicated)
            const u32 rounds = ntse_rounds(n_live);
#pragma unroll 1
            for (u32 round = 0; round < rounds; ++round) {
                const u32 p = round * NTSE_WAVE + lane;
                u32 slot;
                bool legal;
                const float q = ntse_leaf_pair<M>(w, net, scale, G.bd, list, n_live, p, slot, legal);
                const float v0 = quad_best(q, legal);
                if ((p & 3u) == 0 && (p >> 2) < n_live) leaf[slot] = v0;
            }
        } else {
#pragma unroll 1
            for (u32 round = 0; round < 4u * NTS_SLOTS / NTSE_WAVE; ++round) {
                const u32 idx = round * NTSE_WAVE + lane;
                bool legal;
                const float q = nts_leaf_lane<M>(w, net, scale, G.bd, idx >> 2, idx & 3u, legal);
                const float v0 = quad_best(q, legal);
                if ((idx & 3u) == 0) leaf[idx >> 2] = v0;
            }
        }
        __syncthreads();  // (uniform, as above)
        float x = -3.40282347e38f;
        if (lane < 4) {
            bool legal;
            x = ntse_logit(nts_reduce_lane(G.bd, lane, leaf, gamma, legal), G.mask, lane);
        }
        u32 act = lane & 3u;
        quad_round<0xB1>(x, act);
        quad_round<0x4E>(x, act);
        act = (u32)__builtin_amdgcn_readfirstlane((int)act);
        if (!PACKED) __syncthreads();  // (uniform) the fixed slots have no other barrier between this step's leaf reads and the next step's writes
        nte_step<1>(G, act, B_total, g);
    }
    if (lane == 0) {
        chain[2 * i] = G.c0;
        chain[2 * i + 1] = G.c1;
        store_board(boards, i, G.bd);
        masks[i] = (uint8_t)G.mask;
        done[i] = (uint8_t)G.done;
        ep_len[i] = (int32_t)G.len;
        score[i] = G.score;
    }
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %d at line %d\n", (int)e, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
    const int n_steps = argc > 1 ? atoi(argv[1]) : 32;
    if (n_steps < 1 || n_steps > 65536) { printf("n_steps must be in 1 .. 65536\n"); return 1; }
    const uint8_t cells[4][6] = {{0, 1, 2, 3, 4, 5}, {4, 5, 6, 7, 8, 9}, {0, 1, 2, 4, 5, 6}, {4, 5, 6, 8, 9, 10}};
    NtNet net;
    memset(&net, 0, sizeof(net));
    net.L = 6;
    for (int t = 0; t < 4; ++t) for (int j = 0; j < 6; ++j) net.cell[t][j] = cells[t][j];
    const size_t E = (size_t)4 << 24;
    std::vector<int32_t> hw(E);
    uint32_t r = 12345u;
    for (auto &x : hw) x = (int32_t)((r = r * 1664525u + 1013904223u) >> 11) - (1 << 20);
    int32_t *w;
    CK(hipMalloc(&w, E * 4));
    CK(hipMemcpy(w, hw.data(), E * 4, hipMemcpyHostToDevice));
    const u32 sizes[2] = {1000u, 100000u};
    for (int k = 0; k < 2; ++k) {
        const u32 N = sizes[k], bs = 100;
        std::vector<u32> hc(2 * (size_t)N);
        for (u32 i = 0; i < N; ++i) { hc[2 * i] = 0; hc[2 * i + 1] = 42u + (i / bs) * bs; }
        u32 *chain; uint8_t *boards, *masks, *done; int32_t *len; int64_t *score;
        CK(hipMalloc(&chain, 8 * (size_t)N)); CK(hipMalloc(&boards, 16 * (size_t)N)); CK(hipMalloc(&masks, N)); CK(hipMalloc(&done, N));
        CK(hipMalloc(&len, 4 * (size_t)N)); CK(hipMalloc(&score, 8 * (size_t)N));
        std::vector<int64_t> ref_score(N), got(N);
        std::vector<uint8_t> hd(N);
        for (int variant = 0; variant < 2; ++variant) {
            std::vector<float> ms;
            for (int rep = 0; rep < 8; ++rep) {
                CK(hipMemcpy(chain, hc.data(), 8 * (size_t)N, hipMemcpyHostToDevice));
                hipEvent_t a, b;
                CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
                CK(hipEventRecord(a, 0));
                if (variant == 0)
                    hipLaunchKernelGGL(k_search<true>, dim3(N), dim3(kBlock), 0, 0, n_steps, N, bs, w, net, nt_scale(12), 1.0f, chain, boards, masks,
                                       done, len, score);
                else
                    hipLaunchKernelGGL(k_search<false>, dim3(N), dim3(kBlock), 0, 0, n_steps, N, bs, w, net, nt_scale(12), 1.0f, chain, boards, masks,
                                       done, len, score);
                CK(hipEventRecord(b, 0));
                CK(hipEventSynchronize(b));
                CK(hipGetLastError());
                float t;
                CK(hipEventElapsedTime(&t, a, b));
                if (rep >= 3) ms.push_back(t);
                CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
            }
            std::sort(ms.begin(), ms.end());
            CK(hipMemcpy(got.data(), score, 8 * (size_t)N, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hd.data(), done, N, hipMemcpyDeviceToHost));
            u32 live = 0;
            for (u32 i = 0; i < N; ++i) live += hd[i] == 0;
            if (variant == 0) ref_score = got;
            printf("{\"games\": %u, \"n_steps\": %d, \"variant\": \"%s\", \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"us_per_step\": %.3f, "
                   "\"live_afterwards\": %u, \"scores_equal_packed\": %s}\n",
                   N, n_steps, variant == 0 ? "packed list of existing children" : "fixed slots, 8 rounds", ms[2], ms.front(), ms.back(),
                   1000.0 * ms[2] / n_steps, live, got == ref_score ? "true" : "false");
            fflush(stdout);
        }
        CK(hipFree(chain)); CK(hipFree(boards)); CK(hipFree(masks)); CK(hipFree(done)); CK(hipFree(len)); CK(hipFree(score));
    }
    CK(hipFree(w));
    return 0;
}
