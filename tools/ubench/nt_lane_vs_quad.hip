// Micro-benchmark: the two mappings of the n-tuple episode player on the same lane code (csrc/g2048_ntuple_episodes.h) and the same
// games: one quad per game (what k_nt_episodes ships) against one lane per game, whose lane scores the four actions in sequence
// (once as a loop, once unrolled).  Default tuples, random weights, partitionable RNG, batches of 100.  Times one seeding launch of
// n_steps steps (argv[1], default 32: short enough that almost every game is still live) at 1 000 and 100 000 games: HIP events,
// 3 warm-up launches, median of 5 [min, max]; prints one JSON line per (size, variant) and whether the scores equal the quad's.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/ubench/nt_lane_vs_quad tools/ubench/nt_lane_vs_quad.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>

#include "../../2048-ppo-agent_amd/csrc/g2048_ntuple_episodes.h"
using namespace g2048;

constexpr int kBlock = 256;
constexpr int M = 4;

template <int CTRL>
__device__ __forceinline__ u32 quad_swap(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ void quad_round(float &x, u32 &a) {
    const float xo = __uint_as_float(quad_swap<CTRL>(__float_as_uint(x)));
    const u32 ao = quad_swap<CTRL>(a);
    const bool take = nte_beats(xo, ao, x, a);
    x = take ? xo : x;
    a = take ? ao : a;
}

__device__ __forceinline__ void store_game(const NteGame &G, u32 i, u32 *chain, uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len,
                                           int64_t *score) {
    chain[2 * i] = G.c0;
    chain[2 * i + 1] = G.c1;
    store_board(boards, i, G.bd);
    masks[i] = (uint8_t)G.mask;
    done[i] = (uint8_t)G.done;
    ep_len[i] = (int32_t)G.len;
    score[i] = G.score;
}

__global__ void __launch_bounds__(kBlock) k_quad(int n_steps, u32 N, u32 bs, const int32_t *w, const NtNet net, float scale, u32 *chain,
                                                 uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score) {
    const u32 t = blockIdx.x * (u32)kBlock + threadIdx.x, i = t >> 2, a = t & 3u;
    const bool in_range = i < N;
    NteGame G;
    G.bd.r[0] = G.bd.r[1] = G.bd.r[2] = G.bd.r[3] = 0; G.mask = 0xF; G.done = 1; G.len = 0; G.score = 0; G.c0 = G.c1 = 0;
    u32 g = 0, B_total = 1;
    if (in_range) {
        nte_place(i, N, bs, g, B_total);
        nte_seed<1>(G, chain[2 * i], chain[2 * i + 1], B_total, g);
    }
    for (int s = 0; s < n_steps; ++s) {
        if (__all(G.done != 0)) break;
        float x = -3.40282347e38f;
        if (!G.done) x = nte_logit<M>(w, net, scale, G, a);
        u32 act = a;
        quad_round<0xB1>(x, act);
        quad_round<0x4E>(x, act);
        nte_step<1>(G, act, B_total, g);
    }
    if (in_range && a == 0) store_game(G, i, chain, boards, masks, done, ep_len, score);
}

template <bool UNROLL>
__global__ void __launch_bounds__(kBlock) k_lane(int n_steps, u32 N, u32 bs, const int32_t *w, const NtNet net, float scale, u32 *chain,
                                                 uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score) {
    const u32 i = blockIdx.x * (u32)kBlock + threadIdx.x;
    const bool in_range = i < N;
    NteGame G;
    G.bd.r[0] = G.bd.r[1] = G.bd.r[2] = G.bd.r[3] = 0; G.mask = 0xF; G.done = 1; G.len = 0; G.score = 0; G.c0 = G.c1 = 0;
    u32 g = 0, B_total = 1;
    if (in_range) {
        nte_place(i, N, bs, g, B_total);
        nte_seed<1>(G, chain[2 * i], chain[2 * i + 1], B_total, g);
    }
    for (int s = 0; s < n_steps; ++s) {
        if (__all(G.done != 0)) break;
        if (!G.done) {
            float x = nte_logit<M>(w, net, scale, G, 0u);
            u32 act = 0;
            if (UNROLL) {
#pragma unroll
                for (u32 a = 1; a < 4; ++a) {
                    const float xa = nte_logit<M>(w, net, scale, G, a);
                    if (nte_beats(xa, a, x, act)) { x = xa; act = a; }
                }
            } else {
#pragma unroll 1
                for (u32 a = 1; a < 4; ++a) {
                    const float xa = nte_logit<M>(w, net, scale, G, a);
                    if (nte_beats(xa, a, x, act)) { x = xa; act = a; }
                }
            }
            nte_step<1>(G, act, B_total, g);
        }
    }
    if (in_range) store_game(G, i, chain, boards, masks, done, ep_len, score);
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %d at line %d\n", (int)e, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
    const int n_steps = argc > 1 ? atoi(argv[1]) : 32;
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
        for (int variant = 0; variant < 3; ++variant) {
            std::vector<float> ms;
            for (int rep = 0; rep < 8; ++rep) {
                CK(hipMemcpy(chain, hc.data(), 8 * (size_t)N, hipMemcpyHostToDevice));
                hipEvent_t a, b;
                CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
                CK(hipEventRecord(a, 0));
                if (variant == 0)
                    hipLaunchKernelGGL(k_quad, dim3((4 * N + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, n_steps, N, bs, w, net, nt_scale(12), chain,
                                       boards, masks, done, len, score);
                else if (variant == 1)
                    hipLaunchKernelGGL(k_lane<false>, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, n_steps, N, bs, w, net, nt_scale(12), chain, boards,
                                       masks, done, len, score);
                else
                    hipLaunchKernelGGL(k_lane<true>, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, n_steps, N, bs, w, net, nt_scale(12), chain, boards,
                                       masks, done, len, score);
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
                   "\"live_afterwards\": %u, \"scores_equal_quad\": %s}\n",
                   N, n_steps, variant == 0 ? "one quad per game" : (variant == 1 ? "one lane per game, action loop" : "one lane per game, actions unrolled"), ms[2], ms.front(), ms.back(), 1000.0 * ms[2] / n_steps, live,
                   got == ref_score ? "true" : "false");
            fflush(stdout);
        }
        CK(hipFree(chain)); CK(hipFree(boards)); CK(hipFree(masks)); CK(hipFree(done)); CK(hipFree(len)); CK(hipFree(score));
    }
    CK(hipFree(w));
    return 0;
}
