// Expectimax over the n-tuple network (include/g2048.h, "n-tuple expectimax"): one or two plies, searched inside the kernel.
//
//   q1      one workgroup of 256 lanes per POSITION, a board whose one-ply Q is wanted: root blockIdx.x for one ply; for two plies
//           the child in slot blockIdx.x & 127 of root blockIdx.x >> 7, rebuilt with one board_move and one OR (a block whose slot
//           does not exist returns before any barrier).  Two rounds of 256 lanes cover the 128 slots x 4 actions of the position:
//           a lane builds its child in registers and scores one move on it (8 m gathers; a lane of an absent slot or an illegal
//           move gathers nothing), the quad takes the max with two quad-permute DPP moves and lane 0 of the quad writes V0(child)
//           to LDS.  After one barrier four lanes, one per action, run the serial reduction over the 16 cells and write q and v
//           (one ply) or V1 of the position to workspace[root * 128 + slot] (two plies).
//   backup  two plies only, one lane per (root, action): the root's move again, the 16 cells ascending, the (tile 2, tile 4) pair of
//           every existing slot as one aligned float2 from the workspace.  A slot that does not exist is never read, so the
//           workspace needs no clearing.
//
// No child buffer, no scan, no host read, no atomics, no scratch: one launch for one ply, two for two, and results that do not
// depend on scheduling.  The per-lane code is g2048_ntuple_search.h, shared with the host build the CPU tests compare against the
// composed numpy restatements.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_search.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxRoots1 = (int64_t)1 << 24;  // one block per root
constexpr int64_t kMaxRoots2 = (int64_t)1 << 20;  // 128 blocks per root stay below 2^27

// x of the lane whose index differs in bit 0 (0xB1 = quad_perm [1,0,3,2]) / bit 1 (0x4E = quad_perm [2,3,0,1])
template <int CTRL>
__device__ __forceinline__ float quad_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// the max over the legal lanes of a quad, +0 if there is none (every lane of the quad must be active)
__device__ __forceinline__ float quad_best(float q, bool legal) {
    float x = legal ? q : nt_neg_inf();
    x = nt_vmax(x, quad_swap<0xB1>(x));
    x = nt_vmax(x, quad_swap<0x4E>(x));
    return x == nt_neg_inf() ? 0.0f : x;
}

// STAGED = false: the threshold count is a compile-time 0 and no stage work is left (g2048_ntuple.h, nt_kernel_net)
template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_q1(const uint8_t *boards, int plies, const int32_t *weights, const NtNet net_arg,
                                                  float scale, float gamma, float *workspace, float *scores, float *values) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    __shared__ __align__(8) float leaf[NTS_SLOTS];
    const u32 tid = threadIdx.x;
    int64_t b = blockIdx.x;
    u32 slot = 0;
    Board pos;
    if (plies == 1) {
        pos = load_board(boards, b);
    } else {
        slot = blockIdx.x & (NTS_SLOTS - 1);
        b = blockIdx.x >> 7;
        if (!nts_child(load_board(boards, b), slot, pos)) return;  // block-uniform, before the barrier
    }
#pragma unroll 1
    for (u32 round = 0; round < 2; ++round) {
        const u32 idx = round * kBlock + tid;
        bool legal;
        const float q = nts_leaf_lane<M>(weights, net, scale, pos, idx >> 2, idx & 3u, legal);
        const float v0 = quad_best(q, legal);  // every lane of a live block gets here
        if ((idx & 3u) == 0) leaf[idx >> 2] = v0;
    }
    __syncthreads();
    if (tid < 4) {  // one whole quad
        bool legal;
        const float q = nts_reduce_lane(pos, tid, leaf, gamma, legal);
        const float v = quad_best(q, legal);
        if (plies == 1) {
            scores[4 * b + tid] = q;
            if (tid == 0) values[b] = v;
        } else if (tid == 0) {
            workspace[b * NTS_SLOTS + slot] = v;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_nt_backup(const uint8_t *boards, int64_t B, const float *workspace, float gamma,
                                                      float *scores, float *values) {
    // every lane stays to the end: the quad moves want whole quads (4 B lanes: the last quad in range is whole too)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < 4 * B;
    bool legal = false;
    float q = 0.0f;
    if (in_range) q = nts_reduce_lane(load_board(boards, i >> 2), (u32)i & 3u, workspace + (i >> 2) * NTS_SLOTS, gamma, legal);
    const float v = quad_best(q, legal);
    if (in_range) {
        scores[i] = q;
        if (((u32)i & 3u) == 0) values[i >> 2] = v;
    }
}

inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NTS_LAUNCH_M(KERNEL, STAGED, m, grid, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((KERNEL<1, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((KERNEL<4, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((KERNEL<5, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((KERNEL<6, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((KERNEL<7, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<8, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read: a single stage launches the kernels without stage work
#define G2048_NTS_LAUNCH(KERNEL, m, grid, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NTS_LAUNCH_M(KERNEL, true, m, grid, stream, __VA_ARGS__) \
    } else { \
        G2048_NTS_LAUNCH_M(KERNEL, false, m, grid, stream, __VA_ARGS__) \
    }

extern "C" {

int64_t g2048_ntuple_expectimax_workspace_floats(int64_t B, int plies) {
    if (plies == 1) return (B < 1 || B > kMaxRoots1) ? -1 : 0;
    if (plies == 2) return (B < 1 || B > kMaxRoots2) ? -1 : NTS_SLOTS * B;
    return -1;
}

int g2048_ntuple_staged_expectimax(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                                   const uint8_t *stage_tiles, int n_stages, int frac_bits, int plies, double gamma, float *workspace,
                                   float *scores, float *values, void *stream) {
    NtNet net;
    if (!boards || !weights || !scores || !values || g2048_ntuple_expectimax_workspace_floats(B, plies) < 0 ||
        (plies == 2 && !workspace) || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) ||
        !(gamma >= 0.0) || !isfinite(gamma))
        return G2048_EINVAL;
    if (!aligned16(boards) || !aligned4(weights) || !aligned4(scores) || !aligned4(values) || !aligned8(workspace)) return G2048_EINVAL;
    const unsigned grid = (unsigned)(plies == 1 ? B : NTS_SLOTS * B);
    G2048_NTS_LAUNCH(k_nt_q1, m, grid, stream, boards, plies, weights, net, nt_scale(frac_bits), (float)gamma, workspace, scores,
                     values);
    if (plies == 2)
        hipLaunchKernelGGL(k_nt_backup, dim3((unsigned)((4 * B + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, boards, B,
                           workspace, (float)gamma, scores, values);
    return launch_status();
}

// the unstaged entry point: one stage, no thresholds
int g2048_ntuple_expectimax(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                            int frac_bits, int plies, double gamma, float *workspace, float *scores, float *values, void *stream) {
    return g2048_ntuple_staged_expectimax(boards, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, plies, gamma, workspace, scores,
                                          values, stream);
}

}  // extern "C"
