// N-tuple afterstate value network (include/g2048.h, "n-tuple network"): evaluation, the player's scores and TD(0) learning.
//
//   values         one lane per board: 8 m gathers, one f32 out.
//   scores         one lane per (board, action) pair: the four lanes of a board load the same 16 bytes, move, gather the
//                  afterstate's 8 m entries (a lane of an illegal move gathers nothing) and take the max over the legal ones
//                  with two quad-permute DPP moves.  No LDS.
//   td_accumulate  one lane per env: 8 m gathers for V(prev_after), then 8 m pairs of integer atomics (acc += delta, cnt += 1).
//   td_apply       one lane per env over the same entries: cnt is exchanged for 0, the one lane that finds cnt > 0 owns the
//                  entry and updates it with plain accesses.  The kernel boundary orders it after the atomics; the 16^L table is
//                  never scanned.
//   link           one lane per env: the move of the trajectory row replayed, 16 B in, 17 B out.
//
// A multi-stage network (g2048_ntuple_staged_*: one [m][16^L] table set per max-tile stage) runs the same kernels: the stage of
// the board that is looked up enters the offsets in nt_offsets (g2048_ntuple.h) and nowhere here.  The unstaged entry points are
// the staged ones with one stage.
//
// All of them are gather- or atomic-bound: every table access is a random 4- or 8-byte access that costs a cache line.
// The per-lane code is g2048_ntuple.h, shared with the host build the CPU tests compare against the numpy restatement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 28;  // 4 lanes per board stay below 2^31

// Every kernel exists once per (M, STAGED).  STAGED = false makes the threshold count a compile-time 0: the branch of nt_offsets
// and the whole max-tile computation fold away, so the kernels of a single-stage network do no stage work at all.
template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_values(const uint8_t *boards, int64_t n, const int32_t *weights, const NtNet net_arg,
                                                      float scale, float *values) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    values[i] = nt_value(nt_sum<M>(weights, net, load_board(boards, i)), scale);
}

// x of the lane whose index differs in bit 0 (0xB1 = quad_perm [1,0,3,2]) / bit 1 (0x4E = quad_perm [2,3,0,1])
template <int CTRL>
__device__ __forceinline__ float quad_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_scores(const uint8_t *boards, int64_t B, const int32_t *weights, const NtNet net_arg,
                                                      float scale, float *scores, float *values) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    // every lane stays to the end: the quad moves below want whole quads (4 B lanes: the last quad in range is whole too)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < 4 * B;
    const u32 a = (u32)i & 3u;
    bool legal = false;
    float q = 0.0f;
    if (in_range) q = nt_score<M>(weights, net, scale, load_board(boards, i >> 2), a, legal);
    float x = legal ? q : nt_neg_inf();
    x = nt_vmax(x, quad_swap<0xB1>(x));
    x = nt_vmax(x, quad_swap<0x4E>(x));
    if (in_range) {
        scores[i] = q;
        if (a == 0) values[i >> 2] = x == nt_neg_inf() ? 0.0f : x;
    }
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_td_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target,
                                                             int64_t B, const int32_t *weights, const NtNet net_arg, float scale,
                                                             float c, int64_t *acc, int32_t *cnt, float *td_error) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const u32 f = flag[b];
    float e = 0.0f;
    if (f) e = nt_td_accumulate_lane<M>(load_board(prev_after, b), f, target[b], weights, net, scale, c, acc, cnt);
    if (td_error) td_error[b] = e;
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_td_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const NtNet net_arg,
                                                        int32_t *weights, int64_t *acc, int32_t *cnt) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B || !flag[b]) return;
    nt_td_apply_lane<M>(load_board(prev_after, b), net, weights, acc, cnt);
}

__global__ void __launch_bounds__(kBlock) k_nt_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B,
                                                    uint8_t *prev_after, uint8_t *flag) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    Board bd = load_board(tr_boards_row, b);
    flag[b] = (uint8_t)nt_link_lane(bd, tr_meta_row[b]);
    store_board(prev_after, b, bd);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NT_LAUNCH_M(KERNEL, STAGED, m, n, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((KERNEL<1, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((KERNEL<4, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((KERNEL<5, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((KERNEL<6, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((KERNEL<7, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<8, STAGED>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read: a single stage launches the kernels without stage work
#define G2048_NT_LAUNCH(KERNEL, m, n, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NT_LAUNCH_M(KERNEL, true, m, n, stream, __VA_ARGS__) \
    } else { \
        G2048_NT_LAUNCH_M(KERNEL, false, m, n, stream, __VA_ARGS__) \
    }

extern "C" {

// The staged entry points hold the one body of every operation; the unstaged ones are calls of them with (NULL, 1).

int g2048_ntuple_staged_values(const uint8_t *boards, int64_t n, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                               const uint8_t *stage_tiles, int n_stages, int frac_bits, float *values, void *stream) {
    NtNet net;
    if (!boards || !weights || !values || n < 1 || n > kMaxBoards || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) ||
        !nt_frac_ok(frac_bits))
        return G2048_EINVAL;
    if (!aligned16(boards) || !aligned4(weights) || !aligned4(values)) return G2048_EINVAL;
    G2048_NT_LAUNCH(k_nt_values, m, n, stream, boards, n, weights, net, nt_scale(frac_bits), values);
    return launch_status();
}

int g2048_ntuple_values(const uint8_t *boards, int64_t n, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                        int frac_bits, float *values, void *stream) {
    return g2048_ntuple_staged_values(boards, n, weights, tuple_cells, m, L, nullptr, 1, frac_bits, values, stream);
}

int g2048_ntuple_staged_scores(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                               const uint8_t *stage_tiles, int n_stages, int frac_bits, float *scores, float *values, void *stream) {
    NtNet net;
    if (!boards || !weights || !scores || !values || B < 1 || B > kMaxBoards ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits))
        return G2048_EINVAL;
    if (!aligned16(boards) || !aligned4(weights) || !aligned4(scores) || !aligned4(values)) return G2048_EINVAL;
    G2048_NT_LAUNCH(k_nt_scores, m, 4 * B, stream, boards, B, weights, net, nt_scale(frac_bits), scores, values);
    return launch_status();
}

int g2048_ntuple_scores(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                        int frac_bits, float *scores, float *values, void *stream) {
    return g2048_ntuple_staged_scores(boards, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, scores, values, stream);
}

int g2048_ntuple_staged_td_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                                      const int32_t *weights, const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles,
                                      int n_stages, int frac_bits, double alpha, int64_t *acc, int32_t *cnt, float *td_error,
                                      void *stream) {
    NtNet net;
    if (!prev_after || !flag || !target || !weights || !acc || !cnt || B < 1 || B > kMaxBoards ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) || !(alpha > 0.0) || !isfinite(alpha))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(target) || !aligned4(weights) || !aligned8(acc) || !aligned4(cnt) || !aligned4(td_error))
        return G2048_EINVAL;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));
    G2048_NT_LAUNCH(k_nt_td_accumulate, m, B, stream, prev_after, flag, target, B, weights, net, nt_scale(frac_bits), c, acc, cnt,
                    td_error);
    return launch_status();
}

int g2048_ntuple_td_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B, const int32_t *weights,
                               const uint8_t *tuple_cells, int m, int L, int frac_bits, double alpha, int64_t *acc, int32_t *cnt,
                               float *td_error, void *stream) {
    return g2048_ntuple_staged_td_accumulate(prev_after, flag, target, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, alpha, acc,
                                             cnt, td_error, stream);
}

int g2048_ntuple_staged_td_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells, int m, int L,
                                 const uint8_t *stage_tiles, int n_stages, int32_t *weights, int64_t *acc, int32_t *cnt, void *stream) {
    NtNet net;
    if (!prev_after || !flag || !weights || !acc || !cnt || B < 1 || B > kMaxBoards ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(weights) || !aligned8(acc) || !aligned4(cnt)) return G2048_EINVAL;
    G2048_NT_LAUNCH(k_nt_td_apply, m, B, stream, prev_after, flag, B, net, weights, acc, cnt);
    return launch_status();
}

int g2048_ntuple_td_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells, int m, int L,
                          int32_t *weights, int64_t *acc, int32_t *cnt, void *stream) {
    return g2048_ntuple_staged_td_apply(prev_after, flag, B, tuple_cells, m, L, nullptr, 1, weights, acc, cnt, stream);
}

int g2048_ntuple_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B, uint8_t *prev_after, uint8_t *flag,
                      void *stream) {
    if (!tr_boards_row || !tr_meta_row || !prev_after || !flag || B < 1 || B > kMaxBoards) return G2048_EINVAL;
    if (!aligned16(tr_boards_row, prev_after)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_nt_link, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, tr_boards_row, tr_meta_row, B, prev_after,
                       flag);
    return launch_status();
}

}  // extern "C"
