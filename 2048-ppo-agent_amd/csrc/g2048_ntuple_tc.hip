// Temporal-coherence (TC) learning on the n-tuple network (include/g2048.h, "n-tuple TC learning"): the pair of launches that takes
// the place of td_accumulate / td_apply in a lock-step.
//
//   tc_accumulate  one lane per env: 8 m gathers for V(prev_after), then 8 m x (two 64-bit and one 32-bit) integer atomic adds
//                  (acc += delta, abs_acc += |delta|, cnt += 1).
//   tc_apply       one lane per env over the same entries: cnt is exchanged for 0, the one lane that finds cnt > 0 owns the
//                  entry and updates weights, acc, abs_acc, coh_e and coh_a with plain accesses.  The kernel boundary orders it
//                  after the atomics; no table is ever scanned.
//
// Both are atomic-bound like the TD(0) pair.  The per-lane code is g2048_ntuple_tc.h, shared with the host build the CPU tests
// compare against the numpy restatement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_tc.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 28;

// STAGED = false: the threshold count is a compile-time 0 and no stage work is left (g2048_ntuple.h, nt_kernel_net)
template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target,
                                                             int64_t B, const int32_t *weights, const NtNet net_arg, float scale,
                                                             float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                                                             float *td_error) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const u32 f = flag[b];
    float e = 0.0f;
    if (f) e = nt_tc_accumulate_lane<M>(load_board(prev_after, b), f, target[b], weights, net, scale, c, acc, abs_acc, cnt);
    if (td_error) td_error[b] = e;
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_nt_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const NtNet net_arg,
                                                        int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                                                        int32_t *coh_e, int32_t *coh_a) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B || !flag[b]) return;
    nt_tc_apply_lane<M>(load_board(prev_after, b), net, weights, acc, abs_acc, cnt, coh_e, coh_a);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NT_TC_LAUNCH_M(KERNEL, STAGED, m, n, stream, ...) \
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
#define G2048_NT_TC_LAUNCH(KERNEL, m, n, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NT_TC_LAUNCH_M(KERNEL, true, m, n, stream, __VA_ARGS__) \
    } else { \
        G2048_NT_TC_LAUNCH_M(KERNEL, false, m, n, stream, __VA_ARGS__) \
    }

extern "C" {

// The staged entry points hold the one body of each half; the unstaged ones are calls of them with (NULL, 1).

int g2048_ntuple_staged_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                                      const int32_t *weights, const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles,
                                      int n_stages, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                                      float *td_error, void *stream) {
    NtNet net;
    if (!prev_after || !flag || !target || !weights || !acc || !abs_acc || !cnt || B < 1 || B > kMaxBoards ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) || !(alpha > 0.0) || !isfinite(alpha))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(target) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) || !aligned4(cnt) ||
        !aligned4(td_error))
        return G2048_EINVAL;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));
    G2048_NT_TC_LAUNCH(k_nt_tc_accumulate, m, B, stream, prev_after, flag, target, B, weights, net, nt_scale(frac_bits), c, acc,
                       abs_acc, cnt, td_error);
    return launch_status();
}

int g2048_ntuple_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B, const int32_t *weights,
                               const uint8_t *tuple_cells, int m, int L, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc,
                               int32_t *cnt, float *td_error, void *stream) {
    return g2048_ntuple_staged_tc_accumulate(prev_after, flag, target, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, alpha, acc,
                                             abs_acc, cnt, td_error, stream);
}

int g2048_ntuple_staged_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells, int m, int L,
                                 const uint8_t *stage_tiles, int n_stages, int32_t *weights, int64_t *acc, int64_t *abs_acc,
                                 int32_t *cnt, int32_t *coh_e, int32_t *coh_a, void *stream) {
    NtNet net;
    if (!prev_after || !flag || !weights || !acc || !abs_acc || !cnt || !coh_e || !coh_a || B < 1 || B > kMaxBoards ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) || !aligned4(cnt) || !aligned4(coh_e) ||
        !aligned4(coh_a))
        return G2048_EINVAL;
    G2048_NT_TC_LAUNCH(k_nt_tc_apply, m, B, stream, prev_after, flag, B, net, weights, acc, abs_acc, cnt, coh_e, coh_a);
    return launch_status();
}

int g2048_ntuple_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells, int m, int L,
                          int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a,
                          void *stream) {
    return g2048_ntuple_staged_tc_apply(prev_after, flag, B, tuple_cells, m, L, nullptr, 1, weights, acc, abs_acc, cnt, coh_e, coh_a,
                                        stream);
}

}  // extern "C"
