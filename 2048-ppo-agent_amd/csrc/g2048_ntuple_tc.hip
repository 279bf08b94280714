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

template <int M>
__global__ void __launch_bounds__(kBlock) k_nt_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target,
                                                             int64_t B, const int32_t *weights, const NtNet net, float scale,
                                                             float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                                                             float *td_error) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const u32 f = flag[b];
    float e = 0.0f;
    if (f) e = nt_tc_accumulate_lane<M>(load_board(prev_after, b), f, target[b], weights, net, scale, c, acc, abs_acc, cnt);
    if (td_error) td_error[b] = e;
}

template <int M>
__global__ void __launch_bounds__(kBlock) k_nt_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const NtNet net,
                                                        int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                                                        int32_t *coh_e, int32_t *coh_a) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B || !flag[b]) return;
    nt_tc_apply_lane<M>(load_board(prev_after, b), net, weights, acc, abs_acc, cnt, coh_e, coh_a);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

// the shape of the network, checked and copied into the kernarg struct: m in 1 .. 8, L in 1 .. 6, cells < 16, distinct in a tuple
bool read_net(const uint8_t *tuple_cells, int m, int L, NtNet &net) {
    if (!tuple_cells || m < 1 || m > NT_MAX_TUPLES || L < 1 || L > NT_MAX_CELLS) return false;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t) {
        unsigned seen = 0;
        for (int j = 0; j < L; ++j) {
            const uint8_t c = tuple_cells[t * L + j];
            if (c > 15 || ((seen >> c) & 1u)) return false;
            seen |= 1u << c;
            net.cell[t][j] = c;
        }
    }
    return true;
}

inline bool frac_ok(int frac_bits) { return frac_bits >= 0 && frac_bits <= NT_MAX_FRAC_BITS; }

}  // namespace

#define G2048_NT_TC_LAUNCH(KERNEL, m, n, stream, ...)                                                                  \
    switch (m) {                                                                                                       \
        case 1: hipLaunchKernelGGL((KERNEL<1>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((KERNEL<4>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((KERNEL<5>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((KERNEL<6>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((KERNEL<7>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<8>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }

extern "C" {

int g2048_ntuple_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B, const int32_t *weights,
                               const uint8_t *tuple_cells, int m, int L, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc,
                               int32_t *cnt, float *td_error, void *stream) {
    NtNet net;
    if (!prev_after || !flag || !target || !weights || !acc || !abs_acc || !cnt || B < 1 || B > kMaxBoards ||
        !read_net(tuple_cells, m, L, net) || !frac_ok(frac_bits) || !(alpha > 0.0) || !isfinite(alpha))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(target) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) || !aligned4(cnt) ||
        !aligned4(td_error))
        return G2048_EINVAL;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));
    G2048_NT_TC_LAUNCH(k_nt_tc_accumulate, m, B, stream, prev_after, flag, target, B, weights, net, nt_scale(frac_bits), c, acc,
                       abs_acc, cnt, td_error);
    return launch_status();
}

int g2048_ntuple_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells, int m, int L,
                          int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a,
                          void *stream) {
    NtNet net;
    if (!prev_after || !flag || !weights || !acc || !abs_acc || !cnt || !coh_e || !coh_a || B < 1 || B > kMaxBoards ||
        !read_net(tuple_cells, m, L, net))
        return G2048_EINVAL;
    if (!aligned16(prev_after) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) || !aligned4(cnt) || !aligned4(coh_e) ||
        !aligned4(coh_a))
        return G2048_EINVAL;
    G2048_NT_TC_LAUNCH(k_nt_tc_apply, m, B, stream, prev_after, flag, B, net, weights, acc, abs_acc, cnt, coh_e, coh_a);
    return launch_status();
}

}  // extern "C"
