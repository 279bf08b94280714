// Delayed TD(lambda) / TC(lambda) on the n-tuple network (include/g2048.h, "n-tuple delayed TD(lambda)"): the three launches that
// take the place of td_accumulate / td_apply (or the TC pair) and link in a lock-step.
//
//   delayed_accumulate  one lane per env: 8 m gathers for V of the newest afterstate in the ring, the lambda-sums over the env's
//                       ring of errors, then per DUE state one 16-byte board load, 8 m offsets and the integer atomic adds of
//                       TD(0) (or TC).  In the steady state one state per env is due: the atomic volume is TD(0)'s.
//   delayed_apply       one lane per env over the entries of the same due states: cnt is exchanged for 0 and the one lane that
//                       finds cnt > 0 owns the entry, as in td_apply / tc_apply.
//   delayed_link        one lane per env: the move of the trajectory row replayed, the afterstate stored to prev_after and to
//                       its ring slot, hist_len advanced (restarted after an episode end).
//
// No LDS, no scratch.  The per-lane code is g2048_ntuple_delayed.h, shared with the host build the CPU tests compare against
// the numpy restatement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_delayed.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 28;  // h B <= 2^31 boards: 64-bit byte offsets throughout

// a ring length that does not fit the ring (only garbage could hold one) must not take a slot index out of it
__device__ __forceinline__ int ring_len(const uint8_t *hist_len, int64_t b, int h) {
    const int len = hist_len[b];
    return len < h ? len : h;
}

// STAGED = false: the threshold count is a compile-time 0 and no stage work is left (g2048_ntuple.h, nt_kernel_net)
template <int M, bool STAGED, bool TC>
__global__ void __launch_bounds__(kBlock) k_nt_dl_accumulate(const uint8_t *hist, float *hist_err, const uint8_t *hist_len,
                                                             const uint8_t *flag, const float *target, int64_t B, int h, int head,
                                                             float lam, const int32_t *weights, const NtNet net_arg, float scale,
                                                             float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt, float *td_error) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const u32 f = flag[b];
    float e = 0.0f;
    if (f)
        e = nt_dl_accumulate_lane<M, TC>(hist, hist_err, b, B, h, head, ring_len(hist_len, b, h), f, target[b], lam, weights, net, scale,
                                         c, acc, abs_acc, cnt);
    if (td_error) td_error[b] = e;
}

template <int M, bool STAGED, bool TC>
__global__ void __launch_bounds__(kBlock) k_nt_dl_apply(const uint8_t *hist, const uint8_t *hist_len, const uint8_t *flag, int64_t B,
                                                        int h, int head, const NtNet net_arg, int32_t *weights, int64_t *acc,
                                                        int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const u32 f = flag[b];
    if (!f) return;
    nt_dl_apply_lane<M, TC>(hist, b, B, h, head, ring_len(hist_len, b, h), f, net, weights, acc, abs_acc, cnt, coh_e, coh_a);
}

__global__ void __launch_bounds__(kBlock) k_nt_dl_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B, int h,
                                                       int slot, uint8_t *prev_after, uint8_t *flag, uint8_t *hist,
                                                       uint8_t *hist_len) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    Board bd = load_board(tr_boards_row, b);
    u32 f;
    const u32 len = nt_dl_link_lane(bd, tr_meta_row[b], flag[b], hist_len[b], h, f);
    flag[b] = (uint8_t)f;
    hist_len[b] = (uint8_t)len;
    store_board(prev_after, b, bd);
    store_board(hist, (int64_t)slot * B + b, bd);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }
inline bool aligned8(const void *p) { return !((uintptr_t)p & 7); }

}  // namespace

#define G2048_NT_DL_LAUNCH_M(KERNEL, STAGED, TC, m, n, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((KERNEL<1, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((KERNEL<4, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((KERNEL<5, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((KERNEL<6, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((KERNEL<7, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<8, STAGED, TC>), dim3(blocks_for(n)), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read, `tc` whether the TC tables were given
#define G2048_NT_DL_LAUNCH(KERNEL, m, n, stream, ...) \
    if (net.n_stage_tiles) { \
        if (tc) { \
            G2048_NT_DL_LAUNCH_M(KERNEL, true, true, m, n, stream, __VA_ARGS__) \
        } else { \
            G2048_NT_DL_LAUNCH_M(KERNEL, true, false, m, n, stream, __VA_ARGS__) \
        } \
    } else if (tc) { \
        G2048_NT_DL_LAUNCH_M(KERNEL, false, true, m, n, stream, __VA_ARGS__) \
    } else { \
        G2048_NT_DL_LAUNCH_M(KERNEL, false, false, m, n, stream, __VA_ARGS__) \
    }

extern "C" {

int g2048_ntuple_delayed_accumulate(const uint8_t *hist, float *hist_err, const uint8_t *hist_len, const uint8_t *flag,
                                    const float *target, int64_t B, int h, int head, double lam, const int32_t *weights,
                                    const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles, int n_stages, int frac_bits,
                                    double alpha, int64_t *acc, int64_t *abs_acc, int32_t *cnt, float *td_error, void *stream) {
    NtNet net;
    if (!hist || !hist_err || !hist_len || !flag || !target || !weights || !acc || !cnt || B < 1 || B > kMaxBoards ||
        !nt_dl_ring_ok(h, head) || !(lam >= 0.0 && lam <= 1.0) || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) ||
        !nt_frac_ok(frac_bits) || !(alpha > 0.0) || !isfinite(alpha))
        return G2048_EINVAL;
    if (!aligned16(hist) || !aligned4(hist_err) || !aligned4(target) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) ||
        !aligned4(cnt) || !aligned4(td_error))
        return G2048_EINVAL;
    const bool tc = abs_acc != nullptr;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));
    G2048_NT_DL_LAUNCH(k_nt_dl_accumulate, m, B, stream, hist, hist_err, hist_len, flag, target, B, h, head, (float)lam, weights, net,
                       nt_scale(frac_bits), c, acc, abs_acc, cnt, td_error);
    return launch_status();
}

int g2048_ntuple_delayed_apply(const uint8_t *hist, const uint8_t *hist_len, const uint8_t *flag, int64_t B, int h, int head,
                               const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles, int n_stages, int32_t *weights,
                               int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a, void *stream) {
    NtNet net;
    const int n_tc = (abs_acc != nullptr) + (coh_e != nullptr) + (coh_a != nullptr);
    if (!hist || !hist_len || !flag || !weights || !acc || !cnt || (n_tc != 0 && n_tc != 3) || B < 1 || B > kMaxBoards ||
        !nt_dl_ring_ok(h, head) || !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net))
        return G2048_EINVAL;
    if (!aligned16(hist) || !aligned4(weights) || !aligned8(acc) || !aligned8(abs_acc) || !aligned4(cnt) || !aligned4(coh_e) ||
        !aligned4(coh_a))
        return G2048_EINVAL;
    const bool tc = n_tc == 3;
    G2048_NT_DL_LAUNCH(k_nt_dl_apply, m, B, stream, hist, hist_len, flag, B, h, head, net, weights, acc, abs_acc, cnt, coh_e, coh_a);
    return launch_status();
}

int g2048_ntuple_delayed_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B, int h, int slot,
                              uint8_t *prev_after, uint8_t *flag, uint8_t *hist, uint8_t *hist_len, void *stream) {
    if (!tr_boards_row || !tr_meta_row || !prev_after || !flag || !hist || !hist_len || B < 1 || B > kMaxBoards ||
        !nt_dl_ring_ok(h, slot))
        return G2048_EINVAL;
    if (!aligned16(tr_boards_row, prev_after, hist)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_nt_dl_link, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, tr_boards_row, tr_meta_row, B, h, slot,
                       prev_after, flag, hist, hist_len);
    return launch_status();
}

}  // extern "C"
