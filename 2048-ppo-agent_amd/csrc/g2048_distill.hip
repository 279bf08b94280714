// Imitation (distillation) loss of one minibatch (include/g2048.h, "imitation update: loss"): forward, the five logged means and
// the gradient w.r.t. the policy logits and the value estimates, and the minibatch gather out of the trainer's ring.
//
//   k_distill_loss     one sample per lane, ceil(M / 256) workgroups of 256: the per-sample code of g2048_distill.h, the stores of
//                      new_logp / dlogits / dvalues, then the workgroup's five sums (wave shuffles, four wave sums through LDS,
//                      added in wave order) to workspace[wg][5] with vector stores.
//   k_distill_finish   one workgroup: lane k < 5 adds the partials of sum k in ascending workgroup order, scales by 1 / M and writes
//                      sums and running.
//
// Imitation minibatches are larger than PPO's 2048, so unlike k_ppo_loss this is not one workgroup.  No floating-point atomics
// and no ticket counter: the order of every addition is fixed by M alone, so two launches on the same inputs give the same bits
// whatever the CU count, and both launches can be captured.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_distill.h"
#include "g2048_host.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;

__global__ void __launch_bounds__(kBlock)
k_distill_loss(const void *__restrict__ logits, int logits_bf16, const void *__restrict__ values, int values_bf16,
               const uint8_t *__restrict__ mask_bits, const float4 *__restrict__ teacher_q, const float *__restrict__ value_target,
               int64_t M, float tau, float c_value, float c_entropy, float *__restrict__ new_logp, void *__restrict__ dlogits,
               void *__restrict__ dvalues, const float *__restrict__ grad_scale, float *__restrict__ workspace) {
    __shared__ float red[DISTILL_NSUM][kWaves];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    float acc[DISTILL_NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < M) {
        // gradients come out multiplied by the loss scale when one is given, as in k_ppo_loss
        const float inv_m = 1.0f / (float)M;
        const float g_m = grad_scale ? inv_m * *grad_scale : inv_m;
        const uint32_t mb = mask_bits ? mask_bits[i] : 0xFu;
        const float4 q4 = teacher_q[i];
        const float q[4] = {q4.x, q4.y, q4.z, q4.w};
        float l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) l[j] = distill_ld(logits, 4 * i + j, logits_bf16);
        const bool has_v = values != nullptr;
        const float v = has_v ? distill_ld(values, i, values_bf16) : 0.0f, vt = has_v ? value_target[i] : 0.0f;
        DistillOut o;
        distill_sample(l, mb, q, has_v, v, vt, tau, c_value, c_entropy, o);
        new_logp[i] = o.new_logp;
#pragma unroll
        for (int j = 0; j < 4; ++j) distill_st(dlogits, 4 * i + j, logits_bf16, o.dz[j] * g_m);
        if (has_v) distill_st(dvalues, i, values_bf16, o.dv * g_m);
#pragma unroll
        for (int k = 0; k < DISTILL_NSUM; ++k) acc[k] = o.term[k];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < DISTILL_NSUM; ++k) {
        float s = acc[k];
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) red[k][w] = s;
    }
    __syncthreads();
    if (threadIdx.x < DISTILL_NSUM) {
        float s = 0.f;
        for (int ww = 0; ww < kWaves; ++ww) s += red[threadIdx.x][ww];
        workspace[(int64_t)blockIdx.x * DISTILL_NSUM + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(64)
k_distill_finish(const float *__restrict__ workspace, int n_wg, int64_t M, float *__restrict__ sums, double *__restrict__ running) {
    if (threadIdx.x >= DISTILL_NSUM) return;
    float s = 0.f;
    for (int g = 0; g < n_wg; ++g) s += workspace[(int64_t)g * DISTILL_NSUM + threadIdx.x];
    const float mean = s * (1.0f / (float)M);
    sums[threadIdx.x] = mean;
    if (running) running[threadIdx.x] += (double)mean;
}

__global__ void __launch_bounds__(kBlock)
k_distill_gather(const int64_t *__restrict__ idx, int64_t M, int64_t N, const uint4 *__restrict__ boards,
                 const uint8_t *__restrict__ masks, const float4 *__restrict__ teacher_q, const float *__restrict__ value_target,
                 uint4 *__restrict__ o_boards, uint8_t *__restrict__ o_masks, float4 *__restrict__ o_q, float *__restrict__ o_vt) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    int64_t s = idx[i];
    s = s < 0 ? 0 : (s >= N ? N - 1 : s);  // never read out of bounds on a bad index
    o_boards[i] = boards[s];
    o_masks[i] = masks[s];
    o_q[i] = teacher_q[s];
    if (value_target) o_vt[i] = value_target[s];
}

inline bool aligned_to(const void *p, uintptr_t a) { return !((uintptr_t)p & (a - 1)); }

}  // namespace

extern "C" {

int64_t g2048_distill_loss_workspace_floats(int64_t M) {
    if (M < 1 || M > G2048_PPO_LOSS_MAX_BATCH) return -1;
    return (M + kBlock - 1) / kBlock * DISTILL_NSUM;
}

int g2048_distill_loss(const void *logits, int logits_bf16, const void *values, int values_bf16, const uint8_t *mask_bits,
                       const float *teacher_q, const float *value_target, int64_t M, float tau, float c_value, float c_entropy,
                       float *new_logp, float *sums, void *dlogits, void *dvalues, const float *grad_scale, double *running,
                       float *workspace, void *stream) {
    if (!logits || !teacher_q || !new_logp || !sums || !dlogits || !workspace || g2048_distill_loss_workspace_floats(M) < 0)
        return G2048_EINVAL;
    if ((values != nullptr) != (value_target != nullptr) || (values != nullptr) != (dvalues != nullptr)) return G2048_EINVAL;
    if (!(tau >= 0.0f) || !isfinite(tau)) return G2048_EINVAL;
    const uintptr_t la = logits_bf16 ? 2 : 4, va = values_bf16 ? 2 : 4;
    if (!aligned16(teacher_q) || !aligned_to(logits, la) || !aligned_to(dlogits, la) || !aligned_to(values, va) ||
        !aligned_to(dvalues, va) || !aligned_to(value_target, 4) || !aligned_to(new_logp, 4) || !aligned_to(sums, 4) ||
        !aligned_to(grad_scale, 4) || !aligned_to(running, 8) || !aligned_to(workspace, 4))
        return G2048_EINVAL;
    const int n_wg = (int)((M + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_distill_loss, dim3((unsigned)n_wg), dim3(kBlock), 0, (hipStream_t)stream, logits, logits_bf16, values,
                       values_bf16, mask_bits, (const float4 *)teacher_q, value_target, M, tau, c_value, c_entropy, new_logp, dlogits,
                       dvalues, grad_scale, workspace);
    hipLaunchKernelGGL(k_distill_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float *)workspace, n_wg, M, sums, running);
    return launch_status();
}

int g2048_distill_gather(const int64_t *idx, int64_t M, int64_t N, const uint8_t *boards, const uint8_t *masks, const float *teacher_q,
                         const float *value_target, uint8_t *o_boards, uint8_t *o_masks, float *o_q, float *o_vt, void *stream) {
    if (!idx || !boards || !masks || !teacher_q || !o_boards || !o_masks || !o_q || M <= 0 || N <= 0 ||
        (value_target != nullptr) != (o_vt != nullptr))
        return G2048_EINVAL;
    if (!aligned16(boards, o_boards, teacher_q, o_q) || !aligned_to(idx, 8) || !aligned_to(value_target, 4) || !aligned_to(o_vt, 4))
        return G2048_EINVAL;
    hipLaunchKernelGGL(k_distill_gather, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, idx, M, N,
                       (const uint4 *)boards, masks, (const float4 *)teacher_q, value_target, (uint4 *)o_boards, o_masks, (float4 *)o_q,
                       o_vt);
    return launch_status();
}

}  // extern "C"
