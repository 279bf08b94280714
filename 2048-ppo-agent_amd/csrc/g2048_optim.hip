// The optimiser step of the PPO update in two launches: gradient-norm clipping, GradScaler bookkeeping and AdamW over all
// parameters at once (reference: src/ppo/ppo_trainer.py:413-434 - scaler.unscale_, clip_grad_norm_, scaler.step(AdamW),
// scaler.update - which PyTorch runs as ~12 multi-tensor launches per minibatch, 0.25 ms of a 3.2 ms minibatch).
//
// Layout: gradients and both moments live in flat f32 buffers (the gradient buffer is the all-reduce bucket of a
// multi-GPU run); the parameters stay where the module owns them.  A chunk table cuts every parameter tensor into pieces of
// at most OPT_CHUNK elements; workgroup b owns chunk b in both kernels, so the summation order of the norm is fixed.
//   k_opt_sqnorm : partial[b] = sum over chunk b of (g * inv_scale)^2 (the UNSCALED gradients, as clip_grad_norm_ sees them after
//                  scaler.unscale_: summing the squares of the still loss-scaled values overflowed f32 once the scale passed ~2^60,
//                  long before torch's own element-wise inf check would skip a step)
//   k_opt_adamw  : every workgroup adds the partials in the same order -> total norm, found_inf, clip factor; then
//                  g' = (g * inv_scale) * clip;  p -= lr*wd*p;  m = lerp(m, g', 1-b1);  v = b2*v + (1-b2)*g'^2;
//                  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)                      (torch's fused AdamW arithmetic)
//                  unless found_inf
//                  workgroup 0 also advances the step counts and the scaler (scale *= backoff on inf, *= growth after
//                  growth_interval clean steps, as scaler.update() does): finish()
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_bits.h"
#include "g2048_host.h"

namespace {

using namespace g2048_bits;
using namespace g2048_host;

constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC = 4;
constexpr int OPT_CHUNK = G2048_OPT_CHUNK;  // elements per workgroup
static_assert(OPT_CHUNK % (OPT_THREADS * OPT_VEC) == 0, "chunk = whole float4 passes");

__device__ __forceinline__ float block_sum(float v, float *lds) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < OPT_THREADS / 64; ++i) s += lds[i];  // same order in every thread
    __syncthreads();
    return s;
}

struct StepArgs {
    g2048_opt_group groups[G2048_OPT_MAX_GROUPS];
    float max_grad_norm;  // <= 0: no clipping
    float growth, backoff;
    int growth_interval;
};

// per-group constants of one step, derived once (by workgroup 0 of k_opt_sqnorm) from the f64 hyper-parameters and the step
// count: the two f64 pow calls of the bias corrections cost microseconds and must not sit in every workgroup of the update
struct Derived { float step_size, inv_bc2_sqrt, lr_wd, w1, b2, w2, eps, inv_scale; };  // inv_scale: of the scaler BEFORE this step's update
static_assert(sizeof(Derived) == 32, "workspace layout");

__global__ void __launch_bounds__(OPT_THREADS)
k_opt_sqnorm(const g2048_opt_chunk *__restrict__ chunks, const float *__restrict__ grads, float *__restrict__ partial, StepArgs A,
             int n_groups, const float *__restrict__ steps, Derived *__restrict__ derived, const float *__restrict__ scale) {
    __shared__ float lds[OPT_THREADS / 64];
    if (blockIdx.x == 0 && threadIdx.x < n_groups) {
        const g2048_opt_group G = A.groups[threadIdx.x];
        const double t = (double)steps[0] + 1.0;  // (all step counts are equal: every parameter steps on every non-skipped call;
                                                    //  FlatAdamWStep.adopt_state asserts it for loaded states)
        const double bc1 = 1.0 - pow(G.beta1, t), bc2 = 1.0 - pow(G.beta2, t);
        Derived d;
        // hyper-parameters arrive as f64 (what torch.optim holds) and are rounded once, after the f64 arithmetic on them
        d.step_size = (float)(G.lr / bc1);
        d.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
        d.lr_wd = (float)(G.lr * G.weight_decay);
        d.w1 = (float)(1.0 - G.beta1);
        d.b2 = (float)G.beta2;
        d.w2 = (float)(1.0 - G.beta2);
        d.eps = (float)G.eps;
        d.inv_scale = scale ? (float)(1.0 / (double)*scale) : 1.f;  // scaler.unscale_: grads *= scale.double().reciprocal().float()
        derived[threadIdx.x] = d;
    }
    const g2048_opt_chunk c = chunks[blockIdx.x];
    const float *g = grads + c.offset;
    const float inv_scale = scale ? (float)(1.0 / (double)*scale) : 1.f;  // scaler.unscale_: grads *= scale.double().reciprocal().float()
    float s = 0.f;
    for (int i = threadIdx.x * OPT_VEC; i < c.n; i += OPT_THREADS * OPT_VEC) {
        if (i + OPT_VEC <= c.n) {
            float4 v = *reinterpret_cast<const float4 *>(g + i);
            v.x *= inv_scale; v.y *= inv_scale; v.z *= inv_scale; v.w *= inv_scale;
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        } else {
            for (int k = i; k < c.n; ++k) s += (g[k] * inv_scale) * (g[k] * inv_scale);
        }
    }
    s = block_sum(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__device__ __forceinline__ void adamw1(float &p, float g, float &m, float &v, float lr_wd, float w1, float b2, float w2,
                                       float step_size, float inv_bc2_sqrt, float eps) {
    p -= lr_wd * p;
    const float d = g - m;
    m = (w1 < 0.5f) ? m + w1 * d : g - d * (1.f - w1);  // at::lerp
    v = b2 * v + w2 * g * g;
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p -= step_size * m / denom;
}

// bf16 shadows of the parameters the update path multiplies with (dense copy and, for the weights whose input gradient is
// computed by our own GEMM, a transposed copy): rewritten here, in the kernel that changes the parameter, instead of by cast
// and transpose kernels in front of every forward
// `tiled`: the transposed copies of this chunk go through LDS (see k_opt_adamw) and is not written here
__device__ __forceinline__ void refresh_shadow(const g2048_opt_chunk &c, int i, float a, float b, float cc, float d, int n, bool tiled,
                                               uint16_t *stage) {
    const float vals[4] = {a, b, cc, d};
    const int64_t e = (int64_t)c.e0 + i;
    if (tiled) {
        for (int q = 0; q < n; ++q) stage[i + q] = (uint16_t)f2bf(vals[q]);
    }
    if (c.shadow_p) {  // fragment-packed copy: 4 consecutive columns of one row are 8 contiguous bytes there as well
        uint16_t *s = reinterpret_cast<uint16_t *>(c.shadow_p);
        const int64_t row = e / c.cols, col = e - row * c.cols;
        if (n == 4 && !(col & 3)) {
            *reinterpret_cast<uint2 *>(s + packed_off(row, col, c.cols)) =
                make_uint2(pack2(a, b), pack2(cc, d));
        } else {
            for (int q = 0; q < n; ++q) {
                const int64_t eq = e + q, rq = eq / c.cols;
                s[packed_off(rq, eq - rq * c.cols, c.cols)] = (uint16_t)f2bf(vals[q]);
            }
        }
    }
    if (c.shadow_tp && !tiled) {
        uint16_t *t = reinterpret_cast<uint16_t *>(c.shadow_tp);
        for (int q = 0; q < n; ++q) {
            const int64_t eq = e + q, rq = eq / c.cols;
            t[packed_off(eq - rq * c.cols, rq, c.rows)] = (uint16_t)f2bf(vals[q]);
        }
    }
    if (c.shadow) {
        uint16_t *s = reinterpret_cast<uint16_t *>(c.shadow) + e;
        if (n == 4 && !((uintptr_t)s & 7)) {
            *reinterpret_cast<uint2 *>(s) = make_uint2(pack2(a, b), pack2(cc, d));
        } else {
            for (int q = 0; q < n; ++q) s[q] = (uint16_t)f2bf(vals[q]);
        }
    }
    if (c.shadow_t && !tiled) {
        uint16_t *t = reinterpret_cast<uint16_t *>(c.shadow_t);
        for (int q = 0; q < n; ++q) {
            const int64_t eq = e + q, r = eq / c.cols, col = eq - r * c.cols;
            t[col * c.rows + r] = (uint16_t)f2bf(vals[q]);
        }
    }
}

// Bookkeeping of one step, by workgroup 0 of k_opt_adamw: step counts, scaler state (scale *= backoff on inf, *= growth after
// growth_interval clean steps, as scaler.update() does), info.  Nothing of the same launch reads what it writes: the step counts are
// read by k_opt_sqnorm only, the scale reaches the other workgroups through Derived.inv_scale.  (Rounds 2-3: a launch of its own,
// k_opt_finish, ~4.5 us of every minibatch.  A "last workgroup done" counter is NOT what this is: that needed a device-scope release
// fence per workgroup, each writing back its XCD's L2 - measured 114 us for the update kernel instead of 20.)
struct FinishArgs {
    float growth, backoff;
    int growth_interval, n_steps;
    float *steps;
    int32_t *growth_tracker;
    float *info;
};
__device__ __forceinline__ void finish(const FinishArgs &F, float total, bool found_inf, float *scale) {
    if (!found_inf)
        for (int i = threadIdx.x; i < F.n_steps; i += OPT_THREADS) F.steps[i] += 1.f;  // one count per parameter, as torch keeps them
    if (threadIdx.x == 0) {
        if (F.info) {
            F.info[0] = sqrtf(total);  // gradient norm (unscaled) before clipping: what clip_grad_norm_ returns
            F.info[1] = found_inf ? 1.f : 0.f;
        }
        if (scale) {
            if (found_inf) {
                *scale *= F.backoff;
                *F.growth_tracker = 0;
            } else {
                const int32_t ok = *F.growth_tracker + 1;
                if (ok == F.growth_interval) {
                    *scale *= F.growth;
                    *F.growth_tracker = 0;
                } else {
                    *F.growth_tracker = ok;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(OPT_THREADS)
k_opt_adamw(const g2048_opt_chunk *__restrict__ chunks, int n_chunks, const float *__restrict__ grads, float *__restrict__ exp_avg,
            float *__restrict__ exp_avg_sq, const float *__restrict__ partial, const Derived *__restrict__ derived, float max_grad_norm,
            float *__restrict__ scale, FinishArgs F) {
    __shared__ float lds[OPT_THREADS / 64];
    __shared__ float sh[2];
    __shared__ uint16_t stage[OPT_CHUNK];
    // total of the partials, identical in every workgroup (fixed order: strided per thread, then the block tree)
    float s = 0.f;
    for (int i = threadIdx.x; i < n_chunks; i += OPT_THREADS) s += partial[i];
    const float total = block_sum(s, lds);
    const g2048_opt_chunk c = chunks[blockIdx.x];
    const Derived G = derived[c.group];
    // Transposed shadow of a full chunk that covers R = 2, 4 or 8 whole rows of a [rows][cols] weight: the chunk's bf16 values
    // are staged in LDS and written as one 2R-byte run per column (R consecutive rows of the [cols][rows] copy) instead of one
    // scattered 2-byte store per element (round 2: 22 -> 30 us for the step with one transposed weight per layer; round 3 adds
    // the transposed copies the fused CLS tail's backward multiplies with)
    const bool any_t = c.shadow_t || c.shadow_tp;
    const int rows_in_chunk = (any_t && c.cols > 0) ? OPT_CHUNK / c.cols : 0;
    const bool tiled = any_t && c.n == OPT_CHUNK && c.cols > 0 && OPT_CHUNK % c.cols == 0 && c.e0 % c.cols == 0 &&
                       (rows_in_chunk == 2 || rows_in_chunk == 4 || rows_in_chunk == 8) && c.rows % rows_in_chunk == 0 &&
                       !(((uintptr_t)c.shadow_t | (uintptr_t)c.shadow_tp) & 15);
    if (threadIdx.x == 0) {
        const float inv_scale = G.inv_scale;  // (of k_opt_sqnorm's making: workgroup 0 below rewrites *scale while others still start)
        // the norm of the unscaled gradients (k_opt_sqnorm squared g * inv_scale); non-finite anywhere makes the total non-finite
        const float norm = sqrtf(total);
        float clip = 1.f;
        if (max_grad_norm > 0.f) {
            clip = max_grad_norm / (norm + 1e-6f);  // torch.nn.utils.clip_grad_norm_
            if (clip > 1.f) clip = 1.f;
        }
        sh[0] = inv_scale;
        sh[1] = clip;
    }
    __syncthreads();
    const bool found_inf = scale != nullptr && !(fabsf(total) <= 3.4028234664e38f);  // inf or nan; without a scaler torch steps anyway
    if (blockIdx.x == 0) finish(F, total, found_inf, scale);
    if (!found_inf) {
        const float inv_scale = sh[0], clip = sh[1], step_size = G.step_size, inv_bc2_sqrt = G.inv_bc2_sqrt;
        const float lr_wd = G.lr_wd, w1 = G.w1, b2 = G.b2, w2 = G.w2, eps = G.eps;
        float *p = c.param;
        const float *g = grads + c.offset;
        float *m = exp_avg + c.offset, *v = exp_avg_sq + c.offset;
        for (int i = threadIdx.x * OPT_VEC; i < c.n; i += OPT_THREADS * OPT_VEC) {
            if (i + OPT_VEC <= c.n) {
                float4 pv = *reinterpret_cast<float4 *>(p + i), mv = *reinterpret_cast<float4 *>(m + i),
                       vv = *reinterpret_cast<float4 *>(v + i);
                const float4 gv = *reinterpret_cast<const float4 *>(g + i);
                adamw1(pv.x, (gv.x * inv_scale) * clip, mv.x, vv.x, lr_wd, w1, b2, w2, step_size, inv_bc2_sqrt, eps);
                adamw1(pv.y, (gv.y * inv_scale) * clip, mv.y, vv.y, lr_wd, w1, b2, w2, step_size, inv_bc2_sqrt, eps);
                adamw1(pv.z, (gv.z * inv_scale) * clip, mv.z, vv.z, lr_wd, w1, b2, w2, step_size, inv_bc2_sqrt, eps);
                adamw1(pv.w, (gv.w * inv_scale) * clip, mv.w, vv.w, lr_wd, w1, b2, w2, step_size, inv_bc2_sqrt, eps);
                *reinterpret_cast<float4 *>(p + i) = pv;
                *reinterpret_cast<float4 *>(m + i) = mv;
                *reinterpret_cast<float4 *>(v + i) = vv;
                if (c.shadow || c.shadow_p || any_t) refresh_shadow(c, i, pv.x, pv.y, pv.z, pv.w, 4, tiled, stage);
            } else {
                for (int k = i; k < c.n; ++k) {
                    float pk = p[k], mk = m[k], vk = v[k];
                    adamw1(pk, (g[k] * inv_scale) * clip, mk, vk, lr_wd, w1, b2, w2, step_size, inv_bc2_sqrt, eps);
                    p[k] = pk; m[k] = mk; v[k] = vk;
                    if (c.shadow || c.shadow_p || any_t) refresh_shadow(c, k, pk, 0.f, 0.f, 0.f, 1, tiled, stage);
                }
            }
        }
        if (tiled) {  // (uniform per workgroup)
            __syncthreads();
            const int R = rows_in_chunk, r0 = c.e0 / c.cols;
            // the run of R consecutive rows of one column: 2R contiguous bytes of the [cols][rows] copy, and (R <= 8, r0 % R == 0)
            // of its fragment-packed form too
            for (int col = threadIdx.x; col < c.cols; col += OPT_THREADS) {
                const uint16_t *src = stage + col;
                const int cs = c.cols;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (R == 8) {
                    for (int q = 0; q < 4; ++q) w[q] = src[2 * q * cs] | ((uint32_t)src[(2 * q + 1) * cs] << 16);
                } else if (R == 4) {
                    for (int q = 0; q < 2; ++q) w[q] = src[2 * q * cs] | ((uint32_t)src[(2 * q + 1) * cs] << 16);
                } else {
                    w[0] = src[0] | ((uint32_t)src[cs] << 16);
                }
                for (int which = 0; which < 2; ++which) {
                    uint16_t *base = reinterpret_cast<uint16_t *>(which ? c.shadow_tp : c.shadow_t);
                    if (!base) continue;
                    uint16_t *dst = base + (which ? packed_off(col, r0, c.rows) : (int64_t)col * c.rows + r0);
                    if (R == 8) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                    else if (R == 4) *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
                    else *reinterpret_cast<uint32_t *>(dst) = w[0];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- LAMB
// g2048_lamb_step: the same update loop with the reference's Lamb optimiser (src/optim/lamb.py:106-209) in three launches over the
// same chunk table.  The trust ratio r = ||p|| / ||u|| needs two norms per TENSOR of an update u that itself depends on the
// global gradient norm, so the step is three dependent launches (workgroup b owns chunk b in all of them):
//   k_lamb_sqnorm  : partial[b] as k_opt_sqnorm, and LAMB's per-group constants
//   k_lamb_moments : total norm, found_inf, c1 = trainer clip, c2 = LAMB's own clip = max(1, norm * c1 / lamb_max_grad_norm);
//                    g' = g * (inv_scale * c1 / c2) (the factor in f64, rounded once);  m = b1*m + b3*g';  v = b2*v + ((1-b2)*g')*g';  u = lamb_update(m, v, p);
//                    pn[b] = sum p^2, un[b] = sum u^2 over the chunk (block_sum's order); p is not touched
//   k_lamb_apply   : a workgroup adds the pn / un of its own tensor's chunks in ascending order (they are adjacent in the table: the
//                    first is blockIdx.x - e0 / OPT_CHUNK, the count follows from rows * cols), r from the two norms, recomputes u
//                    from the stored m, v and the still unchanged p with the same lamb_update, p -= (lr * r) * u, shadows;
//                    workgroup 0 runs finish()
// The reference takes the norm for c2 again from the clipped elements; norm * c1 is that number up to rounding and saves a pass over
// the gradients.  u is recomputed instead of stored: re-reading m and v costs the bytes that writing and reading u would, and needs
// no fourth flat buffer.  The u whose norm is taken and the u that is applied are the same values because both kernels call
// lamb_update, and this file is compiled with -ffp-contract=off, so neither call site can be contracted differently (the ISA of both
// kernels holds v_mul_f32 / v_add_f32 / the IEEE division and square-root sequences for it, no v_fma outside those sequences).
// Not merged into fewer launches for the reason finish() records: no grid-wide barrier, no "last workgroup done" counter.
// The transposed-shadow code of k_opt_adamw is repeated in tiled_chunk / tiled_flush instead of being called by both: moving it
// out of k_opt_adamw changed that kernel's register allocation and schedule (tried; DESIGN 3, "a helper moves only if every kernel's
// device assembly stays byte-identical"), and g2048_opt_step keeps its kernels bit for bit.
struct LambArgs { g2048_lamb_group groups[G2048_OPT_MAX_GROUPS]; };
struct LambDerived { float lr, b1, b3, b2, w2, bc1, bc2_sqrt, eps, wd, inv_scale; int32_t adapt, trust_clip; };
static_assert(sizeof(LambDerived) == 48, "workspace layout");

__global__ void __launch_bounds__(OPT_THREADS)
k_lamb_sqnorm(const g2048_opt_chunk *__restrict__ chunks, const float *__restrict__ grads, float *__restrict__ partial, LambArgs A,
              int n_groups, const float *__restrict__ steps, LambDerived *__restrict__ derived, const float *__restrict__ scale) {
    __shared__ float lds[OPT_THREADS / 64];
    if (blockIdx.x == 0 && threadIdx.x < n_groups) {
        const g2048_lamb_group G = A.groups[threadIdx.x];
        const double t = (double)steps[0] + 1.0;  // one count for all groups (FlatLambStep.adopt_state asserts it for loaded states)
        LambDerived d;
        d.lr = (float)G.lr;
        d.b1 = (float)G.beta1;
        d.b3 = (float)G.beta3;
        d.b2 = (float)G.beta2;
        d.w2 = (float)(1.0 - G.beta2);
        d.bc1 = G.bias_correction ? (float)(1.0 - pow(G.beta1, t)) : 1.f;
        d.bc2_sqrt = G.bias_correction ? (float)sqrt(1.0 - pow(G.beta2, t)) : 1.f;
        d.eps = (float)G.eps;
        d.wd = (float)G.weight_decay;
        d.inv_scale = scale ? (float)(1.0 / (double)*scale) : 1.f;
        d.adapt = G.adapt != 0 || G.weight_decay != 0.0;
        d.trust_clip = G.trust_clip != 0;
        derived[threadIdx.x] = d;
    }
    const g2048_opt_chunk c = chunks[blockIdx.x];
    const float *g = grads + c.offset;
    const float inv_scale = scale ? (float)(1.0 / (double)*scale) : 1.f;  // scaler.unscale_, as k_opt_sqnorm
    float s = 0.f;
    for (int i = threadIdx.x * OPT_VEC; i < c.n; i += OPT_THREADS * OPT_VEC) {
        if (i + OPT_VEC <= c.n) {
            float4 v = *reinterpret_cast<const float4 *>(g + i);
            v.x *= inv_scale; v.y *= inv_scale; v.z *= inv_scale; v.w *= inv_scale;
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        } else {
            for (int k = i; k < c.n; ++k) s += (g[k] * inv_scale) * (g[k] * inv_scale);
        }
    }
    s = block_sum(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// LAMB's update direction of one element from its moments and the parameter (lamb.py: update = (m / denom) / bc1 + wd * p with
// denom = sqrt(v) / sqrt(bc2) + eps).  THE one expression: k_lamb_moments takes its norm, k_lamb_apply applies it.
__device__ __forceinline__ float lamb_update(float m, float v, float p, const LambDerived &G) {
    const float denom = sqrtf(v) / G.bc2_sqrt + G.eps;
    float u = (m / denom) / G.bc1;
    if (G.wd != 0.f) u = u + G.wd * p;
    return u;
}

__device__ __forceinline__ void lamb_moments1(float g, float &m, float &v, const LambDerived &G) {
    m = G.b1 * m + G.b3 * g;
    v = G.b2 * v + (G.w2 * g) * g;  // addcmul: self + value * t1 * t2
}

// flags: f32[2] = {sum of the squared gradients, found_inf}, written by workgroup 0 for k_lamb_apply
__global__ void __launch_bounds__(OPT_THREADS)
k_lamb_moments(const g2048_opt_chunk *__restrict__ chunks, int n_chunks, const float *__restrict__ grads, float *__restrict__ exp_avg,
               float *__restrict__ exp_avg_sq, const float *__restrict__ partial, const LambDerived *__restrict__ derived,
               float max_grad_norm, float lamb_max_grad_norm, int has_scale, float *__restrict__ pn, float *__restrict__ un,
               float *__restrict__ flags) {
    __shared__ float lds[OPT_THREADS / 64];
    float s = 0.f;  // total of the partials, identical in every workgroup (the order of k_opt_adamw)
    for (int i = threadIdx.x; i < n_chunks; i += OPT_THREADS) s += partial[i];
    const float total = block_sum(s, lds);
    const bool found_inf = has_scale && !(fabsf(total) <= 3.4028234664e38f);  // inf or nan; without a scaler torch steps anyway
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        flags[0] = total;
        flags[1] = found_inf ? 1.f : 0.f;
    }
    if (found_inf) return;
    const g2048_opt_chunk c = chunks[blockIdx.x];
    const LambDerived G = derived[c.group];
    // unscale and both clips as ONE factor, formed in f64 from the f32 total and rounded once: g' = g * gfac has two roundings where
    // the reference's three passes over the gradients (unscale_, clip_grad_norm_, Lamb's grads / clip) have five.  (Measured with
    // the three separate f32 factors: the one-element tensor of tests/test_gpu_lamb.py ended 2.2-2.5 ulp from the f64 result.)
    const double norm = sqrt((double)total);
    double c1 = 1.0, c2 = 1.0;
    if (max_grad_norm > 0.f) {
        c1 = (double)max_grad_norm / (norm + 1e-6);  // torch.nn.utils.clip_grad_norm_
        if (c1 > 1.0) c1 = 1.0;
    }
    if (lamb_max_grad_norm > 0.f) {
        c2 = (norm * c1) / (double)lamb_max_grad_norm;  // lamb.py: clip = (gnorm / max_grad_norm).clamp(min=1); grads / clip
        if (c2 < 1.0) c2 = 1.0;
    }
    const float gfac = (float)((double)G.inv_scale * c1 / c2);
    const bool adapt = G.adapt != 0;  // (uniform per workgroup: a chunk belongs to one group)
    const float *p = c.param;
    const float *g = grads + c.offset;
    float *m = exp_avg + c.offset, *v = exp_avg_sq + c.offset;
    float sp = 0.f, su = 0.f;
    for (int i = threadIdx.x * OPT_VEC; i < c.n; i += OPT_THREADS * OPT_VEC) {
        if (i + OPT_VEC <= c.n) {
            float4 mv = *reinterpret_cast<float4 *>(m + i), vv = *reinterpret_cast<float4 *>(v + i);
            const float4 gv = *reinterpret_cast<const float4 *>(g + i);
            lamb_moments1(gv.x * gfac, mv.x, vv.x, G);
            lamb_moments1(gv.y * gfac, mv.y, vv.y, G);
            lamb_moments1(gv.z * gfac, mv.z, vv.z, G);
            lamb_moments1(gv.w * gfac, mv.w, vv.w, G);
            *reinterpret_cast<float4 *>(m + i) = mv;
            *reinterpret_cast<float4 *>(v + i) = vv;
            if (adapt) {
                const float4 pv = *reinterpret_cast<const float4 *>(p + i);
                const float ux = lamb_update(mv.x, vv.x, pv.x, G), uy = lamb_update(mv.y, vv.y, pv.y, G),
                            uz = lamb_update(mv.z, vv.z, pv.z, G), uw = lamb_update(mv.w, vv.w, pv.w, G);
                sp += pv.x * pv.x + pv.y * pv.y + pv.z * pv.z + pv.w * pv.w;
                su += ux * ux + uy * uy + uz * uz + uw * uw;
            }
        } else {
            for (int k = i; k < c.n; ++k) {
                float mk = m[k], vk = v[k];
                lamb_moments1(g[k] * gfac, mk, vk, G);
                m[k] = mk; v[k] = vk;
                if (adapt) {
                    const float pk = p[k], uk = lamb_update(mk, vk, pk, G);
                    sp += pk * pk;
                    su += uk * uk;
                }
            }
        }
    }
    if (adapt) {
        sp = block_sum(sp, lds);
        su = block_sum(su, lds);
        if (threadIdx.x == 0) {
            pn[blockIdx.x] = sp;
            un[blockIdx.x] = su;
        }
    }
}

// whether the transposed copies of chunk c go through LDS, and their write-out: the code of k_opt_adamw (see there and above)
__device__ __forceinline__ bool tiled_chunk(const g2048_opt_chunk &c, bool any_t, int rows_in_chunk) {
    return any_t && c.n == OPT_CHUNK && c.cols > 0 && OPT_CHUNK % c.cols == 0 && c.e0 % c.cols == 0 &&
           (rows_in_chunk == 2 || rows_in_chunk == 4 || rows_in_chunk == 8) && c.rows % rows_in_chunk == 0 &&
           !(((uintptr_t)c.shadow_t | (uintptr_t)c.shadow_tp) & 15);
}
__device__ __forceinline__ void tiled_flush(const g2048_opt_chunk &c, int rows_in_chunk, const uint16_t *stage) {
    __syncthreads();
    const int R = rows_in_chunk, r0 = c.e0 / c.cols;
    for (int col = threadIdx.x; col < c.cols; col += OPT_THREADS) {
        const uint16_t *src = stage + col;
        const int cs = c.cols;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (R == 8) {
            for (int q = 0; q < 4; ++q) w[q] = src[2 * q * cs] | ((uint32_t)src[(2 * q + 1) * cs] << 16);
        } else if (R == 4) {
            for (int q = 0; q < 2; ++q) w[q] = src[2 * q * cs] | ((uint32_t)src[(2 * q + 1) * cs] << 16);
        } else {
            w[0] = src[0] | ((uint32_t)src[cs] << 16);
        }
        for (int which = 0; which < 2; ++which) {
            uint16_t *base = reinterpret_cast<uint16_t *>(which ? c.shadow_tp : c.shadow_t);
            if (!base) continue;
            uint16_t *dst = base + (which ? packed_off(col, r0, c.rows) : (int64_t)col * c.rows + r0);
            if (R == 8) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            else if (R == 4) *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
            else *reinterpret_cast<uint32_t *>(dst) = w[0];
        }
    }
}

__global__ void __launch_bounds__(OPT_THREADS)
k_lamb_apply(const g2048_opt_chunk *__restrict__ chunks, int n_chunks, const float *__restrict__ exp_avg,
             const float *__restrict__ exp_avg_sq, const LambDerived *__restrict__ derived, const float *__restrict__ pn,
             const float *__restrict__ un, const float *__restrict__ flags, float *__restrict__ scale, FinishArgs F) {
    __shared__ uint16_t stage[OPT_CHUNK];
    const float total = flags[0];
    const bool found_inf = flags[1] != 0.f;
    if (blockIdx.x == 0) finish(F, total, found_inf, scale);
    if (found_inf) return;
    const g2048_opt_chunk c = chunks[blockIdx.x];
    const LambDerived G = derived[c.group];
    float r = 1.f;
    if (G.adapt) {
        // the chunks of this tensor, in ascending order (the same order, hence the same r, in every workgroup of the tensor)
        int first = (int)blockIdx.x - c.e0 / OPT_CHUNK;
        int count = (int)(((int64_t)c.rows * c.cols + OPT_CHUNK - 1) / OPT_CHUNK);
        if (first < 0) first = 0;  // (a table that is not laid out as documented must not make this read out of bounds)
        if (count > n_chunks - first) count = n_chunks - first;
        float sp = 0.f, su = 0.f;
        for (int i = 0; i < count; ++i) {
            sp += pn[first + i];
            su += un[first + i];
        }
        const float wn = sqrtf(sp), upd = sqrtf(su);
        if (wn > 0.f && upd > 0.f) r = wn / upd;  // lamb.py: where((wn > 0) & (un > 0), wn / un, 1)
        if (G.trust_clip && r > 1.f) r = 1.f;
    }
    const float step = G.lr * r;
    const bool any_t = c.shadow_t || c.shadow_tp;
    const int rows_in_chunk = (any_t && c.cols > 0) ? OPT_CHUNK / c.cols : 0;
    const bool tiled = tiled_chunk(c, any_t, rows_in_chunk);
    float *p = c.param;
    const float *m = exp_avg + c.offset, *v = exp_avg_sq + c.offset;
    for (int i = threadIdx.x * OPT_VEC; i < c.n; i += OPT_THREADS * OPT_VEC) {
        if (i + OPT_VEC <= c.n) {
            float4 pv = *reinterpret_cast<float4 *>(p + i);
            const float4 mv = *reinterpret_cast<const float4 *>(m + i), vv = *reinterpret_cast<const float4 *>(v + i);
            pv.x -= step * lamb_update(mv.x, vv.x, pv.x, G);
            pv.y -= step * lamb_update(mv.y, vv.y, pv.y, G);
            pv.z -= step * lamb_update(mv.z, vv.z, pv.z, G);
            pv.w -= step * lamb_update(mv.w, vv.w, pv.w, G);
            *reinterpret_cast<float4 *>(p + i) = pv;
            if (c.shadow || c.shadow_p || any_t) refresh_shadow(c, i, pv.x, pv.y, pv.z, pv.w, 4, tiled, stage);
        } else {
            for (int k = i; k < c.n; ++k) {
                float pk = p[k];
                pk -= step * lamb_update(m[k], v[k], pk, G);
                p[k] = pk;
                if (c.shadow || c.shadow_p || any_t) refresh_shadow(c, k, pk, 0.f, 0.f, 0.f, 1, tiled, stage);
            }
        }
    }
    if (tiled) tiled_flush(c, rows_in_chunk, stage);  // (uniform per workgroup)
}

}  // namespace

extern "C" int g2048_opt_step(const g2048_opt_chunk *chunks, int n_chunks, const float *grads, float *exp_avg, float *exp_avg_sq,
                              const g2048_opt_group *groups, int n_groups, float max_grad_norm, float *steps, int n_steps, float *scale,
                              int32_t *growth_tracker, float growth, float backoff, int growth_interval, float *workspace,
                              float *info, void *stream) {
    if (!chunks || n_chunks <= 0 || !grads || !exp_avg || !exp_avg_sq || !groups || n_groups <= 0 ||
        n_groups > G2048_OPT_MAX_GROUPS || !steps || n_steps <= 0 || !workspace || (scale && !growth_tracker) ||
        !aligned16(grads, exp_avg, exp_avg_sq, workspace))
        return G2048_EINVAL;
    StepArgs A;
    for (int i = 0; i < G2048_OPT_MAX_GROUPS; ++i) A.groups[i] = groups[i < n_groups ? i : 0];
    // workspace: [n_chunks] partial sums, then the per-group constants
    float *partial = workspace;
    Derived *derived = reinterpret_cast<Derived *>(workspace + ((n_chunks + 3) & ~3));
    hipLaunchKernelGGL(k_opt_sqnorm, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, chunks, grads, partial, A,
                       n_groups, steps, derived, scale);
    FinishArgs F;
    F.growth = growth, F.backoff = backoff, F.growth_interval = growth_interval, F.n_steps = n_steps;
    F.steps = steps, F.growth_tracker = growth_tracker, F.info = info;
    hipLaunchKernelGGL(k_opt_adamw, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, chunks, n_chunks, grads,
                       exp_avg, exp_avg_sq, partial, derived, max_grad_norm, scale, F);
    return launch_status();
}

extern "C" int64_t g2048_opt_workspace_floats(int n_chunks) {
    return n_chunks <= 0 ? 0 : (int64_t)((n_chunks + 3) & ~3) + G2048_OPT_MAX_GROUPS * (int64_t)(sizeof(Derived) / sizeof(float));
}

// workspace: [nc4] gradient partials, [nc4] sum p^2 per chunk, [nc4] sum u^2 per chunk, f32[4] flags, then the per-group constants
extern "C" int g2048_lamb_step(const g2048_opt_chunk *chunks, int n_chunks, const float *grads, float *exp_avg, float *exp_avg_sq,
                               const g2048_lamb_group *groups, int n_groups, float max_grad_norm, float lamb_max_grad_norm,
                               float *steps, int n_steps, float *scale, int32_t *growth_tracker, float growth, float backoff,
                               int growth_interval, float *workspace, float *info, void *stream) {
    if (!chunks || n_chunks <= 0 || !grads || !exp_avg || !exp_avg_sq || !groups || n_groups <= 0 ||
        n_groups > G2048_OPT_MAX_GROUPS || !steps || n_steps <= 0 || !workspace || (scale && !growth_tracker) ||
        !aligned16(grads, exp_avg, exp_avg_sq, workspace))
        return G2048_EINVAL;
    LambArgs A;
    for (int i = 0; i < G2048_OPT_MAX_GROUPS; ++i) A.groups[i] = groups[i < n_groups ? i : 0];
    const int64_t nc4 = (n_chunks + 3) & ~3;
    float *partial = workspace, *pn = workspace + nc4, *un = workspace + 2 * nc4, *flags = workspace + 3 * nc4;
    LambDerived *derived = reinterpret_cast<LambDerived *>(flags + 4);
    const dim3 grid((unsigned)n_chunks), block(OPT_THREADS);
    hipLaunchKernelGGL(k_lamb_sqnorm, grid, block, 0, (hipStream_t)stream, chunks, grads, partial, A, n_groups, steps, derived, scale);
    hipLaunchKernelGGL(k_lamb_moments, grid, block, 0, (hipStream_t)stream, chunks, n_chunks, grads, exp_avg, exp_avg_sq, partial,
                       derived, max_grad_norm, lamb_max_grad_norm, scale ? 1 : 0, pn, un, flags);
    FinishArgs F;
    F.growth = growth, F.backoff = backoff, F.growth_interval = growth_interval, F.n_steps = n_steps;
    F.steps = steps, F.growth_tracker = growth_tracker, F.info = info;
    hipLaunchKernelGGL(k_lamb_apply, grid, block, 0, (hipStream_t)stream, chunks, n_chunks, exp_avg, exp_avg_sq, derived, pn, un, flags,
                       scale, F);
    return launch_status();
}

extern "C" int64_t g2048_lamb_workspace_floats(int n_chunks) {
    return n_chunks <= 0 ? 0 : 3 * (int64_t)((n_chunks + 3) & ~3) + 4 + G2048_OPT_MAX_GROUPS * (int64_t)(sizeof(LambDerived) / sizeof(float));
}
