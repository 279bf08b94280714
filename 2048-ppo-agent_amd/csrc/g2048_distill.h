// Per-sample code of the imitation (distillation) loss (include/g2048.h, "imitation update: loss"): cross-entropy of the policy's
// masked softmax to a teacher's action scores, the optional critic regression and entropy terms, and their gradients.
//
//   z_j   = logit_j, or logit_j - 1e8 where action j is illegal                          (k_ppo_loss's convention)
//   pi    = softmax(z), lp = log pi, ent = -sum_j lp_j pi_j
//   a*    = the first maximum over j of q_j - (legal ? 0 : 1e8)                           (the engine's masked argmax)
//   p*    = one-hot at a* (tau == 0), or exp((q_j - q_a*) / tau) / sum over the legal j, 0 where illegal (tau > 0)
//   ce    = -sum over the legal j of p*_j lp_j,  vl = (V - value_target)^2,  el = -ent,  tot = ce + c_value vl + c_entropy el
//   d tot / d z_j = (pi_j - p*_j) + c_entropy pi_j (lp_j + ent),   d tot / d V = 2 c_value (V - value_target)
//
// Every exponent is <= 0 (q_a* is the largest legal score), so teacher scores of any magnitude give a one-hot p* by underflow and
// never a NaN.  A row without a legal action is all zeros.  The text builds for the device and, with G2048_HOST_TEST, for the host
// (tests/host_swar/distill_host.cpp), where expf / logf are libm's: the two agree within the bounds of tests/distill_ref.py, not
// bit for bit.
#pragma once
#include "g2048_device.h"

namespace g2048 {

enum { DISTILL_NSUM = 5 };  // ce, vl, el, tot, agreement

struct DistillOut {
    float dz[4];             // d tot / d z_j (unscaled: the caller multiplies by grad_scale / M)
    float dv;                // d tot / d V
    float new_logp;          // lp[a*]
    float term[DISTILL_NSUM];
};

G_DEV float distill_u32_as_float(uint32_t x) {
    float f;
    memcpy(&f, &x, 4);
    return f;
}
G_DEV uint32_t distill_float_as_u32(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    return x;
}

// element i of a bf16 or f32 array
G_DEV float distill_ld(const void *p, int64_t i, int bf16) {
    if (bf16) return distill_u32_as_float((uint32_t)((const uint16_t *)p)[i] << 16);
    return ((const float *)p)[i];
}
// round to nearest even, NaN stays NaN
G_DEV void distill_st(void *p, int64_t i, int bf16, float v) {
    if (bf16) {
        uint32_t x = distill_float_as_u32(v);
        if ((x & 0x7FFFFFFFu) > 0x7F800000u)
            x = (x >> 16) | 0x40u;
        else
            x = (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
        ((uint16_t *)p)[i] = (uint16_t)x;
    } else {
        ((float *)p)[i] = v;
    }
}

// first maximum of x[j] - (legal ? 0 : 1e8)
G_DEV int distill_masked_argmax(const float x[4], uint32_t mb) {
    int a = 0;
    float best = ((mb & 1u) ? x[0] : x[0] - 1e8f);
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const float v = ((mb >> j) & 1u) ? x[j] : x[j] - 1e8f;
        if (v > best) {
            best = v;
            a = j;
        }
    }
    return a;
}

// one sample.  mb: bit j = action j legal (0xF for no masking); has_v: the critic terms are on (else vl = dv = 0)
G_DEV void distill_sample(const float l[4], uint32_t mb, const float q[4], bool has_v, float v, float vt, float tau, float c_value,
                          float c_entropy, DistillOut &o) {
    mb &= 0xFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.dz[j] = 0.0f;
    o.dv = 0.0f;
    o.new_logp = 0.0f;
#pragma unroll
    for (int k = 0; k < DISTILL_NSUM; ++k) o.term[k] = 0.0f;
    if (mb == 0u) return;

    float z[4], zmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        z[j] = ((mb >> j) & 1u) ? l[j] : l[j] - 1e8f;
        zmax = fmaxf(zmax, z[j]);
    }
    float se = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) se += expf(z[j] - zmax);
    const float lse = zmax + logf(se);
    float lp[4], p[4], ent = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lp[j] = z[j] - lse;
        p[j] = expf(lp[j]);
        ent -= lp[j] * p[j];
    }

    const int a = distill_masked_argmax(q, mb);
    const float qa = a == 0 ? q[0] : (a == 1 ? q[1] : (a == 2 ? q[2] : q[3]));  // selects: no run-time register index
    float t[4], ts = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool legal = (mb >> j) & 1u;
        if (tau > 0.0f)
            t[j] = legal ? expf((q[j] - qa) / tau) : 0.0f;
        else
            t[j] = j == a ? 1.0f : 0.0f;
        ts += t[j];
    }
    float ce = 0.0f, nlp = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[j] = t[j] / ts;  // ts >= 1: the term of a* is exp(0)
        if ((mb >> j) & 1u) ce -= t[j] * lp[j];
        if (j == a) nlp = lp[j];
    }
    float vl = 0.0f;
    if (has_v) {
        const float dv = v - vt;
        vl = dv * dv;
        o.dv = 2.0f * c_value * dv;
    }
    const float el = -ent;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.dz[j] = (p[j] - t[j]) + c_entropy * p[j] * (lp[j] + ent);
    o.new_logp = nlp;
    o.term[0] = ce;
    o.term[1] = vl;
    o.term[2] = el;
    o.term[3] = ce + c_value * vl + c_entropy * el;
    o.term[4] = distill_masked_argmax(l, mb) == a ? 1.0f : 0.0f;
}

}  // namespace g2048
