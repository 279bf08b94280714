// Scalar and bit-level device helpers shared by every update kernel: f32 <-> bf16 bits, the wave reduction, the update's dropout
// hash, the fragment-packed weight offset.  No MFMA, no LDS: usable from any translation unit (csrc/g2048_mfma.h builds on it).
// ONE definition each: the dropout hash and packed_off are contracts between kernels, not conveniences.
// Device code only; users pull the names in with `using namespace g2048_bits` inside their anonymous namespace.
#ifndef G2048_BITS_H
#define G2048_BITS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g2048_bits {

// ---- f32 <-> bf16 bits ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf2f(uint32_t hi16) { return __uint_as_float(hi16 << 16); }
__device__ __forceinline__ uint32_t f2bf(float f) {  // round to nearest even (the compiler's conversion)
    const __bf16 b = (__bf16)f;
    return *reinterpret_cast<const uint16_t *>(&b);
}
__device__ __forceinline__ uint32_t pack2(float a, float b) { return f2bf(a) | (f2bf(b) << 16); }

// ---- wave reduction ---------------------------------------------------------------------------------------------------
// sum over the 64 lanes by __shfl_xor (ds_bpermute_b32); the DPP form of csrc/g2048_rowgemm.hip adds in another order
__device__ __forceinline__ float wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- the update's dropout hash ----------------------------------------------------------------------------------------
// keep(element idx) = bits of fin(idx.lo * HASH_MUL ^ s0 ^ (idx.hi * HASH_MUL_HI + s1)) against a threshold.  Every forward and
// its backward, fused or not, must draw the same mask for the same element index: all of them are written on these definitions.
// (tests/test_gpu_tail.py restates the hash in numpy on purpose.)
constexpr uint32_t HASH_MUL = 0x9E3779B1u, HASH_MUL_HI = 0x85EBCA77u;  // multipliers of the index's low and high word
// The finaliser, in place on a uint32_t lvalue.  A macro ON PURPOSE: a forced-inline function is simplified on its own before it is
// inlined, and the sites that compare the two 16-bit halves of one hash (k_relu_dropout_fwd, the epilogues of k_linear / k_linear_ws,
// Drop::apply4) then come out of the vectoriser with another instruction order than with the statements in their body.
#define G2048_HASH_FIN(x) ((x) ^= (x) >> 16, (x) *= 0x7FEB352Du, (x) ^= (x) >> 15, (x) *= 0x846CA68Bu, (x) ^= (x) >> 16)
// 24 hash bits of element idx against thr = p * 2^24
__device__ __forceinline__ bool keep_elem(uint32_t s0, uint32_t s1, uint32_t thr, uint64_t idx) {
    uint32_t x = (uint32_t)idx * HASH_MUL ^ s0;
    x ^= (uint32_t)(idx >> 32) * HASH_MUL_HI + s1;
    G2048_HASH_FIN(x);
    return (x >> 8) >= thr;
}
// the optional device-resident word mixed into the seed (advanced between hipGraph replays)
__device__ __forceinline__ void mix_seed_state(const uint64_t *seed_state, uint32_t &s0, uint32_t &s1) {
    if (seed_state) {
        const uint64_t s = *seed_state;
        s0 ^= (uint32_t)s * HASH_MUL;
        s1 += (uint32_t)(s >> 32) * HASH_MUL_HI + (uint32_t)s;
    }
}
struct Drop {
    uint32_t s0, s1, thr;
    float inv_keep;
    __device__ __forceinline__ Drop site(uint32_t k) const { return Drop{s0 + k * 0x632BE5ABu, s1 ^ (k * 0x7F4A7C15u), thr, inv_keep}; }
    // four consecutive elements idx .. idx + 3 (idx a multiple of 4): one hash per PAIR, its two 16-bit halves compared with the
    // threshold at 16-bit resolution (the convention of g2048_relu_dropout_fwd): half the vector instructions of four full hashes
    __device__ __forceinline__ void apply4(float v[4], uint64_t idx) const {
        if (!thr) return;
        const uint32_t thr16 = thr >> 8;
        for (int pr = 0; pr < 2; ++pr) {
            const uint64_t id = (idx >> 1) + pr;
            uint32_t x = (uint32_t)id * HASH_MUL ^ s0;
            x ^= (uint32_t)(id >> 32) * HASH_MUL_HI + s1;
            G2048_HASH_FIN(x);
            v[2 * pr] = (x & 0xFFFFu) >= thr16 ? v[2 * pr] * inv_keep : 0.0f;
            v[2 * pr + 1] = (x >> 16) >= thr16 ? v[2 * pr + 1] * inv_keep : 0.0f;
        }
    }
};
__device__ __forceinline__ Drop make_drop(uint64_t seed, const uint64_t *seed_state, float p_drop) {
    uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
    mix_seed_state(seed_state, s0, s1);
    return Drop{s0, s1, (uint32_t)(p_drop * 16777216.0f), 1.0f / (1.0f - p_drop)};
}

// ---- fragment-packed weights ------------------------------------------------------------------------------------------
// Fragment-packed layout of a bf16 matrix X[rows][cols] (rows % 32 == 0, cols % 16 == 0), the order in which a wavefront reads
// it as an MFMA operand (include/g2048.h): for every 32-row tile and every 16-column k-step, 64 lanes x 16 bytes = 1 KB contiguous,
//   offset(row, col) = ((((row / 32) * (cols / 16) + col / 16) * 2 + (col / 8) % 2) * 32 + row % 32) * 8 + col % 8.
// Row-major operands make every lane of a fragment load touch a different cache line (lane = row): 64 requests of 16 bytes per
// instruction, measured ~8 B/clk per CU; packed, one instruction is one contiguous KB.
// The optimiser writes the shadows with this formula; tail, rowgemm and mlp read them with it.
__device__ __forceinline__ int64_t packed_off(int64_t row, int64_t col, int64_t cols) {
    return ((((row >> 5) * (cols >> 4) + (col >> 4)) * 2 + ((col >> 3) & 1)) * 32 + (row & 31)) * 8 + (col & 7);
}

}  // namespace g2048_bits
#endif  // G2048_BITS_H
