// MFMA and LDS building blocks shared by the HIP translation units: vector typedefs, the fragment layouts of
// v_mfma_f32_32x32x16_bf16, compile-time loops and scheduling fences, the LDS-DMA wrappers, LDS-only barriers, the cycle-stamp
// struct of the diagnostic builds; then what the fused update kernels (csrc/g2048_tail.hip, g2048_rowgemm.hip, g2048_mlp.hip) add:
// the register ring that streams fragment-packed weight units ahead of their MFMAs and LDS activation tiles.
// Scalar helpers (bf16 bits, dropout hash, packed_off) live in csrc/g2048_bits.h and are visible through this namespace.
// Device code only; users write `using namespace g2048_mfma` inside their anonymous namespace, or `using` declarations for single
// names where a file has shapes of its own under the same name (csrc/g2048_policy.hip: bias_tile, gemm_tile).
// Helpers that share a name elsewhere but not a body keep distinct names here (lds_barrier / lds_barrier_asm).
#ifndef G2048_MFMA_H
#define G2048_MFMA_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "g2048_bits.h"

namespace g2048_mfma {

using namespace g2048_bits;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// accumulator register i of lane (r, h) holds row rowof(i, h), column r of a 32 x 32 tile
__device__ __forceinline__ int rowof(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// v_mfma_f32_32x32x16_f16: the same operand and accumulator maps as the bf16 form (csrc/g2048_f32split.hip)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x16 mfma_f16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// two-way fp16 split of s * v (s a power of two): hi = f16(s v), lo = f16(s v - hi); the subtraction is exact in f32
__device__ __forceinline__ void split_f16(const float v[8], float s, f16x8 &hi, f16x8 &lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float sv = s * v[j];
        const _Float16 t = (_Float16)sv;
        hi[j] = t;
        lo[j] = (_Float16)(sv - (float)t);
    }
}

// compile-time loop: f(integral_constant<int, I>) for I = I0..N-1, every index a constant (register arrays stay registers,
// `if constexpr` on the step number prunes the body per step)
template <int I, int N, class Fn>
__device__ __forceinline__ void static_for(Fn &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// nothing is scheduled across this point
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// ---- LDS-DMA ----------------------------------------------------------------------------------------------------------
// One LDS-DMA wave-instruction (BYTES per lane, lane l lands at lds + BYTES l), written as inline assembly ON PURPOSE: for the builtin
// the compiler's wait-count pass makes every later LDS read of the wave wait for the DMA (it cannot tell the buffers of one dynamic
// LDS array apart), i.e. `s_waitcnt vmcnt(0)` right after the fetch that is meant to stay in flight for a whole tile.  The waits for
// these fetches are therefore all explicit in the kernels that use them (`s_waitcnt vmcnt(0)` + barrier).  Unknown to the compiler,
// they can only make ITS counted waits longer, never shorter (vmcnt retires in order and they are younger than what it waits for or it
// waits for 0).
// (m0 is "reserved" for the compiler; it writes it only right in front of its own LDS-DMA builtins, which these kernels do not use)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ uint32_t lds_addr(void *lds) {  // wave-uniform LDS byte address, in a scalar register
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)lds);
}
template <int BYTES>
__device__ __forceinline__ void dma_async(const void *g, void *lds) {
    const uint32_t l = lds_addr(lds);
    if (BYTES == 16) asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(l) : "memory", "m0");
    else asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g), "s"(l) : "memory", "m0");
}
// 16 bytes per lane with a scalar base and a 32-bit per-lane byte offset: no vector address arithmetic per instruction
__device__ __forceinline__ void dma16(const void *sbase, uint32_t voff, uint32_t lds_address) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_address) : "memory", "m0");
}
__device__ __forceinline__ void dma_async16(const void *sbase, uint32_t voff, void *lds) { dma16(sbase, voff, lds_addr(lds)); }
#pragma clang diagnostic pop

// ---- LDS-only workgroup barriers: __syncthreads() also drains vmcnt, i.e. waits for the global fetches that are meant to stay in
// flight and for the wave's global stores.  Two bodies on purpose.
// builtin barrier + scheduling fence (tail, rowgemm, mlp)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    sched_fence();
}
// wait and barrier as ONE asm statement, no scheduling fence (linear, dweight)
__device__ __forceinline__ void lds_barrier_asm() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- cycle stamps of the diagnostic builds (tools/stamps_encoder.py, tools/stamps_linear.py; never in the product library):
// s_memtime at phase boundaries, summed per phase in scalar registers; at kernel exit the waves with Site::on(lane, w) add
// their sums to Site::table(w)
template <int N, class Site>
struct Stamps {
    unsigned long long last, acc[N];
    __device__ __forceinline__ static unsigned long long now() {
        unsigned long long t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        return t;
    }
    __device__ __forceinline__ void start() {
        for (int i = 0; i < N; ++i) acc[i] = 0;
        last = now();
    }
    __device__ __forceinline__ void mark(int k) {
        const unsigned long long t = now();
        acc[k] += t - last;
        last = t;
    }
    __device__ __forceinline__ void flush(int lane, int w) {
        if (Site::on(lane, w))
            for (int i = 0; i < N; ++i) atomicAdd(&Site::table(w)[i], acc[i]);
    }
};

// ---- fused update kernels: accumulator tiles, LDS activation tiles, the weight ring ------------------------------------------
// acc[i] = b[row0 + rowof(i, h)]: the bias enters through the accumulator's initial value
__device__ __forceinline__ f32x16 bias_tile(const float *b, int row0, int h) {
    f32x16 a;
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(b + row0 + 8 * g + 4 * h);
        for (int q = 0; q < 4; ++q) a[4 * g + q] = v[q];
    }
    return a;
}
__device__ __forceinline__ f32x16 zero_tile() {
    f32x16 a;
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
    return a;
}
// acc += W[row0 .. row0+31][k0 .. k0 + 16 NK) . X, X = NK operand fragments (rows on lanes).  W row-major with leading
// dimension ld (elements); the A fragment of k-step ks is 16 bytes of row row0 + r at column k0 + 16 ks + 8 h.
template <int NK>
__device__ __forceinline__ f32x16 tile_gemm(const __bf16 *__restrict__ W, int ld, int row0, int k0, const bf16x8 *xf, f32x16 acc, int r,
                                            int h) {
    const __bf16 *p = W + (size_t)(row0 + r) * ld + k0 + 8 * h;
    bf16x8 a[NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) a[ks] = *reinterpret_cast<const bf16x8 *>(p + 16 * ks);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) acc = mfma(a[ks], xf[ks], acc);
    return acc;
}
// operand fragments of an LDS activation tile (row-major bf16, byte stride `stride`): columns k0 .. k0 + 16 NK of row r
template <int NK>
__device__ __forceinline__ void load_frags(const char *buf, int stride, int k0, bf16x8 *xf, int r, int h) {
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) xf[ks] = *reinterpret_cast<const bf16x8 *>(buf + r * stride + 2 * (k0 + 16 * ks + 8 * h));
}
// four consecutive features (accumulator group g) of row r into a row-major LDS tile
__device__ __forceinline__ void put4(char *buf, int stride, int r, int col, const float v[4]) {
    bf16x4 pk;
    for (int q = 0; q < 4; ++q) pk[q] = (__bf16)v[q];
    *reinterpret_cast<bf16x4 *>(buf + r * stride + 2 * col) = pk;
}
constexpr int RING = 3, DIST = 2;  // RING = DIST + 1: the slot of unit i + DIST was last read by unit i - 1


struct Ring {
    bf16x8 a[RING][16];
};
// fragments 0..7 at p + 512 ks, fragments 8..15 at p + off2 + 512 ks (elements; p = this lane's 16 bytes of the first fragment of a
// fragment-packed weight: one contiguous KB per wave-instruction)
template <int SLOT>
__device__ __forceinline__ void fetch_unit(Ring &R, const __bf16 *p, int64_t off2) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) R.a[SLOT][ks] = *reinterpret_cast<const bf16x8 *>(p + 512 * ks);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) R.a[SLOT][8 + ks] = *reinterpret_cast<const bf16x8 *>(p + off2 + 512 * ks);
}
template <int SLOT>
__device__ __forceinline__ f32x16 mm16(const Ring &R, const bf16x8 *xf, f32x16 acc) {
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) acc = mfma(R.a[SLOT][ks], xf[ks], acc);
    return acc;
}
template <int SLOT, int HALF>
__device__ __forceinline__ f32x16 mm8(const Ring &R, const bf16x8 *xf, f32x16 acc) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) acc = mfma(R.a[SLOT][8 * HALF + ks], xf[ks], acc);
    return acc;
}
// per-lane address of a unit's first fragment in a fragment-packed [rows][cols] weight: row tile row0 / 32, k-step k0 / 16
__device__ __forceinline__ const __bf16 *unit_ptr(const void *W, int cols, int row0, int k0, int lane) {
    return (const __bf16 *)W + ((size_t)(row0 >> 5) * (cols >> 4) + (k0 >> 4)) * 512 + lane * 8;
}
constexpr int64_t NEXT_8_STEPS = 8 * 512;  // off2 of a unit = one row tile over 256 columns
__device__ __forceinline__ int64_t next_row_tile(int cols) { return (int64_t)(cols >> 4) * 512; }  // off2 of a unit = two row tiles over 128 columns

}  // namespace g2048_mfma
#endif  // G2048_MFMA_H
