// Per-lane primitives of the canonical frame (include/g2048.h, "canonical frame"): the eight dihedral views of a board held as
// four row dwords (g2048_device.h), the lexicographically largest of them, and the action / mask / logit permutations that
// turn with the view.  Branch-free; compiles as plain host C++ under G2048_HOST_TEST like g2048_device.h.
//
// With t = transpose(m), H = byte reversal inside every row (fliplr) and V = row order reversal (flipud), np.rot90 is
// V(transpose(.)), so the views g = 4 f + k of m are
//
//   g      0    1      2        3      4    5      6        7
//   view   m    V(t)   V(H(m))  H(t)   t    V(m)   V(H(t))  H(m)
//
// i.e. the four register sets m, t, H(m), H(t) in forward or reversed row order: one transpose (8 v_perm_b32) and eight byte
// reversals (one v_perm_b32 each) build all eight.  "Compared from cell 0 upward" is the order of the byte-reversed row dwords
// taken as one 128-bit number, and the byte-reversed rows of a view built from X are the rows of H(X): the four sets are also
// each other's compare keys, nothing more is computed.
#pragma once
#include "g2048_device.h"

namespace g2048 {

G_DEV u32 reverse_bytes(u32 x) { return perm(0u, x, 0x00010203u); }

// sigma_g(a) = ((a ^ f) - k) mod 4: the action that does in view g what a does in the env's frame
G_DEV u32 sym_sigma(u32 g, u32 a) { return ((a ^ (g >> 2)) - (g & 3u)) & 3u; }

// bit sigma_g(a) of the result = bit a of mask; the high bits are dropped
G_DEV u32 sym_perm_mask(u32 g, u32 mask) {
    u32 out = 0;
    for (u32 a = 0; a < 4; ++a) out |= ((mask >> a) & 1u) << sym_sigma(g, a);
    return out;
}

// one candidate view: rows x[0..3] (already in the view's row order) with compare key k[0..3]; replaces the best so far only if
// strictly larger, so that among equal views the smallest g stays
G_DEV void sym_consider(u32 g, u32 x0, u32 x1, u32 x2, u32 x3, u32 k0, u32 k1, u32 k2, u32 k3, Board &best, uint64_t &bhi,
                        uint64_t &blo, u32 &bg) {
    const uint64_t hi = ((uint64_t)k0 << 32) | k1, lo = ((uint64_t)k2 << 32) | k3;
    const bool gt = hi > bhi || (hi == bhi && lo > blo);
    best.r[0] = gt ? x0 : best.r[0]; best.r[1] = gt ? x1 : best.r[1];
    best.r[2] = gt ? x2 : best.r[2]; best.r[3] = gt ? x3 : best.r[3];
    bhi = gt ? hi : bhi;
    blo = gt ? lo : blo;
    bg = gt ? g : bg;
}

// bd -> canon(bd); returns frame(bd), the smallest g with view_g(bd) == canon(bd)
G_DEV u32 sym_canon(Board &bd) {
    const Board m = bd;
    Board t = bd, hm, ht;
    transpose(t);
    for (int i = 0; i < 4; ++i) {
        hm.r[i] = reverse_bytes(m.r[i]);
        ht.r[i] = reverse_bytes(t.r[i]);
    }
    Board best = m;  // g = 0
    uint64_t bhi = ((uint64_t)hm.r[0] << 32) | hm.r[1], blo = ((uint64_t)hm.r[2] << 32) | hm.r[3];
    u32 bg = 0;
#define G2048_FWD(g, X, K) sym_consider(g, X.r[0], X.r[1], X.r[2], X.r[3], K.r[0], K.r[1], K.r[2], K.r[3], best, bhi, blo, bg)
#define G2048_REV(g, X, K) sym_consider(g, X.r[3], X.r[2], X.r[1], X.r[0], K.r[3], K.r[2], K.r[1], K.r[0], best, bhi, blo, bg)
    G2048_REV(1u, t, ht);
    G2048_REV(2u, hm, m);
    G2048_FWD(3u, ht, t);
    G2048_FWD(4u, t, ht);
    G2048_REV(5u, m, hm);
    G2048_REV(6u, ht, t);
    G2048_FWD(7u, hm, m);
#undef G2048_FWD
#undef G2048_REV
    bd = best;
    return bg;
}

// out[a] = in[sigma_g(a)] on four 32-bit patterns (selects: a register array indexed by a lane value would go to scratch)
G_DEV u32 sym_pick(u32 x, u32 y, u32 z, u32 w, u32 i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }

// ---- eight-view ensemble (include/g2048.h, "eight-view ensemble") ----------------------------------------------------------------
// view_g(m), g in 0 .. 7 (the low three bits count).  In the table at the top of the file the view is built from t for
// g in {1, 3, 4, 6}, byte-reversed for g in {2, 3, 6, 7} and in reversed row order for g in {1, 2, 5, 6}: three bits of g, three
// rounds of selects (a register array indexed by a lane value would go to scratch).
G_DEV Board sym_view(const Board &m, u32 g) {
    Board t = m, hm, ht, out;
    transpose(t);
    for (int i = 0; i < 4; ++i) {
        hm.r[i] = reverse_bytes(m.r[i]);
        ht.r[i] = reverse_bytes(t.r[i]);
    }
    const bool from_t = ((g ^ (g >> 2)) & 1u) != 0, flipped = (g & 2u) != 0, reversed = ((g ^ (g >> 1)) & 1u) != 0;
    u32 x[4];
    for (int i = 0; i < 4; ++i) {
        const u32 plain = from_t ? t.r[i] : m.r[i], turned = from_t ? ht.r[i] : hm.r[i];
        x[i] = flipped ? turned : plain;
    }
    for (int i = 0; i < 4; ++i) out.r[i] = reversed ? x[3 - i] : x[i];
    return out;
}

G_DEV u32 float_as_u32(float x) {
#if G2048_ON_DEVICE
    return __float_as_uint(x);
#else
    u32 b;
    memcpy(&b, &x, 4);
    return b;
#endif
}

// f32 bit pattern <-> an unsigned key whose order is the total order of the patterns as sign-magnitude numbers:
// -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN
G_DEV u32 sym_sort_key(u32 bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
G_DEV u32 sym_sort_unkey(u32 key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

G_DEV void sym_cmpx(u32 &a, u32 &b) {
    const u32 lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// The mean of eight f32 (as bit patterns, result as a bit pattern) as a function of their MULTISET: sorted by the order above
// with a fixed 19-compare-exchange network on the integer keys (which, unlike fminf / fmaxf, cannot drop a NaN), added in
// ascending order, every add rounded on its own, times 0.125 (exact short of underflow).  NaN whenever an addend is NaN or both
// infinities occur (payload unspecified); equal keys are equal patterns, and -0 / +0 are neighbours in the order, so no
// permutation of the eight changes a bit of the result.  x[] is left sorted as keys; all indices are constants after unrolling.
G_DEV u32 sym_sorted_mean8(u32 x[8]) {
    for (int i = 0; i < 8; ++i) x[i] = sym_sort_key(x[i]);
    sym_cmpx(x[0], x[2]); sym_cmpx(x[1], x[3]); sym_cmpx(x[4], x[6]); sym_cmpx(x[5], x[7]);
    sym_cmpx(x[0], x[4]); sym_cmpx(x[1], x[5]); sym_cmpx(x[2], x[6]); sym_cmpx(x[3], x[7]);
    sym_cmpx(x[0], x[1]); sym_cmpx(x[2], x[3]); sym_cmpx(x[4], x[5]); sym_cmpx(x[6], x[7]);
    sym_cmpx(x[2], x[4]); sym_cmpx(x[3], x[5]);
    sym_cmpx(x[1], x[4]); sym_cmpx(x[3], x[6]);
    sym_cmpx(x[1], x[2]); sym_cmpx(x[3], x[4]); sym_cmpx(x[5], x[6]);
    float s = u32_as_float(sym_sort_unkey(x[0]));
    for (int i = 1; i < 8; ++i) s = add_rn(s, u32_as_float(sym_sort_unkey(x[i])));
    return float_as_u32(mul_rn(s, 0.125f));
}

}  // namespace g2048
