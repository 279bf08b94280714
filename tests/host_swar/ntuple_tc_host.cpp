// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple_tc.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: lets tests/ check the per-lane TC code the kernels of g2048_ntuple_tc.hip run against the numpy
// restatement without a GPU.  Accumulate and apply are emulated sequentially, env by env.  The product never builds or loads this.
// With NTUPLE_TC_HOST_MAIN it is a stand-alone program (for a sanitizer build): six consecutive steps that include the halving.
#define G2048_HOST_TEST 1
#include "g2048_ntuple_tc.h"
using namespace g2048;

namespace {

NtNet make_net(const uint8_t *cells, int m, int L) {
    NtNet net;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t)
        for (int j = 0; j < L; ++j) net.cell[t][j] = cells[t * L + j];
    return net;
}

Board get(const uint8_t *p, int64_t i) {
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
}

template <int M>
void accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w, const NtNet &net,
                float scale, float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt, float *td_error) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_tc_accumulate
        float e = 0.0f;
        if (flag[b]) e = nt_tc_accumulate_lane<M>(get(prev, b), flag[b], target[b], w, net, scale, c, acc, abs_acc, cnt);
        if (td_error) td_error[b] = e;
    }
}

template <int M>
void apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const NtNet &net, int32_t *w, int64_t *acc, int64_t *abs_acc,
           int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    for (int64_t b = 0; b < B; ++b)  // the body of k_nt_tc_apply
        if (flag[b]) nt_tc_apply_lane<M>(get(prev, b), net, w, acc, abs_acc, cnt, coh_e, coh_a);
}

}  // namespace

#define NT_SWITCH(FN, m, ...)              \
    switch (m) {                           \
        case 1: FN<1>(__VA_ARGS__); break; \
        case 2: FN<2>(__VA_ARGS__); break; \
        case 3: FN<3>(__VA_ARGS__); break; \
        case 4: FN<4>(__VA_ARGS__); break; \
        case 5: FN<5>(__VA_ARGS__); break; \
        case 6: FN<6>(__VA_ARGS__); break; \
        case 7: FN<7>(__VA_ARGS__); break; \
        default: FN<8>(__VA_ARGS__); break; \
    }

extern "C" {
void hst_nt_tc_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w,
                          const uint8_t *cells, int m, int L, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                          float *td_error) {
    const NtNet net = make_net(cells, m, L);
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));  // as the entry point computes it
    NT_SWITCH(accumulate, m, prev, flag, target, B, w, net, nt_scale(frac_bits), c, acc, abs_acc, cnt, td_error);
}
void hst_nt_tc_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const uint8_t *cells, int m, int L, int32_t *w, int64_t *acc,
                     int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    const NtNet net = make_net(cells, m, L);
    NT_SWITCH(apply, m, prev, flag, B, net, w, acc, abs_acc, cnt, coh_e, coh_a);
}
}

#ifdef NTUPLE_TC_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// six TC steps on the same boards (tiles above 15, self-symmetric boards) with alpha = 1000 and targets of +-1e9, so that delta
// sits on the +-2^30 clamp and A reaches 2^31 at the second step: exits non-zero if acc / abs_acc / cnt are not all zero after a
// step, if |E| > A or A < 0 anywhere, or if the entry that board 1 hits was not halved.  Under -fsanitize=address,undefined an
// out-of-table access or a signed overflow aborts the run.
int main() {
    const int m = 3, L = 2, F = 12;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const int64_t E = (int64_t)m << (4 * L), B = 40;
    std::vector<int32_t> w(E), cnt(E, 0), coh_e(E, 0), coh_a(E, 0);
    std::vector<int64_t> acc(E, 0), abs_acc(E, 0);
    std::vector<uint8_t> prev(16 * B), flag(B);
    std::vector<float> target(B), err(B);
    uint32_t s = 12345u;
    auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
    for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
    w[0] = 2147483647;
    w[1] = -2147483647 - 1;
    for (int64_t b = 0; b < B; ++b) {
        for (int c = 0; c < 16; ++c) prev[16 * b + c] = b == 0 ? 0 : (b == 1 ? 3 : (b == 2 ? 16 + (c & 1) : (uint8_t)(rnd() >> 28)));
        flag[b] = (uint8_t)(b % 7 == 3 ? 0 : (b % 5 == 0 ? 2 : 1));
    }
    for (int step = 0; step < 6; ++step) {
        for (int64_t b = 0; b < B; ++b) target[b] = (b == 1 || (rnd() & 4)) ? 1e9f : -1e9f;  // board 1: the same sign every step
        hst_nt_tc_accumulate(prev.data(), flag.data(), target.data(), B, w.data(), cells, m, L, F, 1000.0, acc.data(), abs_acc.data(),
                             cnt.data(), err.data());
        hst_nt_tc_apply(prev.data(), flag.data(), B, cells, m, L, w.data(), acc.data(), abs_acc.data(), cnt.data(), coh_e.data(),
                        coh_a.data());
        for (int64_t i = 0; i < E; ++i) {
            if (acc[i] != 0 || abs_acc[i] != 0 || cnt[i] != 0) return 2;
            const int64_t e = coh_e[i], a = coh_a[i];
            if (a < 0 || (e < 0 ? -e : e) > a) return 3;
        }
        for (int64_t b = 0; b < B; ++b)
            if (!(err[b] == err[b])) return 4;
    }
    // board 1 hits entry 0x33 of tuple 0 at every step with |delta| = 2^30: six means of 2^30 stay at 2^30 only through a halving
    // at every step from the second on
    if (coh_a[0x33] != (1 << 30)) return 5;
    printf("ntuple_tc_host ok\n");
    return 0;
}
#endif
