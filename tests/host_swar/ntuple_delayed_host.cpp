// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple_delayed.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: lets tests/ check the per-lane code the kernels of g2048_ntuple_delayed.hip run against the numpy
// restatement without a GPU.  The launches are emulated sequentially, env by env.  The product never builds or loads this.
// With NTUPLE_DELAYED_HOST_MAIN it is a stand-alone program (for a sanitizer build): lock-steps of accumulate, apply and link at
// h = 8 on a ring and tables of exactly the sizes the definition states.
#define G2048_HOST_TEST 1
#include "g2048_ntuple_delayed.h"
using namespace g2048;

namespace {

// the network as the entry points read it (nt_read_staged), without their argument checks
NtNet make_net(const uint8_t *cells, int m, int L, const uint8_t *tiles, int n_stages) {
    NtNet net;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t)
        for (int j = 0; j < L; ++j) net.cell[t][j] = cells[t * L + j];
    for (int i = 0; i + 1 < n_stages; ++i) net.stage_tile[i] = tiles[i];
    net.n_stage_tiles = n_stages - 1;
    return net;
}

int ring_len(const uint8_t *hist_len, int64_t b, int h) { return hist_len[b] < h ? hist_len[b] : h; }  // as the kernels read it

template <int M>
void accumulate(bool tc, const uint8_t *hist, float *hist_err, const uint8_t *hist_len, const uint8_t *flag, const float *target,
                int64_t B, int h, int head, float lam, const int32_t *w, const NtNet &net, float scale, float c, int64_t *acc,
                int64_t *abs_acc, int32_t *cnt, float *td_error) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_dl_accumulate
        const u32 f = flag[b];
        float e = 0.0f;
        if (f) {
            const int len = ring_len(hist_len, b, h);
            e = tc ? nt_dl_accumulate_lane<M, true>(hist, hist_err, b, B, h, head, len, f, target[b], lam, w, net, scale, c, acc, abs_acc, cnt)
                   : nt_dl_accumulate_lane<M, false>(hist, hist_err, b, B, h, head, len, f, target[b], lam, w, net, scale, c, acc, abs_acc,
                                                     cnt);
        }
        if (td_error) td_error[b] = e;
    }
}

template <int M>
void apply(bool tc, const uint8_t *hist, const uint8_t *hist_len, const uint8_t *flag, int64_t B, int h, int head, const NtNet &net,
           int32_t *w, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_dl_apply
        const u32 f = flag[b];
        if (!f) continue;
        const int len = ring_len(hist_len, b, h);
        if (tc)
            nt_dl_apply_lane<M, true>(hist, b, B, h, head, len, f, net, w, acc, abs_acc, cnt, coh_e, coh_a);
        else
            nt_dl_apply_lane<M, false>(hist, b, B, h, head, len, f, net, w, acc, abs_acc, cnt, coh_e, coh_a);
    }
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
// abs_acc null: TD (as the entry point decides)
void hst_nt_dl_accumulate(const uint8_t *hist, float *hist_err, const uint8_t *hist_len, const uint8_t *flag, const float *target,
                          int64_t B, int h, int head, double lam, const int32_t *w, const uint8_t *cells, int m, int L,
                          const uint8_t *tiles, int n_stages, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                          float *td_error) {
    const NtNet net = make_net(cells, m, L, tiles, n_stages);
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));  // as the entry point computes it
    NT_SWITCH(accumulate, m, abs_acc != nullptr, hist, hist_err, hist_len, flag, target, B, h, head, (float)lam, w, net,
              nt_scale(frac_bits), c, acc, abs_acc, cnt, td_error);
}
void hst_nt_dl_apply(const uint8_t *hist, const uint8_t *hist_len, const uint8_t *flag, int64_t B, int h, int head, const uint8_t *cells,
                     int m, int L, const uint8_t *tiles, int n_stages, int32_t *w, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                     int32_t *coh_e, int32_t *coh_a) {
    const NtNet net = make_net(cells, m, L, tiles, n_stages);
    NT_SWITCH(apply, m, abs_acc != nullptr, hist, hist_len, flag, B, h, head, net, w, acc, abs_acc, cnt, coh_e, coh_a);
}
void hst_nt_dl_link(const uint8_t *boards_row, const uint8_t *meta_row, int64_t B, int h, int slot, uint8_t *prev_after, uint8_t *flag,
                    uint8_t *hist, uint8_t *hist_len) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_dl_link
        Board bd = nt_dl_board(boards_row, b);
        u32 f;
        const u32 len = nt_dl_link_lane(bd, meta_row[b], flag[b], hist_len[b], h, f);
        flag[b] = (uint8_t)f;
        hist_len[b] = (uint8_t)len;
        memcpy(prev_after + 16 * b, bd.r, 16);
        memcpy(hist + 16 * ((int64_t)slot * B + b), bd.r, 16);
    }
}
int hst_nt_dl_ring_ok(int h, int pos) { return nt_dl_ring_ok(h, pos) ? 1 : 0; }
}

#ifdef NTUPLE_DELAYED_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// 40 lock-steps of TC(lambda) and of TD(lambda) at h = 8 (head and slot go round the ring five times) on B = 37 envs over a
// three-stage network, with targets of +-1e9 at alpha 1000 so that delta sits on the +-2^30 clamp, tiles above 15, and episode ends
// that flush rings shorter than h.  The ring is exactly [8][B][16] / [8][B] / [B] and every table exactly [S][m][16^L]: under
// -fsanitize=address,undefined a slot or an offset one past them, or a signed overflow, aborts the run.  Exits non-zero if an
// accumulator is not zero after a step, if hist_len leaves 1 .. h, or if |E| > A anywhere.
int main() {
    const int m = 3, L = 2, F = 12, S = 3, h = 8;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15}, tiles[S - 1] = {3, 16};
    const int64_t E = (int64_t)S * m << (4 * L), B = 37;
    for (int tc = 0; tc < 2; ++tc) {
        std::vector<int32_t> w(E), cnt(E, 0), coh_e(E, 0), coh_a(E, 0);
        std::vector<int64_t> acc(E, 0), abs_acc(E, 0);
        std::vector<uint8_t> hist(h * B * 16, 0), hist_len(B, 0), flag(B, 0), prev(16 * B, 0), row(16 * B), meta(B);
        std::vector<float> hist_err(h * B, 0.0f), target(B), err(B);
        uint32_t s = 12345u;
        auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
        for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
        for (int n = 0; n < 40; ++n) {
            for (int64_t b = 0; b < B; ++b) target[b] = (rnd() & 4) ? 1e9f : -1e9f;
            const int head = (n + h - 1) % h;
            hst_nt_dl_accumulate(hist.data(), hist_err.data(), hist_len.data(), flag.data(), target.data(), B, h, head, 0.5, w.data(),
                                 cells, m, L, tiles, S, F, 1000.0, acc.data(), tc ? abs_acc.data() : nullptr, cnt.data(), err.data());
            hst_nt_dl_apply(hist.data(), hist_len.data(), flag.data(), B, h, head, cells, m, L, tiles, S, w.data(), acc.data(),
                            tc ? abs_acc.data() : nullptr, cnt.data(), tc ? coh_e.data() : nullptr, tc ? coh_a.data() : nullptr);
            for (int64_t i = 0; i < E; ++i) {
                if (acc[i] != 0 || abs_acc[i] != 0 || cnt[i] != 0) return 2;
                const int64_t e = coh_e[i], a = coh_a[i];
                if (a < 0 || (e < 0 ? -e : e) > a) return 3;
            }
            for (int64_t b = 0; b < B; ++b) {
                if (!(err[b] == err[b])) return 4;
                for (int c = 0; c < 16; ++c) row[16 * b + c] = b == 0 ? 3 : (b == 1 ? (uint8_t)(16 + (c & 1)) : (uint8_t)(rnd() >> 28));
                meta[b] = (uint8_t)((rnd() >> 30) | 0x3C | ((rnd() >> 29) == 0 ? 0x40 : 0));  // an episode end one time in eight
            }
            hst_nt_dl_link(row.data(), meta.data(), B, h, n % h, prev.data(), flag.data(), hist.data(), hist_len.data());
            for (int64_t b = 0; b < B; ++b)
                if (hist_len[b] < 1 || hist_len[b] > h || (flag[b] != 1 && flag[b] != 2)) return 5;
        }
    }
    printf("ntuple_delayed_host ok\n");
    return 0;
}
#endif
