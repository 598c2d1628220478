// Stand-alone check of resshift_amd/csrc/weight_pack.h (tests/test_host_cpu.py builds it host-only with AddressSanitizer + UBSan and runs
// it; no device, never loaded into Python).  Every weight encodes its own index, so the packed forms are checked against known answers.
#include "weight_pack.h"
#include <cstdio>
#include <limits>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); } } while (0)

// reference tensor [Cout][Cin][taps]: n = 1 + linear index (<= 512) plus a fraction of 1 .. 5 / 2048 - at most 21 significant bits, so a
// split pair holds it exactly; floor() gives the index back
static float enc(int co, int ci, int t, int Cin, int taps) {
    const int n = 1 + (co * Cin + ci) * taps + t;
    return (float)n + (float)(n % 5 + 1) / 2048.0f;
}
static std::vector<float> ref_weight(int Cout, int Cin, int taps) {
    std::vector<float> w((size_t)Cout * Cin * taps);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t) w[((size_t)co * Cin + ci) * taps + t] = enc(co, ci, t, Cin, taps);
    return w;
}

static void check_rows(int Cout, int Cin, int taps, int CinP) {
    const std::vector<float> w = ref_weight(Cout, Cin, taps);
    const size_t K = (size_t)taps * CinP;
    std::vector<float> f32(Cout * K, 0.f), tap(w.size(), 0.f);
    std::vector<f16> h16(Cout * K, (f16)0.f), sp(2 * Cout * K, (f16)0.f);
    const PackStat s32 = rs_pack_rows_f32(w.data(), Cout, Cin, taps, CinP, f32.data());
    const PackStat s16 = rs_pack_rows_f16(w.data(), Cout, Cin, taps, CinP, h16.data());
    const PackStat ssp = rs_pack_rows_split(w.data(), Cout, Cin, taps, CinP, sp.data());
    rs_pack_tap_major(w.data(), Cout, Cin, taps, tap.data());
    const float top = enc(Cout - 1, Cin - 1, taps - 1, Cin, taps);
    CHECK(s32.max_abs == top && s16.max_abs == top && ssp.max_abs == top);
    CHECK(!s32.non_finite && !s16.non_finite && !ssp.non_finite);
    for (int co = 0; co < Cout; ++co)
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < CinP; ++c) {
                const size_t k = (size_t)t * CinP + c;
                const float want = c < Cin ? enc(co, c, t, Cin, taps) : 0.f;   // (padded columns stay zero)
                CHECK(f32[co * K + k] == want);
                CHECK(h16[co * K + k] == (f16)f32[co * K + k]);
                const f16 hi = sp[co * 2 * K + k], lo = sp[co * 2 * K + K + k];
                CHECK(hi == h16[co * K + k]);
                CHECK((float)hi + (float)lo / 2048.0f == want);
                if (c < Cin) CHECK(tap[((size_t)t * Cin + c) * Cout + co] == want);
            }
    // what the packers report to the caller's policy: a negative extreme counts by magnitude, a non-finite value is flagged and not a maximum
    std::vector<float> v = w;
    v[1] = -4000.0f; v[2] = std::numeric_limits<float>::infinity(); v[3] = std::numeric_limits<float>::quiet_NaN();
    const PackStat sv = rs_pack_rows_f32(v.data(), Cout, Cin, taps, CinP, f32.data());
    CHECK(sv.non_finite && sv.max_abs == 4000.0f);
}

static void check_frag_major() {
    const int N = 16, K = 32;   // one (16-row block, k step)
    const std::vector<float> w = ref_weight(N, K, 1);
    std::vector<f16> o16((size_t)N * K), osp((size_t)2 * N * K);
    rs_pack_frag_major(w.data(), N, K, o16.data(), nullptr);
    rs_pack_frag_major(w.data(), N, K, nullptr, osp.data());
    for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
            const float want = enc(lane & 15, 8 * (lane >> 4) + e, 0, K, 1);
            CHECK(o16[lane * 8 + e] == (f16)want);
            CHECK(osp[lane * 8 + e] == (f16)want);   // hi plane, then the lo plane at +512
            CHECK((float)osp[lane * 8 + e] + (float)osp[512 + lane * 8 + e] / 2048.0f == want);
        }
}

static void check_bias_tables() {
    const int heads = 2;
    std::vector<float> table((size_t)225 * heads);
    for (int k = 0; k < 225; ++k)
        for (int h = 0; h < heads; ++h) table[(size_t)k * heads + h] = (float)(k + 256 * h);
    std::vector<float> bt((size_t)heads * 4096, -1.f), bn((size_t)heads * 4096, -1.f), bc((size_t)heads * 256, -1.f);
    rs_pack_bias_tables(table.data(), heads, bt.data(), nullptr);   // (each form on its own, as the model packer fills them)
    rs_pack_bias_tables(table.data(), heads, nullptr, bn.data());
    rs_pack_bias_compact(table.data(), heads, bc.data());
    CHECK(rs_rel_pos_index(0, 0) == 112 && rs_rel_pos_index(63, 0) == 224 && rs_rel_pos_index(0, 63) == 0);
    for (int h = 0; h < heads; ++h) {
        CHECK(bn[((size_t)h * 64 + 0) * 64 + 0] == 112.f + 256 * h);
        CHECK(bn[((size_t)h * 64 + 63) * 64 + 0] == 224.f + 256 * h);
        CHECK(bn[((size_t)h * 64 + 0) * 64 + 63] == 0.f + 256 * h);
        for (int i = 0; i < 64; ++i)
            for (int j = 0; j < 64; ++j) CHECK(bt[((size_t)h * 64 + j) * 64 + i] == bn[((size_t)h * 64 + i) * 64 + j]);
        for (int k = 0; k < 256; ++k) CHECK(bc[h * 256 + k] == (k < 225 ? table[(size_t)k * heads + h] * 1.44269504088896f : 0.f));
    }
}

static void check_derived() {
    // nearest x2 + an all-ones 3x3 kernel: how many taps land on each of the 2 x 2 source pixels, per output parity (py, px)
    const float ones[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    const float want[4][4] = {{1, 2, 2, 4}, {2, 1, 4, 2}, {2, 4, 1, 2}, {4, 2, 2, 1}};
    for (int q = 0; q < 4; ++q) {
        const std::vector<float> s = rs_subpixel_weight(ones, 1, q >> 1, q & 1);
        CHECK(s.size() == 4);
        for (int i = 0; i < 4; ++i) CHECK(s[i] == want[q][i]);
    }
    // [Wu W2 | Wu] and Wu b2 + bu with C = 2, E = 3, hidden = 2, by hand
    const float wu[6] = {1, 2, 3, 4, 5, 6}, w2[6] = {1, 0, 0, 1, 1, 1}, bu[2] = {0.5f, -1.f}, b2[3] = {1, 2, 3};
    const float fw[10] = {4, 5, 1, 2, 3, 10, 11, 4, 5, 6}, fb[2] = {14.5f, 31.f};
    const std::vector<float> gw = rs_unembed_fold_weight(wu, w2, 2, 3, 2), gb = rs_unembed_fold_bias(wu, bu, b2, 2, 3);
    CHECK(gw.size() == 10 && gb.size() == 2);
    for (int i = 0; i < 10; ++i) CHECK(gw[i] == fw[i]);
    for (int i = 0; i < 2; ++i) CHECK(gb[i] == fb[i]);
}

int main() {
    check_rows(5, 3, 9, 8);    // CinP 8 > Cin 3
    check_rows(4, 8, 4, 8);
    check_rows(16, 32, 1, 32);
    check_frag_major();
    check_bias_tables();
    check_derived();
    if (failures) { fprintf(stderr, "weight_pack_check: %d check(s) failed\n", failures); return 1; }
    printf("weight_pack_check: ok\n");
    return 0;
}
