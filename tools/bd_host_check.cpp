// bd_host_check.cpp -- stand-alone driver of fastbn_amd/csrc/hc_bd.h (the Bayesian Dirichlet arithmetic and
// its host twin of one family) for host sanitizer runs (no device, no libfastbn, never loaded into Python):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tools/bd_host_check.cpp -o bd_host_check && ./bd_host_check
// Checks, on tables generated here: D against the C library's lgammal within 1e-12 of the magnitudes, at
// and around the threshold and both parameter branches; ln 1 = +0.0; an all-zero table and a one-state
// child score exactly 0.0; the fold of a packed sub-group (width w >= q, offsets w/2 .. 1) gives the bits
// of the 64-lane fold; BDeu's score equivalence on a two-variable table.  Exits non-zero on a wrong answer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fastbn_amd/csrc/hc_bd.h"

static int g_fail = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                              \
        }                                                          \
    } while (0)

static bool SameBits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// the score of a table straight from the definition in long double, and the summed magnitudes
static void Plain(const std::vector<uint32_t> &t, int r, int q, double a_cell, double a_cfg, long double *sc, long double *mag) {
    *sc = *mag = 0;
    for (int j = 0; j < q; ++j) {
        uint32_t nj = 0;
        for (int k = 0; k < r; ++k) {
            const uint32_t n = t[(size_t)k * q + j];
            nj += n;
            if (!n) continue;
            *sc += lgammal((long double)a_cell + n) - lgammal((long double)a_cell);
            *mag += fabsl(lgammal((long double)a_cell + n)) + fabsl(lgammal((long double)a_cell));
        }
        if (!nj) continue;
        *sc -= lgammal((long double)a_cfg + nj) - lgammal((long double)a_cfg);
        *mag += fabsl(lgammal((long double)a_cfg + nj)) + fabsl(lgammal((long double)a_cfg));
    }
}

// what a packed sub-group of w lanes computes: partials of lanes 0 .. w-1, folded from w/2 down
static double PackedScore(const std::vector<uint32_t> &t, int r, int q, int w, double a_cell, double a_cfg) {
    const FbnBdPrior cell = fbn_bd_prior(a_cell), cfg = fbn_bd_prior(a_cfg);
    double p[kHcLanes];
    for (int l = 0; l < w; ++l) p[l] = fbn_bd_lane_partial(t.data(), r, q, l, cell, cfg);
    for (int off = w / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) p[l] += p[l + off];
    return p[0];
}

int main() {
    std::mt19937 rng(77);
    CHECK(SameBits(fbn_bd_ln(1.0), 0.0));
    // ---- D against lgammal
    double worst = 0;
    for (double a : {0x1p-40, 0x1p-32, 0x1p-20, 1.0 / 1024, 0.5, 1.0, 1.5, 15.999, 16.0, 256.0, 1e4, 1e9})
        for (uint32_t n : {1u, 2u, 3u, 15u, 16u, 17u, 1000u, 1u << 24, 0xffffffffu}) {
            const double d = fbn_bd_term(n, fbn_bd_prior(a));
            const long double hi = lgammal((long double)a + n), lo = lgammal((long double)a);
            const long double mag = fabsl(hi) + fabsl(lo);
            CHECK(fabsl(d - (hi - lo)) <= 1e-12L * mag);
            if (mag > 0) worst = fmax(worst, (double)(fabsl(d - (hi - lo)) / mag));
        }
    // ---- exact zeros
    double ll, sc;
    {
        const std::vector<uint32_t> zero(3 * 70, 0u);
        const std::vector<double> L{0.0};
        fbn_bd_family_host(zero.data(), 3, 70, L.data(), 1.0 / 210, 1.0 / 70, &ll, &sc);
        CHECK(SameBits(ll, 0.0) && SameBits(sc, 0.0));
    }
    // ---- random tables: the definition, the packed fold, a one-state child
    for (int it = 0; it < 400; ++it) {
        const int r = it % 7 == 0 ? 1 : 1 + (int)(rng() % 6), q = 1 + (int)(rng() % (it % 3 ? 32 : 200));
        std::vector<uint32_t> t((size_t)r * q);
        uint32_t N = 0;
        for (auto &c : t) N += c = rng() % 4 == 0 ? (uint32_t)(rng() % (it % 2 ? 40 : 5000)) : 0u;
        std::vector<double> L((size_t)N + 1);
        fbn_hc_fill_table(L.data(), N);
        for (int kind : {kBdKindBde, kBdKindK2}) {
            double a_cell, a_cfg;
            fbn_bd_alphas(kind, it % 5 ? 1.0 : 0.37, r, q, &a_cell, &a_cfg);
            fbn_bd_family_host(t.data(), r, q, L.data(), a_cell, a_cfg, &ll, &sc);
            long double ref, mag;
            Plain(t, r, q, a_cell, a_cfg, &ref, &mag);
            CHECK(fabsl(sc - ref) <= 1e-12L * mag);
            if (r == 1) CHECK(SameBits(sc, 0.0));
            double p[kHcLanes];
            for (int l = 0; l < kHcLanes; ++l) p[l] = fbn_hc_lane_partial(t.data(), r, q, l, L.data());
            CHECK(SameBits(ll, fbn_hc_fold(p)));
            if (q <= 32) {
                int w = 1;
                while (w < q) w *= 2;
                CHECK(SameBits(sc, PackedScore(t, r, q, w, a_cell, a_cfg)));
            }
        }
    }
    // ---- BDeu is score-equivalent: x -> y and y -> x on a 2 x 3 table
    {
        const uint32_t n[2][3] = {{120, 7, 33}, {4, 250, 61}};
        std::vector<uint32_t> yx(6), xy(6), x{160, 315}, y{124, 257, 94};  // tab[k * q + j]
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 3; ++j) yx[(size_t)j * 2 + i] = xy[(size_t)i * 3 + j] = n[i][j];
        std::vector<double> L(476);
        fbn_hc_fill_table(L.data(), 475);
        auto score = [&](const std::vector<uint32_t> &t, int r, int q) {
            double a_cell, a_cfg, l, s;
            fbn_bd_alphas(kBdKindBde, 2.0, r, q, &a_cell, &a_cfg);
            fbn_bd_family_host(t.data(), r, q, L.data(), a_cell, a_cfg, &l, &s);
            return s;
        };
        const double fwd = score(x, 2, 1) + score(yx, 3, 2), bwd = score(y, 3, 1) + score(xy, 2, 3);
        CHECK(fabs(fwd - bwd) <= 1e-12 * 8000);  // the lnGamma magnitudes of 475 samples sum to about 8,000
    }
    printf("%s: %d failures; worst |D - lgammal| / magnitudes = %.3g\n", g_fail ? "FAILED" : "ok", g_fail, worst);
    return g_fail ? 1 : 0;
}
