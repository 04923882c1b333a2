// blockcg_check.cpp -- stand-alone check of the host half of the coupled-block
// family (smfv::gram_host, smfv::small_solve_host and the argument checks
// smfv::blockcg_check_* in csrc/smfv_plan.cpp), built with
// -fsanitize=address,undefined by tests/test_blockcg_host.py: the two rules
// against plain restatements of include/smfv.h written here, on exactly sized
// heap blocks (a read outside a window is a sanitizer report), then every
// refusal with its message.  Exit 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "smfv_plan.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
            ++failures;                           \
        }                                         \
    } while (0)

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double rnd()  // uniform [-1, 1)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

bool same(double a, double b)
{
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// the column-dot rule of include/smfv.h on column i of x and column j of y
double rule(int m, const double *x, int64_t ldx, int i, const double *y, int64_t ldy, int j)
{
    double d = 0.0;
    for (int c = 0; c * 512 < m; ++c) {
        double v[32];
        for (int s = 0; s < 32; ++s) {
            v[s] = 0.0;
            for (int t = 0; t < 16; ++t) {
                const int64_t r = (int64_t)c * 512 + s + t * 32;
                if (r < m) v[s] = v[s] + x[r * ldx + i] * y[r * ldy + j];
            }
        }
        for (int h = 16; h >= 1; h /= 2)
            for (int s = 0; s < h; ++s) v[s] = v[s] + v[s + h];
        d = d + v[0];
    }
    return d;
}

// a window of exactly (rows - 1) * ld + cols doubles
std::vector<double> window(int rows, int cols, int64_t ld)
{
    std::vector<double> b(rows > 0 ? (size_t)((int64_t)(rows - 1) * ld + cols) : 0, std::numeric_limits<double>::quiet_NaN());
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) b[(size_t)(i * ld + j)] = rnd();
    return b;
}

void check_gram(int m, int Kx, int Ky, int pad)
{
    const int64_t ldx = Kx + pad, ldy = Ky + 2 * pad, ldg = Ky + pad;
    std::vector<double> X = window(m, Kx, ldx), Y = window(m, Ky, ldy), G = window(Kx, Ky, ldg);
    if (m > 40) {
        X[(size_t)(5 * ldx)] = std::numeric_limits<double>::infinity();
        X[(size_t)(38 * ldx)] = -std::numeric_limits<double>::infinity();
        Y[(size_t)(7 * ldy + Ky - 1)] = std::numeric_limits<double>::quiet_NaN();
    }
    smfv::gram_host(m, Kx, Ky, X.data(), ldx, Y.data(), ldy, G.data(), ldg);
    for (int i = 0; i < Kx; ++i)
        for (int j = 0; j < Ky; ++j) {
            const double got = G[(size_t)(i * ldg + j)], want = rule(m, X.data(), ldx, i, Y.data(), ldy, j);
            CHECK(same(got, want), "gram m %d K %d %d pad %d entry (%d, %d): %a, want %a", m, Kx, Ky, pad, i, j, got, want);
            CHECK(!(got == 0.0 && std::signbit(got)), "gram m %d entry (%d, %d) is -0.0", m, i, j);
        }
    if (Kx == Ky) {  // X may be Y
        smfv::gram_host(m, Kx, Kx, X.data(), ldx, X.data(), ldx, G.data(), ldg);
        for (int i = 0; i < Kx; ++i)
            CHECK(same(G[(size_t)(i * ldg + i)], rule(m, X.data(), ldx, i, X.data(), ldx, i)), "X is Y, m %d diagonal %d", m, i);
    }
}

// the small-solve rule of include/smfv.h, restated row by row
void check_small_solve(int K, int N, int pad, bool in_place)
{
    const int64_t ldg = K + pad, ldh = N + pad, ldc = in_place ? ldh : N + 2 * pad;
    std::vector<double> G = window(K, K, ldg), H = window(K, N, ldh), C = window(K, N, ldc);
    for (int i = 0; i < K; ++i) G[(size_t)(i * ldg + i)] = (i % 3 ? 1.0 : -1.0) * (K + 1.0);
    std::vector<double> W((size_t)K * K), T((size_t)K * N);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) W[(size_t)(i * K + j)] = G[(size_t)(i * ldg + j)];
    for (int i = 0; i < K; ++i)
        for (int k = 0; k < i; ++k) {
            W[(size_t)(i * K + k)] = W[(size_t)(i * K + k)] / W[(size_t)(k * K + k)];
            for (int j = k + 1; j < K; ++j) {
                const double p = W[(size_t)(i * K + k)] * W[(size_t)(k * K + j)];
                W[(size_t)(i * K + j)] = W[(size_t)(i * K + j)] - p;
            }
        }
    for (int n = 0; n < N; ++n) {
        for (int i = 0; i < K; ++i) {
            double s = H[(size_t)(i * ldh + n)];
            for (int k = 0; k < i; ++k) {
                const double p = W[(size_t)(i * K + k)] * T[(size_t)(k * N + n)];
                s = s - p;
            }
            T[(size_t)(i * N + n)] = s;
        }
        for (int i = K - 1; i >= 0; --i) {
            double s = T[(size_t)(i * N + n)];
            for (int k = i + 1; k < K; ++k) {
                const double p = W[(size_t)(i * K + k)] * T[(size_t)(k * N + n)];
                s = s - p;
            }
            T[(size_t)(i * N + n)] = s / W[(size_t)(i * K + i)];
        }
    }
    const std::vector<double> G0 = G;
    double *out = in_place ? H.data() : C.data();
    smfv::small_solve_host(K, N, G.data(), ldg, H.data(), ldh, out, ldc);
    for (int i = 0; i < K; ++i)
        for (int n = 0; n < N; ++n)
            CHECK(same(out[(size_t)(i * ldc + n)], T[(size_t)(i * N + n)]), "small_solve K %d N %d pad %d in place %d entry (%d, %d)", K, N,
                  pad, (int)in_place, i, n);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) CHECK(same(G[(size_t)(i * ldg + j)], G0[(size_t)(i * ldg + j)]), "small_solve modified G (%d, %d)", i, j);
}

void refused(bool ok, const std::string &err, const char *word, const char *what)
{
    CHECK(!ok, "%s was accepted", what);
    CHECK(err.find(word) != std::string::npos, "%s: message '%s' lacks '%s'", what, err.c_str(), word);
}

void check_refusals()
{
    std::vector<double> a(8192), b(8192), c(8192), g(128 * 128), s(64);
    const int m = 20, K = 8;
    std::string e;
    double *A = a.data(), *B = b.data(), *Cb = c.data(), *Gm = g.data(), *S = s.data();

    CHECK(smfv::blockcg_check_gram(m, K, 5, A, K, B, 7, Gm, 5, S, &e), "valid gram refused: %s", e.c_str());
    CHECK(smfv::blockcg_check_gram(m, K, K, A, K, A, K, Gm, K, S, &e), "gram with X is Y refused: %s", e.c_str());
    CHECK(smfv::blockcg_check_gram(0, K, K, nullptr, K, nullptr, K, Gm, K, S, &e), "gram with m = 0 and null blocks refused");
    refused(smfv::blockcg_check_gram(m, 0, K, A, K, B, K, Gm, K, S, &e), e, "Kx = 0", "Kx = 0");
    refused(smfv::blockcg_check_gram(m, K, 129, A, K, B, 129, Gm, 129, S, &e), e, "Ky = 129", "Ky = 129");
    refused(smfv::blockcg_check_gram(-1, K, K, A, K, B, K, Gm, K, S, &e), e, "m = -1", "m = -1");
    refused(smfv::blockcg_check_gram(m, K, K, A, K - 1, B, K, Gm, K, S, &e), e, "leading dimension of X", "ldx");
    refused(smfv::blockcg_check_gram(m, K, K, A, K, B, K - 1, Gm, K, S, &e), e, "leading dimension of Y", "ldy");
    refused(smfv::blockcg_check_gram(m, K, K, A, K, B, K, Gm, K - 1, S, &e), e, "leading dimension of G", "ldg");
    refused(smfv::blockcg_check_gram(m, K, K, nullptr, K, B, K, Gm, K, S, &e), e, "null X", "null X");
    refused(smfv::blockcg_check_gram(m, K, K, A, K, nullptr, K, Gm, K, S, &e), e, "null Y", "null Y");
    refused(smfv::blockcg_check_gram(m, K, K, A, K, B, K, nullptr, K, S, &e), e, "null G", "null G");
    refused(smfv::blockcg_check_gram(m, K, K, A, K, B, K, Gm, K, nullptr, &e), e, "null workspace", "null workspace");

    auto mul = [&](int Kx, int Ky, int flags, const double *X, int64_t ldx, const double *C, int64_t ldc, const double *Z,
                   int64_t ldz, const double *Y, int64_t ldy) {
        return smfv::blockcg_check_block_mul(m, Kx, Ky, flags, X, ldx, C, ldc, Z, ldz, Y, ldy, &e);
    };
    CHECK(mul(K, 5, 1, A, K, Gm, 5, B, 5, Cb, 5), "valid block_mul refused: %s", e.c_str());
    CHECK(mul(K, 5, 0, A, K, Gm, 5, nullptr, 0, Cb, 5), "block_mul without Z refused: %s", e.c_str());
    CHECK(mul(K, K, 0, A, K, Gm, K, B, K, B, K), "Y == Z refused: %s", e.c_str());
    CHECK(mul(K, K, 0, A, K, Gm, K, B, K, A, K), "Y == X refused: %s", e.c_str());
    CHECK(mul(K, K, 0, A, K, Gm, K, A, K, A, K), "Y == X == Z refused: %s", e.c_str());
    CHECK(mul(K, K, 0, A, 3 * K, Gm, K, A + K, 3 * K, A + 2 * K, 3 * K), "column windows refused: %s", e.c_str());
    CHECK(smfv::blockcg_check_block_mul(0, K, K, 0, nullptr, K, Gm, K, nullptr, K, nullptr, K, &e), "m = 0 with null blocks refused");
    refused(mul(0, K, 0, A, K, Gm, K, B, K, Cb, K), e, "Kx = 0", "Kx = 0");
    refused(mul(K, 200, 0, A, K, Gm, 200, B, 200, Cb, 200), e, "Ky = 200", "Ky = 200");
    refused(smfv::blockcg_check_block_mul(-2, K, K, 0, A, K, Gm, K, B, K, Cb, K, &e), e, "m = -2", "m = -2");
    refused(mul(K, K, 2, A, K, Gm, K, B, K, Cb, K), e, "unknown flags 2", "flags 2");
    refused(mul(K, K, 0, A, K - 1, Gm, K, B, K, Cb, K), e, "leading dimension of X", "ldx");
    refused(mul(K, K, 0, A, K, Gm, K - 1, B, K, Cb, K), e, "leading dimension of C", "ldc");
    refused(mul(K, K, 0, A, K, Gm, K, B, K - 1, Cb, K), e, "leading dimension of Z", "ldz");
    refused(mul(K, K, 0, A, K, Gm, K, B, K, Cb, K - 1), e, "leading dimension of Y", "ldy");
    refused(mul(K, K, 0, nullptr, K, Gm, K, B, K, Cb, K), e, "null X", "null X");
    refused(mul(K, K, 0, A, K, nullptr, K, B, K, Cb, K), e, "null C", "null C");
    refused(mul(K, K, 0, A, K, Gm, K, B, K, nullptr, K), e, "null Y", "null Y");
    refused(mul(K, 5, 0, A, K, Gm, 5, B, 5, A, 5), e, "X and Y overlap", "Y == X with Kx != Ky");
    refused(mul(K, K, 0, A, K, Gm, K, B, K, A + 3 * K, K), e, "X and Y overlap", "Y three rows into X");
    refused(mul(K, K, 0, A, K, Gm, K, B, K, A, K + 1), e, "X and Y overlap", "Y == X with another ld");
    refused(mul(K, K, 0, A, K, Gm, K, B, K, B + 1, K), e, "Z and Y overlap", "Y one double into Z");
    refused(mul(K, K, 0, A, K, Gm, K, B, K + 2, B, K), e, "Z and Y overlap", "Y == Z with another ld");
    refused(mul(K, K, 0, A, K, Cb + K, K, B, K, Cb, K), e, "C and Y overlap", "C inside Y");
    refused(mul(K, 5, 0, A, 2 * K, Gm, 5, B, 5, A + K - 1, 2 * K), e, "X and Y overlap", "windows sharing a column");

    auto sol = [&](int Ks, int N, const double *G, int64_t ldg, const double *H, int64_t ldh, const double *C, int64_t ldc) {
        return smfv::blockcg_check_small_solve(Ks, N, G, ldg, H, ldh, C, ldc, &e);
    };
    CHECK(sol(K, 5, Gm, K, A, 5, B, 5), "valid small_solve refused: %s", e.c_str());
    CHECK(sol(K, 5, Gm, K, A, 7, A, 7), "C == H refused: %s", e.c_str());
    refused(sol(0, 5, Gm, K, A, 5, B, 5), e, "K = 0", "K = 0");
    refused(sol(129, 5, Gm, 129, A, 5, B, 5), e, "K = 129", "K = 129");
    refused(sol(K, 0, Gm, K, A, 5, B, 5), e, "N = 0", "N = 0");
    refused(sol(K, 129, Gm, K, A, 129, B, 129), e, "N = 129", "N = 129");
    refused(sol(K, 5, Gm, K - 1, A, 5, B, 5), e, "leading dimension of G", "ldg");
    refused(sol(K, 5, Gm, K, A, 4, B, 5), e, "leading dimension of H", "ldh");
    refused(sol(K, 5, Gm, K, A, 5, B, 4), e, "leading dimension of C", "ldc");
    refused(sol(K, 5, nullptr, K, A, 5, B, 5), e, "null G", "null G");
    refused(sol(K, 5, Gm, K, nullptr, 5, B, 5), e, "null H", "null H");
    refused(sol(K, 5, Gm, K, A, 5, nullptr, 5), e, "null C", "null C");
    refused(sol(K, 5, Gm, K, A, 5, Gm + 8, 5), e, "G and C overlap", "C inside G");
    refused(sol(K, 5, Gm, K, A, 5, A + 2, 5), e, "H and C overlap", "C two doubles into H");
    refused(sol(K, 5, Gm, K, A, 5, A, 6), e, "H and C overlap", "C == H with another ld");
}

}  // namespace

int main()
{
    for (int m : {0, 1, 31, 32, 33, 511, 512, 513, 1025})
        for (int pad : {0, 3}) {
            check_gram(m, 1, 1, pad);
            check_gram(m, 3, 8, pad);
            check_gram(m, 5, 5, pad);
        }
    check_gram(600, 33, 31, 1);
    for (int K : {1, 2, 3, 8, 31, 32, 33})
        for (int N : {1, K, 40}) {
            check_small_solve(K, N, 0, false);
            check_small_solve(K, N, 2, false);
            check_small_solve(K, N, 1, true);
        }
    check_refusals();
    if (failures) {
        std::fprintf(stderr, "blockcg_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("blockcg_check: OK\n");
    return 0;
}
