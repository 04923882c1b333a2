// blockvec_check.cpp -- stand-alone check of the host half of the block-vector
// family (smfv::coldot_host and the argument checks smfv::blockvec_check_* in
// csrc/smfv_plan.cpp), built with -fsanitize=address,undefined by
// tests/test_blockvec_host.py: the rule against a plain restatement of
// include/smfv.h written here, on exactly sized heap blocks (a read outside the
// K columns of a padded block, or past the last row, is a sanitizer report),
// then every refusal with its message.  Exit 0 and no sanitizer report = pass.
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

// the rule of include/smfv.h, restated: chunks of 512, 32 strands, the tree
double rule(int m, const double *x, int64_t ldx, const double *y, int64_t ldy, int j)
{
    double d = 0.0;
    for (int c = 0; c * 512 < m; ++c) {
        double v[32];
        for (int s = 0; s < 32; ++s) {
            v[s] = 0.0;
            for (int t = 0; t < 16; ++t) {
                const int64_t r = (int64_t)c * 512 + s + t * 32;
                if (r < m) v[s] = v[s] + x[r * ldx + j] * y[r * ldy + j];
            }
        }
        for (int h = 16; h >= 1; h /= 2)
            for (int s = 0; s < h; ++s) v[s] = v[s] + v[s + h];
        d = d + v[0];
    }
    return d;
}

bool same(double a, double b)
{
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// a block of exactly (m - 1) * ld + K doubles: nothing after the last row's K columns
std::vector<double> block(int m, int K, int64_t ld)
{
    std::vector<double> b(m > 0 ? (size_t)((int64_t)(m - 1) * ld + K) : 0, std::numeric_limits<double>::quiet_NaN());
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < K; ++j) b[(size_t)(i * ld + j)] = rnd();
    return b;
}

void check_rule(int m, int K, int64_t ldx, int64_t ldy)
{
    std::vector<double> X = block(m, K, ldx), Y = block(m, K, ldy), out((size_t)K, -7.0);
    if (m > 40 && K > 2) {  // special values in three columns
        X[(size_t)(5 * ldx + 0)] = std::numeric_limits<double>::infinity();
        X[(size_t)(38 * ldx + 0)] = -std::numeric_limits<double>::infinity();
        X[(size_t)(7 * ldx + 1)] = std::numeric_limits<double>::quiet_NaN();
        for (int i = 0; i < m; ++i) X[(size_t)(i * ldx + 2)] = -0.0;
    }
    smfv::coldot_host(m, K, X.data(), ldx, Y.data(), ldy, out.data());
    for (int j = 0; j < K; ++j) {
        const double want = rule(m, X.data(), ldx, Y.data(), ldy, j);
        CHECK(same(out[(size_t)j], want), "m %d K %d ld %lld %lld column %d: %a, want %a", m, K, (long long)ldx, (long long)ldy,
              j, out[(size_t)j], want);
        CHECK(!(out[(size_t)j] == 0.0 && std::signbit(out[(size_t)j])), "m %d column %d is -0.0", m, j);
    }
    // X may be Y
    smfv::coldot_host(m, K, X.data(), ldx, X.data(), ldx, out.data());
    for (int j = 0; j < K; ++j) CHECK(same(out[(size_t)j], rule(m, X.data(), ldx, X.data(), ldx, j)), "X is Y, m %d column %d", m, j);
}

void refused(bool ok, const std::string &err, const char *word, const char *what)
{
    CHECK(!ok, "%s was accepted", what);
    CHECK(err.find(word) != std::string::npos, "%s: message '%s' lacks '%s'", what, err.c_str(), word);
}

void check_refusals()
{
    std::vector<double> a(4096), b(4096), c(4096), d(4096), s(64);
    const int m = 20, K = 8;
    std::string e;
    CHECK(smfv::blockvec_check_coldot(m, K, a.data(), K, b.data(), K + 3, s.data(), s.data(), &e), "valid coldot refused: %s", e.c_str());
    CHECK(smfv::blockvec_check_coldot(0, K, nullptr, K, nullptr, K, s.data(), s.data(), &e), "m = 0 with null blocks refused");
    refused(smfv::blockvec_check_coldot(m, 0, a.data(), K, b.data(), K, s.data(), s.data(), &e), e, "K = 0", "K = 0");
    refused(smfv::blockvec_check_coldot(-1, K, a.data(), K, b.data(), K, s.data(), s.data(), &e), e, "m = -1", "m = -1");
    refused(smfv::blockvec_check_coldot(m, K, a.data(), K - 1, b.data(), K, s.data(), s.data(), &e), e, "leading dimension of X", "ldx < K");
    refused(smfv::blockvec_check_coldot(m, K, a.data(), K, b.data(), 0, s.data(), s.data(), &e), e, "leading dimension of Y", "ldy < K");
    refused(smfv::blockvec_check_coldot(m, K, nullptr, K, b.data(), K, s.data(), s.data(), &e), e, "null X", "null X");
    refused(smfv::blockvec_check_coldot(m, K, a.data(), K, nullptr, K, s.data(), s.data(), &e), e, "null Y", "null Y");
    refused(smfv::blockvec_check_coldot(m, K, a.data(), K, b.data(), K, nullptr, s.data(), &e), e, "null out", "null out");
    refused(smfv::blockvec_check_coldot(m, K, a.data(), K, b.data(), K, s.data(), nullptr, &e), e, "null workspace", "null workspace");

    CHECK(smfv::blockvec_check_update("col_axpy", m, K, s.data(), 3, a.data(), K, a.data(), K, &e), "in-place axpy refused: %s", e.c_str());
    refused(smfv::blockvec_check_update("col_axpy", m, K, nullptr, 0, a.data(), K, b.data(), K, &e), e, "null num", "null num");
    refused(smfv::blockvec_check_update("col_xpay", m, K, s.data(), 4, a.data(), K, b.data(), K, &e), e, "unknown flags 4", "flags 4");
    refused(smfv::blockvec_check_update("col_xpay", m, K, s.data(), 0, a.data(), K, nullptr, K, &e), e, "col_xpay: null Y", "null Y");
    refused(smfv::blockvec_check_update("col_axpy", m, -3, s.data(), 0, a.data(), K, b.data(), K, &e), e, "K = -3", "K = -3");

    auto pcg = [&](const double *P, int64_t ldp, const double *Q, int64_t ldq, const double *X, int64_t ldx, const double *R,
                   int64_t ldr) {
        return smfv::blockvec_check_pcg_update(m, K, s.data(), 2, P, ldp, Q, ldq, X, ldx, R, ldr, s.data(), s.data(), &e);
    };
    CHECK(pcg(a.data(), K, b.data(), K, c.data(), K, d.data(), K), "valid pcg_update refused: %s", e.c_str());
    // four disjoint column windows of one buffer
    CHECK(pcg(a.data(), 4 * K, a.data() + K, 4 * K, a.data() + 2 * K, 4 * K, a.data() + 3 * K, 4 * K), "column windows refused: %s", e.c_str());
    refused(pcg(a.data(), K, b.data(), K, c.data(), K, c.data(), K), e, "X and R overlap", "X is R");
    refused(pcg(a.data(), K, a.data(), K, c.data(), K, d.data(), K), e, "P and Q overlap", "P is Q");
    refused(pcg(a.data(), K, b.data(), K, c.data(), K, c.data() + 3 * K, K), e, "X and R overlap", "R three rows into X");
    refused(pcg(a.data(), K, a.data() + 5, K, c.data(), K, d.data(), K), e, "P and Q overlap", "Q five doubles into P");
    refused(pcg(a.data(), 2 * K, b.data(), K, c.data(), K, a.data() + K - 1, 2 * K), e, "P and R overlap", "windows sharing a column");
    refused(pcg(a.data(), 2 * K, b.data(), K, c.data(), K, a.data() + K + 1, 2 * K), e, "P and R overlap", "a window wrapping into the next row");
    refused(pcg(a.data(), K, b.data(), K, c.data(), K + 1, c.data() + 2, K + 3), e, "X and R overlap", "ranges meeting under two leading dimensions");
    refused(pcg(nullptr, K, b.data(), K, c.data(), K, d.data(), K), e, "null P", "null P");
    refused(pcg(a.data(), K, b.data(), K - 1, c.data(), K, d.data(), K), e, "leading dimension of Q", "ldq < K");
    refused(smfv::blockvec_check_pcg_update(m, K, s.data(), 0, a.data(), K, b.data(), K, c.data(), K, d.data(), K, nullptr, s.data(), &e), e,
            "null rr", "null rr");
    refused(smfv::blockvec_check_pcg_update(m, K, s.data(), 8, a.data(), K, b.data(), K, c.data(), K, d.data(), K, s.data(), s.data(), &e), e,
            "unknown flags", "flags 8");
    CHECK(smfv::coldot_chunks(0) == 1 && smfv::coldot_chunks(1) == 1 && smfv::coldot_chunks(512) == 1 && smfv::coldot_chunks(513) == 2,
          "coldot_chunks");
}

}  // namespace

int main()
{
    for (int m : {0, 1, 31, 32, 33, 511, 512, 513, 1025, 1500})
        for (int K : {1, 3, 8}) {
            check_rule(m, K, K, K);
            check_rule(m, K, K + 3, K + 1);
        }
    check_refusals();
    if (failures) {
        std::fprintf(stderr, "blockvec_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("blockvec_check: OK\n");
    return 0;
}
