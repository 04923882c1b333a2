// transpose_check.cpp -- stand-alone check of smfv::csr_transpose
// (csrc/smfv_plan.cpp), built with -fsanitize=address,undefined by
// tests/test_transpose_host.py: generated patterns (unsorted rows, repeated
// columns, empty rows and columns, long rows, degenerate shapes), each result
// re-checked here against a plain stable sort; bad inputs must be refused
// without a write.  Exit 0 and no sanitizer report = pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "smfv_plan.h"

namespace {

struct Pattern {
    int m = 0, n = 0;
    std::vector<int> rp, ci;
};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// rows of length (r * 7 + 3) % maxlen, every 5th row empty, columns from a
// band or (every 11th row) from all of n, every 3rd row repeats its first
// column at its end; columns with c % skip == skip - 1 are never used
Pattern make(int m, int n, int maxlen, int skip)
{
    Pattern P;
    P.m = m;
    P.n = n;
    P.rp.assign((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) {
        int L = (n == 0 || r % 5 == 4) ? 0 : (r * 7 + 3) % maxlen;
        const size_t first = P.ci.size();
        for (int k = 0; k < L; ++k) {
            int c = r % 11 == 0 ? (int)(rnd() % (uint32_t)n) : (int)(((int64_t)r * n / std::max(m, 1) + rnd() % 17) % n);
            if (skip > 1 && c % skip == skip - 1) c -= 1;
            if (c < 0) c = 0;
            P.ci.push_back(c);
        }
        if (L > 1 && r % 3 == 0) P.ci.push_back(P.ci[first]);
        P.rp[(size_t)r + 1] = (int)P.ci.size();
    }
    return P;
}

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

void check_ok(const Pattern &P, const char *name)
{
    const size_t nnz = P.ci.size();
    std::vector<int> t_rp((size_t)P.n + 1, -7), t_ci(nnz, -7), t_perm(nnz, -7);
    std::string err;
    const bool ok = smfv::csr_transpose(P.m, P.n, P.rp.data(), P.ci.data(), t_rp.data(), t_ci.data(), t_perm.data(), &err);
    CHECK(ok, "%s: refused: %s", name, err.c_str());
    if (!ok) return;
    // the expected result: a stable sort of the entries by column
    std::vector<int> order(nnz), row(nnz);
    std::iota(order.begin(), order.end(), 0);
    for (int r = 0; r < P.m; ++r)
        for (int j = P.rp[(size_t)r]; j < P.rp[(size_t)r + 1]; ++j) row[(size_t)j] = r;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return P.ci[(size_t)a] < P.ci[(size_t)b]; });
    std::vector<int> cnt((size_t)P.n + 1, 0);
    for (size_t j = 0; j < nnz; ++j) ++cnt[(size_t)P.ci[j] + 1];
    for (int c = 0; c < P.n; ++c) cnt[(size_t)c + 1] += cnt[(size_t)c];
    CHECK(t_rp == cnt, "%s: row_ptr differs", name);
    CHECK(t_perm == order, "%s: perm differs", name);
    bool rows_ok = true;
    for (size_t j = 0; j < nnz; ++j) rows_ok = rows_ok && t_ci[j] == row[(size_t)order[j]];
    CHECK(rows_ok, "%s: col_idx differs", name);
}

void check_refused(Pattern P, const char *name)
{
    const size_t nnz = P.ci.size();
    std::vector<int> t_rp((size_t)P.n + 1, -7), t_ci(nnz, -7), t_perm(nnz, -7);
    std::string err;
    const bool ok = smfv::csr_transpose(P.m, P.n, P.rp.data(), P.ci.data(), t_rp.data(), t_ci.data(), t_perm.data(), &err);
    CHECK(!ok, "%s: accepted", name);
    CHECK(!err.empty(), "%s: no message", name);
    // refused before the scatter: the entry arrays are untouched
    CHECK(std::all_of(t_ci.begin(), t_ci.end(), [](int v) { return v == -7; }), "%s: wrote col_idx", name);
    CHECK(std::all_of(t_perm.begin(), t_perm.end(), [](int v) { return v == -7; }), "%s: wrote perm", name);
}

}  // namespace

int main()
{
    check_ok(make(3000, 2400, 41, 1), "3000x2400");
    check_ok(make(2400, 3000, 41, 7), "2400x3000 with empty columns");
    check_ok(make(500, 700, 1300, 3), "long rows");
    check_ok(make(1, 500, 300, 1), "1x500");
    check_ok(make(500, 1, 5, 1), "500x1");
    check_ok(make(1, 1, 2, 1), "1x1");
    check_ok(make(2000, 3, 5, 1), "2000x3");
    check_ok(make(0, 0, 1, 1), "0x0");
    check_ok(make(0, 9, 1, 1), "0x9");
    check_ok(make(9, 0, 4, 1), "9x0");
    {
        Pattern P = make(40, 30, 1, 1);  // no entries at all
        check_ok(P, "40x30 empty");
    }
    {
        Pattern P = make(300, 200, 23, 1);
        Pattern Q = P;
        Q.ci[Q.ci.size() / 2] = Q.n;
        check_refused(Q, "column n");
        Q = P;
        Q.ci[0] = -1;
        check_refused(Q, "column -1");
        Q = P;
        Q.ci.back() = 0x7fffffff;
        check_refused(Q, "column INT_MAX");
        Q = P;
        Q.rp[0] = 1;
        check_refused(Q, "row_ptr[0] != 0");
        Q = P;
        std::swap(Q.rp[10], Q.rp[11]);
        if (Q.rp[10] != Q.rp[11]) check_refused(Q, "row_ptr decreases");
    }
    {
        std::string err;
        int one = 0;
        CHECK(!smfv::csr_transpose(-1, 3, &one, nullptr, &one, nullptr, nullptr, &err), "m = -1 accepted");
        CHECK(!smfv::csr_transpose(1, 3, nullptr, nullptr, &one, nullptr, nullptr, &err), "null row_ptr accepted");
        CHECK(!smfv::csr_transpose(-1, 3, &one, nullptr, &one, nullptr, nullptr, nullptr), "m = -1 accepted (no err)");
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("transpose_check: OK\n");
    return 0;
}
