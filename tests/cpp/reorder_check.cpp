// reorder_check.cpp -- stand-alone check of the multicolour ordering and the
// symmetric renumbering (smfv::order_multicolor, smfv::csr_permute_sym,
// smfv::check_permutation in csrc/smfv_plan.cpp), built with
// -fsanitize=address,undefined by tests/test_reorder_host.py: generated
// patterns (unsorted rows, repeated columns, empty rows, one-sided entries,
// degenerate shapes); each result is re-checked here against a plain
// restatement of the two rules of include/smfv.h, and the renumbered pattern's
// levels against the colour count; bad inputs must be refused with a message.
// Exit 0 and no sanitizer report = pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "smfv_plan.h"

namespace {

struct Pattern {
    int m = 0;
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

// rows of (r * 7 + 3) % maxlen columns from a band of +-band around r or
// (every 11th row) from all of m, repeats allowed, unsorted; every 5th row
// empty; with_diag adds the diagonal entry at a random place
Pattern make(int m, int maxlen, int band, bool with_diag)
{
    Pattern P;
    P.m = m;
    P.rp.assign((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) {
        const int L = r % 5 == 4 ? 0 : (r * 7 + 3) % maxlen;
        std::vector<int> row;
        for (int k = 0; k < L; ++k) {
            int c = r % 11 == 0 ? (int)(rnd() % (uint32_t)m) : r - band + (int)(rnd() % (uint32_t)(2 * band + 1));
            row.push_back(std::min(std::max(c, 0), m - 1));
        }
        if (with_diag) row.insert(row.begin() + (row.empty() ? 0 : (long)(rnd() % row.size())), r);
        P.ci.insert(P.ci.end(), row.begin(), row.end());
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
    const int m = P.m;
    const int64_t nnz = P.rp[(size_t)m];
    std::string err;
    std::vector<int> perm((size_t)m, -7), color((size_t)m, -7);
    int nc = -7;
    const bool ok = smfv::order_multicolor(m, P.rp.data(), P.ci.data(), 0, perm.data(), color.data(), &nc, &err);
    CHECK(ok, "%s: ordering refused: %s", name, err.c_str());
    if (!ok) return;
    // the rule, restated with a set of neighbours per row
    std::vector<std::set<int>> nb((size_t)m);
    for (int i = 0; i < m; ++i)
        for (int j = P.rp[(size_t)i]; j < P.rp[(size_t)i + 1]; ++j) {
            const int c = P.ci[(size_t)j];
            if (c != i) nb[(size_t)i].insert(c), nb[(size_t)c].insert(i);
        }
    std::vector<int> want((size_t)m, -1);
    int want_nc = 0;
    for (int i = 0; i < m; ++i) {
        std::set<int> taken;
        for (int j : nb[(size_t)i])
            if (j < i) taken.insert(want[(size_t)j]);
        int c = 0;
        while (taken.count(c)) ++c;
        want[(size_t)i] = c;
        want_nc = std::max(want_nc, c + 1);
    }
    CHECK(color == want && nc == want_nc, "%s: colours differ from the rule (%d / %d colours)", name, nc, want_nc);
    std::vector<int> by((size_t)m);
    for (int i = 0; i < m; ++i) by[(size_t)i] = i;
    std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return want[(size_t)a] < want[(size_t)b]; });
    CHECK(perm == by, "%s: perm is not the rows by (colour, row)", name);
    // without the colour array: the same perm
    std::vector<int> perm2((size_t)m, -7);
    int nc2 = -7;
    CHECK(smfv::order_multicolor(m, P.rp.data(), P.ci.data(), 0, perm2.data(), nullptr, &nc2, &err) && perm2 == perm && nc2 == nc,
          "%s: the ordering without a colour array differs", name);

    // the renumbering
    std::vector<int> b_rp((size_t)m + 1, -7), b_ci((size_t)nnz, -7), vperm((size_t)nnz, -7);
    const bool pk = smfv::csr_permute_sym(m, P.rp.data(), P.ci.data(), perm.data(), b_rp.data(), b_ci.data(), vperm.data(), &err);
    CHECK(pk, "%s: renumbering refused: %s", name, err.c_str());
    if (!pk) return;
    std::vector<int> inv((size_t)m);
    for (int i = 0; i < m; ++i) inv[(size_t)perm[(size_t)i]] = i;
    CHECK(b_rp[0] == 0 && b_rp[(size_t)m] == nnz, "%s: b_row_ptr ends", name);
    int64_t d = 0;
    for (int i = 0; i < m; ++i) {
        const int r = perm[(size_t)i];
        for (int j = P.rp[(size_t)r]; j < P.rp[(size_t)r + 1]; ++j, ++d) {
            CHECK(vperm[(size_t)d] == j && b_ci[(size_t)d] == inv[(size_t)P.ci[(size_t)j]], "%s: entry %lld of B", name, (long long)d);
            // two rows of one colour never couple
            CHECK(b_ci[(size_t)d] == i || color[(size_t)perm[(size_t)b_ci[(size_t)d]]] != color[(size_t)r], "%s: entry %lld joins one colour", name,
                  (long long)d);
        }
        CHECK(b_rp[(size_t)i + 1] == d, "%s: b_row_ptr[%d]", name, i + 1);
    }
    // the point: both triangles of B have at most nc levels
    for (int flags : {0, smfv::TRSM_UPPER}) {
        std::vector<int> lev((size_t)m), order((size_t)m);
        int nlev = -7;
        CHECK(smfv::trsm_levels(m, b_rp.data(), b_ci.data(), flags, lev.data(), order.data(), &nlev, &err), "%s: trsm_levels refused", name);
        CHECK(nlev <= nc, "%s: %d levels with %d colours (flags %d)", name, nlev, nc, flags);
    }
}

void check_refused(const Pattern &P, const char *word, const char *name)
{
    const int m = P.m;
    std::vector<int> perm((size_t)m + 1, -7), color((size_t)m + 1, -7), b_rp((size_t)m + 1, -7), b_ci(P.ci.size() + 1, -7), vp(P.ci.size() + 1, -7);
    std::vector<int> ident((size_t)m);
    for (int i = 0; i < m; ++i) ident[(size_t)i] = i;
    int nc = -7;
    std::string err;
    CHECK(!smfv::order_multicolor(m, P.rp.data(), P.ci.data(), 0, perm.data(), color.data(), &nc, &err), "%s: ordering accepted", name);
    CHECK(err.find(word) != std::string::npos && err.rfind("order", 0) == 0, "%s: message '%s' lacks '%s'", name, err.c_str(), word);
    CHECK(nc == -7, "%s: ncolors written on refusal", name);
    err.clear();
    CHECK(!smfv::csr_permute_sym(m, P.rp.data(), P.ci.data(), ident.data(), b_rp.data(), b_ci.data(), vp.data(), &err), "%s: renumbering accepted", name);
    CHECK(err.find(word) != std::string::npos && err.rfind("permute", 0) == 0, "%s: message '%s' lacks '%s'", name, err.c_str(), word);
    CHECK(!smfv::order_multicolor(m, P.rp.data(), P.ci.data(), 0, perm.data(), color.data(), &nc, nullptr), "%s: accepted (no err)", name);
}

}  // namespace

int main()
{
    check_ok(make(400, 23, 9, true), "band400");
    check_ok(make(401, 23, 9, false), "band401_no_diag");
    check_ok(make(1000, 60, 40, true), "band1000");
    check_ok(make(64, 64, 64, false), "dense64");
    check_ok(make(1, 1, 1, true), "m1");
    {
        Pattern P;  // m = 0
        P.rp = {0};
        check_ok(P, "m0");
        int nc = -7;
        std::string err;
        CHECK(smfv::order_multicolor(0, P.rp.data(), nullptr, 0, nullptr, nullptr, &nc, &err) && nc == 0, "m0 with null arrays: %s", err.c_str());
    }
    {
        Pattern P;  // one-sided: (i, i - 1) for odd i, (i - 1, i) for even i, and (0, m - 1) alone
        P.m = 41;
        std::vector<std::vector<int>> rows(41);
        for (int i = 1; i < 41; ++i) (i % 2 ? rows[(size_t)i] : rows[(size_t)i - 1]).push_back(i % 2 ? i - 1 : i);
        rows[0].push_back(40);
        P.rp.push_back(0);
        for (auto &r : rows) {
            P.ci.insert(P.ci.end(), r.begin(), r.end());
            P.rp.push_back((int)P.ci.size());
        }
        check_ok(P, "one_sided");
    }
    {
        Pattern P;  // empty rows only
        P.m = 7;
        P.rp.assign(8, 0);
        check_ok(P, "nnz0");
    }
    // refusals
    {
        Pattern P = make(50, 9, 4, true);
        Pattern Q = P;
        Q.ci[5] = 50;
        check_refused(Q, "column index 50", "column m");
        Q = P;
        Q.ci[7] = -1;
        check_refused(Q, "column index -1", "column -1");
        Q = P;
        Q.rp[0] = 1;
        check_refused(Q, "row_ptr[0]", "row_ptr[0]");
        Q = P;
        Q.rp[20] = Q.rp[19] - 1;
        check_refused(Q, "row_ptr decreases", "row_ptr down");

        std::string err;
        std::vector<int> perm(50), color(50), b_rp(51), b_ci(P.ci.size()), vp(P.ci.size());
        int nc = -7;
        CHECK(!smfv::order_multicolor(50, P.rp.data(), P.ci.data(), 1, perm.data(), color.data(), &nc, &err) &&
                  err.find("unknown flags") != std::string::npos, "flags 1 accepted: %s", err.c_str());
        CHECK(!smfv::order_multicolor(50, P.rp.data(), P.ci.data(), 0, nullptr, color.data(), &nc, &err) &&
                  err.find("null") != std::string::npos, "null perm accepted: %s", err.c_str());
        CHECK(!smfv::order_multicolor(50, P.rp.data(), P.ci.data(), 0, perm.data(), color.data(), nullptr, &err) &&
                  err.find("null") != std::string::npos, "null ncolors accepted: %s", err.c_str());
        CHECK(!smfv::order_multicolor(50, nullptr, P.ci.data(), 0, perm.data(), color.data(), &nc, &err), "null row_ptr accepted");
        CHECK(!smfv::order_multicolor(-1, P.rp.data(), P.ci.data(), 0, perm.data(), color.data(), &nc, &err), "m = -1 accepted");
        // no permutation: a value twice (the second place is named), a value out of range
        std::vector<int> bad(50);
        for (int i = 0; i < 50; ++i) bad[(size_t)i] = i;
        bad[30] = 4;
        CHECK(!smfv::csr_permute_sym(50, P.rp.data(), P.ci.data(), bad.data(), b_rp.data(), b_ci.data(), vp.data(), &err) &&
                  err.find("position 30 ") != std::string::npos && err.find("second time") != std::string::npos,
              "perm with a repeat accepted: %s", err.c_str());
        bad[30] = 30;
        bad[12] = 50;
        CHECK(!smfv::csr_permute_sym(50, P.rp.data(), P.ci.data(), bad.data(), b_rp.data(), b_ci.data(), vp.data(), &err) &&
                  err.find("position 12 ") != std::string::npos, "perm out of range accepted: %s", err.c_str());
        bad[12] = -3;
        CHECK(!smfv::check_permutation(50, bad.data(), nullptr, "x", &err) && err.find("position 12 holds -3") != std::string::npos,
              "negative entry accepted: %s", err.c_str());
        CHECK(!smfv::csr_permute_sym(50, P.rp.data(), P.ci.data(), nullptr, b_rp.data(), b_ci.data(), vp.data(), &err), "null perm accepted");
        CHECK(!smfv::csr_permute_sym(50, P.rp.data(), P.ci.data(), perm.data(), nullptr, b_ci.data(), vp.data(), &err), "null b_row_ptr accepted");
        CHECK(!smfv::csr_permute_sym(50, P.rp.data(), P.ci.data(), perm.data(), b_rp.data(), nullptr, vp.data(), &err), "null b_col_idx accepted");
        CHECK(!smfv::check_permutation(-1, bad.data(), nullptr, "x", nullptr), "size -1 accepted");
        std::vector<int> inv(50, -7);
        for (int i = 0; i < 50; ++i) bad[(size_t)i] = 49 - i;
        CHECK(smfv::check_permutation(50, bad.data(), inv.data(), "x", &err) && inv[0] == 49 && inv[49] == 0, "reversal refused");
    }
    if (failures) {
        std::fprintf(stderr, "reorder_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("reorder_check: OK\n");
    return 0;
}
