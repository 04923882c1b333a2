// trsm_check.cpp -- stand-alone check of the triangular-solve host analysis
// (smfv::trsm_levels, smfv::build_trsm_plan in csrc/smfv_plan.cpp), built with
// -fsanitize=address,undefined by tests/test_trsm_host.py: generated patterns
// (unsorted rows, repeated columns and diagonals, empty rows, long rows,
// degenerate shapes), both triangles, unit and non-unit, every chain setting
// and several thresholds; each plan is re-checked here against a plain
// restatement (levels by a sweep, order by a stable sort, the schedule's
// dependency rule entry by entry); bad inputs must be refused with a message.
// Exit 0 and no sanitizer report = pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
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

// rows of length (r * 7 + 3) % maxlen, every 5th row empty but for its
// diagonal, columns from a band of +-band around r or (every 11th row) from
// all of m, every 3rd row repeats its first column at its end; with `diag`
// every row gets a diagonal entry at a random place and every 7th row a second
Pattern make(int m, int maxlen, int band, bool diag)
{
    Pattern P;
    P.m = m;
    P.rp.assign((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) {
        const int L = r % 5 == 4 ? 0 : (r * 7 + 3) % maxlen;
        const size_t first = P.ci.size();
        for (int k = 0; k < L; ++k) {
            int c = r % 11 == 0 ? (int)(rnd() % (uint32_t)m) : r - band + (int)(rnd() % (uint32_t)(2 * band + 1));
            c = std::min(std::max(c, 0), m - 1);
            if (!diag && c == r) c = r > 0 ? r - 1 : (m > 1 ? 1 : 0);
            P.ci.push_back(c);
        }
        if (L > 1 && r % 3 == 0) P.ci.push_back(P.ci[first]);
        if (diag)
            for (int rep = 0; rep < (r % 7 == 0 ? 2 : 1); ++rep) {
                const size_t len = P.ci.size() - first;
                P.ci.insert(P.ci.begin() + (long)(first + rnd() % (len + 1)), r);
            }
        P.rp[(size_t)r + 1] = (int)P.ci.size();
    }
    if (!diag && m == 1) P.ci.clear(), P.rp[1] = 0;
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

void check_ok(const Pattern &P, int K, int flags, const char *name)
{
    const bool upper = flags & smfv::TRSM_UPPER, unit = flags & smfv::TRSM_UNIT_DIAG;
    const int m = P.m;
    smfv::TrsmPlan T;
    std::string err;
    const bool ok = smfv::build_trsm_plan(m, P.rp.data(), P.ci.data(), K, flags, T, &err);
    CHECK(ok, "%s (flags %d): refused: %s", name, flags, err.c_str());
    if (!ok) return;
    // levels by a plain sweep, order by a stable sort
    std::vector<int> lev((size_t)m, 0), order((size_t)m);
    int nlev = 0;
    for (int t = 0; t < m; ++t) {
        const int i = upper ? m - 1 - t : t;
        int l = 0;
        for (int j = P.rp[(size_t)i]; j < P.rp[(size_t)i + 1]; ++j) {
            const int c = P.ci[(size_t)j];
            if (upper ? c > i : c < i) l = std::max(l, lev[(size_t)c]);
        }
        lev[(size_t)i] = l + 1;
        nlev = std::max(nlev, l + 1);
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lev[(size_t)a] < lev[(size_t)b]; });
    CHECK(T.nlevels == nlev, "%s: %d levels, expected %d", name, T.nlevels, nlev);
    CHECK(T.level == lev, "%s: levels differ", name);
    CHECK(T.order == order, "%s: order differs", name);
    {
        std::vector<int> l2((size_t)m, -7), o2((size_t)m, -7);
        int n2 = -7;
        CHECK(smfv::trsm_levels(m, P.rp.data(), P.ci.data(), flags, l2.data(), o2.data(), &n2, &err), "%s: trsm_levels refused", name);
        CHECK(l2 == lev && o2 == order && n2 == nlev, "%s: trsm_levels differs", name);
    }
    // entries: strict in CSR order per position, diagonals apart, the rest ignored
    int64_t strict = 0, diag = 0, ignored = 0;
    bool layout = (int)T.ent_ptr.size() == m + 1 && (unit || (int)T.diag_ptr.size() == m + 1);
    for (int p = 0; layout && p < m; ++p) {
        const int i = order[(size_t)p];
        int e = T.ent_ptr[(size_t)p], d = unit ? 0 : T.diag_ptr[(size_t)p];
        for (int j = P.rp[(size_t)i]; j < P.rp[(size_t)i + 1]; ++j) {
            const int c = P.ci[(size_t)j];
            if (upper ? c > i : c < i) {
                layout = layout && e < (int)T.ent_col.size() && T.ent_col[(size_t)e] == c && T.ent_src[(size_t)e] == j;
                ++e, ++strict;
            } else if (c == i && !unit) {
                layout = layout && d < (int)T.diag_src.size() && T.diag_src[(size_t)d] == j;
                ++d, ++diag;
            } else {
                ++ignored;
            }
        }
        layout = layout && e == T.ent_ptr[(size_t)p + 1] && (unit || d == T.diag_ptr[(size_t)p + 1]);
    }
    CHECK(layout, "%s (flags %d): entry layout differs", name, flags);
    CHECK(T.strict == strict && T.diag == diag && T.ignored == ignored, "%s: entry counts differ", name);
    // schedule: levels in order, wide = its own launch, thin runs maximal, and
    // every dependency earlier
    std::vector<int> launch_of((size_t)m, -1);
    int next_lev = 0, chains = 0, most = 0;
    int64_t chain_rows = 0;
    bool sched = true;
    for (size_t q = 0; q < T.launches.size(); ++q) {
        const smfv::TrsmLaunch &L = T.launches[q];
        sched = sched && L.lev_begin == next_lev && L.lev_end > L.lev_begin && L.lev_end <= nlev &&
                L.pos_begin == T.lev_ptr[(size_t)L.lev_begin] && L.pos_end == T.lev_ptr[(size_t)L.lev_end];
        if (!sched) break;
        for (int l = L.lev_begin; l < L.lev_end; ++l) {
            const int w = T.lev_ptr[(size_t)l + 1] - T.lev_ptr[(size_t)l];
            const bool thin = (flags & smfv::TRSM_NO_CHAIN) ? false : (flags & smfv::TRSM_CHAIN_ALL) ? true : w <= T.thin;
            sched = sched && thin == (L.chain != 0);
        }
        if (!L.chain) sched = sched && L.lev_end == L.lev_begin + 1;
        if (L.chain && q > 0) sched = sched && !T.launches[q - 1].chain;  // maximal runs
        for (int p = L.pos_begin; p < L.pos_end; ++p) launch_of[(size_t)order[(size_t)p]] = (int)q;
        if (L.chain) ++chains, chain_rows += L.pos_end - L.pos_begin, most = std::max(most, L.lev_end - L.lev_begin);
        next_lev = L.lev_end;
    }
    CHECK(sched && next_lev == nlev, "%s (flags %d): schedule differs", name, flags);
    CHECK(chains == T.chain_launches && chain_rows == T.chain_rows && most == T.chain_max_levels, "%s: chain figures differ", name);
    bool deps = sched;
    for (int i = 0; deps && i < m; ++i)
        for (int j = P.rp[(size_t)i]; j < P.rp[(size_t)i + 1]; ++j) {
            const int c = P.ci[(size_t)j];
            if (!(upper ? c > i : c < i)) continue;
            const int a = launch_of[(size_t)c], b = launch_of[(size_t)i];
            deps = deps && a >= 0 && (a < b || (a == b && T.launches[(size_t)b].chain && lev[(size_t)c] < lev[(size_t)i]));
        }
    CHECK(deps, "%s (flags %d): a dependency is not scheduled earlier", name, flags);
    double out[smfv::TRSM_NSTATS];
    T.stats(out);
    CHECK(out[0] == nlev && out[2] == (double)T.launches.size() && out[6] == (double)strict && out[11] == T.thin, "%s: stats differ", name);
}

void check_all_flags(const Pattern &P, int K, const char *name, bool has_diag)
{
    for (int tri : {0, smfv::TRSM_UPPER})
        for (int unit : {0, smfv::TRSM_UNIT_DIAG}) {
            if (!unit && !has_diag) continue;
            for (int chain : {0, smfv::TRSM_NO_CHAIN, smfv::TRSM_CHAIN_ALL}) check_ok(P, K, tri | unit | chain, name);
            for (int thin : {1, 3, 17, 65535}) check_ok(P, K, tri | unit | (thin << smfv::TRSM_THIN_SHIFT), name);
        }
}

void check_refused(const Pattern &P, int K, int flags, const char *needle, const char *name)
{
    smfv::TrsmPlan T;
    std::string err;
    const bool ok = smfv::build_trsm_plan(P.m, P.rp.data(), P.ci.data(), K, flags, T, &err);
    CHECK(!ok, "%s: accepted", name);
    CHECK(err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", name, err.c_str(), needle);
}

}  // namespace

int main()
{
    check_all_flags(make(3000, 41, 40, true), 32, "3000 band", true);
    check_all_flags(make(700, 1300, 300, true), 8, "700 long rows", true);
    check_all_flags(make(2000, 7, 2, true), 1, "2000 narrow band", true);
    check_all_flags(make(500, 23, 30, false), 3, "500 no diagonal", false);
    check_all_flags(make(1, 2, 1, true), 5, "1x1", true);
    check_all_flags(make(1, 2, 1, false), 5, "1x1 empty", false);
    check_all_flags(make(0, 1, 1, true), 4, "0x0", true);
    check_all_flags(make(40, 1, 1, false), 4, "40 rows, no entries", false);
    check_all_flags(make(300, 1, 1, true), 128, "300 diagonal only", true);
    {
        Pattern P;  // a pure chain: row r names r - 1
        P.m = 300;
        P.rp.push_back(0);
        for (int r = 0; r < 300; ++r) {
            if (r) P.ci.push_back(r - 1);
            P.ci.push_back(r);
            P.rp.push_back((int)P.ci.size());
        }
        check_all_flags(P, 32, "300 chain", true);
    }
    {
        Pattern P = make(300, 23, 30, true), Q = P;
        Q.ci[Q.ci.size() / 2] = Q.m;
        check_refused(Q, 8, 0, "column index 300", "column m");
        Q = P;
        Q.ci[0] = -1;
        check_refused(Q, 8, 0, "column index -1", "column -1");
        Q = P;
        Q.rp[0] = 1;
        check_refused(Q, 8, 0, "row_ptr[0]", "row_ptr[0] != 0");
        check_refused(P, 0, 0, "K = 0", "K = 0");
        check_refused(P, -3, 0, "K = -3", "K < 0");
        check_refused(P, 8, smfv::TRSM_NO_CHAIN | smfv::TRSM_CHAIN_ALL, "exclude", "both chain flags");
        check_refused(P, 8, 1 << 30, "unknown flags", "unknown flag");
        // the first row without a diagonal entry is named
        Q = make(300, 23, 30, false);
        check_refused(Q, 8, 0, "row 0 has no diagonal", "no diagonal at all");
        Q = P;
        int removed = 0;
        for (int r : {212, 57}) {  // drop these rows' diagonal entries (turn them into a neighbour)
            for (int j = Q.rp[(size_t)r]; j < Q.rp[(size_t)r + 1]; ++j)
                if (Q.ci[(size_t)j] == r) Q.ci[(size_t)j] = r - 1, ++removed;
        }
        CHECK(removed >= 2, "no diagonal removed");
        check_refused(Q, 8, 0, "row 57 has no diagonal", "missing diagonal, lower");
        check_refused(Q, 8, smfv::TRSM_UPPER, "row 57 has no diagonal", "missing diagonal, upper");
        check_ok(Q, 8, smfv::TRSM_UNIT_DIAG, "missing diagonal with UNIT_DIAG");
        std::string err;
        int one = 0;
        CHECK(!smfv::trsm_levels(-1, &one, nullptr, 0, nullptr, nullptr, nullptr, &err), "m = -1 accepted");
        CHECK(!smfv::trsm_levels(1, nullptr, nullptr, 0, &one, &one, &one, nullptr), "null row_ptr accepted");
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("trsm_check: OK\n");
    return 0;
}
