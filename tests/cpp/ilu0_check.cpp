// ilu0_check.cpp -- stand-alone check of the ILU(0) host analysis
// (smfv::build_ilu0_plan in csrc/smfv_plan.cpp), built with
// -fsanitize=address,undefined by tests/test_ilu0_host.py: generated patterns
// (unsorted rows, empty-but-diagonal rows, long rows, degenerate shapes),
// every chain setting and several thresholds; each plan is re-checked here
// against a plain restatement (steps by a sort, pairs by a search in row i's sorted columns,
// the schedule's dependency rule step by step); bad inputs must be refused
// with a message.  Exit 0 and no sanitizer report = pass.
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

// rows of up to (r * 7 + 3) % maxlen distinct columns from a band of +-band
// around r or (every 11th row) from all of m, every 5th row its diagonal
// alone; the diagonal entry at a random place, the row in random order
Pattern make(int m, int maxlen, int band)
{
    Pattern P;
    P.m = m;
    P.rp.assign((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) {
        const int L = r % 5 == 4 ? 0 : (r * 7 + 3) % maxlen;
        std::set<int> cols{r};
        for (int k = 0; k < L; ++k) {
            int c = r % 11 == 0 ? (int)(rnd() % (uint32_t)m) : r - band + (int)(rnd() % (uint32_t)(2 * band + 1));
            cols.insert(std::min(std::max(c, 0), m - 1));
        }
        std::vector<int> row(cols.begin(), cols.end());
        for (size_t t = row.size(); t > 1; --t) std::swap(row[t - 1], row[rnd() % t]);
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

void check_ok(const Pattern &P, int flags, const char *name)
{
    const int m = P.m;
    smfv::Ilu0Plan I;
    std::string err;
    const bool ok = smfv::build_ilu0_plan(m, P.rp.data(), P.ci.data(), flags, I, &err);
    CHECK(ok, "%s (flags %d): refused: %s", name, flags, err.c_str());
    if (!ok) return;
    // the lower solve's levels and order
    std::vector<int> lev((size_t)m, -7), order((size_t)m, -7);
    int nlev = -7;
    CHECK(smfv::trsm_levels(m, P.rp.data(), P.ci.data(), 0, lev.data(), order.data(), &nlev, &err), "%s: trsm_levels refused", name);
    CHECK(I.nlevels == nlev && I.level == lev && I.order == order, "%s: levels or order differ from the lower solve's", name);
    // steps and pairs, restated
    int64_t steps = 0, pairs = 0, max_pairs = 0;
    int max_steps = 0, nlong = 0;
    bool layout = (int)I.step_ptr.size() == m + 1 && (int)I.row_beg.size() == m && (int)I.row_len.size() == m;
    for (int p = 0; layout && p < m; ++p) {
        const int i = order[(size_t)p], rs = P.rp[(size_t)i], len = P.rp[(size_t)i + 1] - rs;
        layout = layout && I.row_beg[(size_t)p] == rs && I.row_len[(size_t)p] == len;
        nlong += len > smfv::ILU0_SLOT;
        std::vector<std::pair<int, int>> low;
        for (int t = 0; t < len; ++t)
            if (P.ci[(size_t)rs + t] < i) low.push_back({P.ci[(size_t)rs + t], t});
        std::sort(low.begin(), low.end());
        std::vector<std::pair<int, int>> mine;  // (column, index inside the row), sorted
        for (int t = 0; t < len; ++t) mine.push_back({P.ci[(size_t)rs + t], t});
        std::sort(mine.begin(), mine.end());
        int s = I.step_ptr[(size_t)p];
        layout = layout && I.step_ptr[(size_t)p + 1] - s == (int)low.size();
        int64_t row_pairs = 0;
        for (size_t x = 0; layout && x < low.size(); ++x, ++s) {
            const int k = low[x].first;
            layout = layout && I.step_ent[(size_t)s] == low[x].second && P.ci[(size_t)I.step_diag[(size_t)s]] == k &&
                     I.step_diag[(size_t)s] >= P.rp[(size_t)k] && I.step_diag[(size_t)s] < P.rp[(size_t)k + 1];
            int u = I.pair_ptr[(size_t)s];
            for (int q = P.rp[(size_t)k]; q < P.rp[(size_t)k + 1]; ++q) {
                const int c = P.ci[(size_t)q];
                if (c <= k) continue;
                const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(c, 0));
                if (it == mine.end() || it->first != c) continue;
                const int tg = it->second;
                layout = layout && u < I.pair_ptr[(size_t)s + 1] && I.pair_tgt[(size_t)u] == tg && I.pair_src[(size_t)u] == q;
                ++u, ++row_pairs;
            }
            layout = layout && u == I.pair_ptr[(size_t)s + 1];
        }
        steps += (int64_t)low.size();
        pairs += row_pairs;
        max_steps = std::max(max_steps, (int)low.size());
        max_pairs = std::max(max_pairs, row_pairs);
    }
    CHECK(layout, "%s (flags %d): steps or pairs differ", name, flags);
    CHECK(I.steps == steps && I.pairs == pairs && I.max_steps == max_steps && I.max_pairs == max_pairs && I.long_rows == nlong,
          "%s: counts differ", name);
    CHECK((int)I.long_pos.size() == nlong && (int)I.long_ptr.size() == nlev + 1 && (nlev == 0 || I.long_ptr.back() == nlong),
          "%s: long-row lists differ", name);
    for (int l = 0; l < nlev; ++l)
        for (int t = I.long_ptr[(size_t)l]; t < I.long_ptr[(size_t)l + 1]; ++t)
            CHECK(lev[(size_t)order[(size_t)I.long_pos[(size_t)t]]] == l + 1 && I.row_len[(size_t)I.long_pos[(size_t)t]] > smfv::ILU0_SLOT,
                  "%s: long row %d is not of level %d", name, t, l);
    // schedule: the solves' rule, and every dependency earlier
    std::vector<int> launch_of((size_t)m, -1);
    int next_lev = 0;
    bool sched = true;
    for (size_t q = 0; q < I.launches.size() && sched; ++q) {
        const smfv::TrsmLaunch &L = I.launches[q];
        sched = L.lev_begin == next_lev && L.lev_end > L.lev_begin && L.lev_end <= nlev &&
                L.pos_begin == I.lev_ptr[(size_t)L.lev_begin] && L.pos_end == I.lev_ptr[(size_t)L.lev_end];
        if (!sched) break;
        for (int l = L.lev_begin; l < L.lev_end; ++l) {
            const int w = I.lev_ptr[(size_t)l + 1] - I.lev_ptr[(size_t)l];
            const bool thin = (flags & smfv::ILU0_NO_CHAIN) ? false : (flags & smfv::ILU0_CHAIN_ALL) ? true : w <= I.thin;
            sched = sched && thin == (L.chain != 0);
        }
        if (!L.chain) sched = sched && L.lev_end == L.lev_begin + 1;
        if (L.chain && q > 0) sched = sched && !I.launches[q - 1].chain;
        for (int p = L.pos_begin; p < L.pos_end; ++p) launch_of[(size_t)order[(size_t)p]] = (int)q;
        next_lev = L.lev_end;
    }
    CHECK(sched && next_lev == nlev, "%s (flags %d): schedule differs", name, flags);
    bool deps = sched;
    for (int i = 0; deps && i < m; ++i)
        for (int j = P.rp[(size_t)i]; j < P.rp[(size_t)i + 1]; ++j) {
            const int c = P.ci[(size_t)j];
            if (c >= i) continue;
            const int a = launch_of[(size_t)c], b = launch_of[(size_t)i];
            deps = deps && a >= 0 && (a < b || (a == b && I.launches[(size_t)b].chain && lev[(size_t)c] < lev[(size_t)i]));
        }
    CHECK(deps, "%s (flags %d): a dependency is not scheduled earlier", name, flags);
    double out[smfv::ILU0_NSTATS];
    I.stats(out);
    CHECK(out[0] == nlev && out[2] == (double)I.launches.size() && out[6] == (double)steps && out[7] == (double)pairs &&
              out[11] == smfv::ILU0_SLOT && out[14] == I.thin,
          "%s: stats differ", name);
}

void check_all_flags(const Pattern &P, const char *name)
{
    for (int chain : {0, smfv::ILU0_NO_CHAIN, smfv::ILU0_CHAIN_ALL}) check_ok(P, chain, name);
    for (int thin : {1, 3, 17, 65535}) check_ok(P, thin << smfv::ILU0_THIN_SHIFT, name);
}

void check_refused(const Pattern &P, int flags, const char *needle, const char *name)
{
    smfv::Ilu0Plan I;
    std::string err;
    const bool ok = smfv::build_ilu0_plan(P.m, P.rp.data(), P.ci.data(), flags, I, &err);
    CHECK(!ok, "%s: accepted", name);
    CHECK(err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", name, err.c_str(), needle);
}

}  // namespace

int main()
{
    check_all_flags(make(3000, 41, 40), "3000 band");
    check_all_flags(make(400, 700, 200), "400 long rows");
    check_all_flags(make(2000, 7, 2), "2000 narrow band");
    check_all_flags(make(1, 2, 1), "1x1");
    check_all_flags(make(0, 1, 1), "0x0");
    check_all_flags(make(300, 1, 1), "300 diagonal only");
    {
        Pattern P;  // an arrow: tridiagonal, the last row and column full
        P.m = 600;
        P.rp.push_back(0);
        for (int r = 0; r < 600; ++r) {
            if (r == 599) {
                for (int c = 598; c >= 0; --c) P.ci.push_back(c);
            } else {
                if (r) P.ci.push_back(r - 1);
                P.ci.push_back(599);
                if (r < 598) P.ci.push_back(r + 1);
            }
            P.ci.push_back(r);
            P.rp.push_back((int)P.ci.size());
        }
        check_all_flags(P, "600 arrow");
    }
    {
        Pattern P = make(300, 23, 30), Q = P;
        Q.ci[Q.ci.size() / 2] = Q.m;
        check_refused(Q, 0, "column index 300", "column m");
        Q = P;
        Q.ci[0] = -1;
        check_refused(Q, 0, "column index -1", "column -1");
        Q = P;
        Q.rp[0] = 1;
        check_refused(Q, 0, "row_ptr[0]", "row_ptr[0] != 0");
        Q = P;
        Q.rp[100] = Q.rp[99] - 1;
        check_refused(Q, 0, "row_ptr decreases", "row_ptr decreases");
        check_refused(P, smfv::ILU0_NO_CHAIN | smfv::ILU0_CHAIN_ALL, "exclude", "both chain flags");
        check_refused(P, 1 << 30, "unknown flags", "unknown flag");
        check_refused(P, 1, "unknown flags", "a trsm flag");
        // the first row without a diagonal entry is named
        Q = P;
        int removed = 0;
        for (int r : {212, 57})
            for (int j = Q.rp[(size_t)r]; j < Q.rp[(size_t)r + 1]; ++j)
                if (Q.ci[(size_t)j] == r) {
                    int c = 299;  // a column the row lacks
                    while (std::find(Q.ci.begin() + Q.rp[(size_t)r], Q.ci.begin() + Q.rp[(size_t)r + 1], c) != Q.ci.begin() + Q.rp[(size_t)r + 1]) --c;
                    Q.ci[(size_t)j] = c, ++removed;
                }
        CHECK(removed == 2, "no diagonal removed");
        check_refused(Q, 0, "row 57 has no diagonal", "missing diagonal");
        // a repeated column: row and column are named
        Q = P;
        int row = 0, a = -1, b = -1;
        for (; b < 0; ++row) {  // the first row with two entries off the diagonal
            a = b = -1;
            for (int j = Q.rp[(size_t)row]; j < Q.rp[(size_t)row + 1]; ++j)
                if (Q.ci[(size_t)j] != row) (a < 0 ? a : b) = j;
        }
        --row;
        Q.ci[(size_t)b] = Q.ci[(size_t)a];
        const std::string want = "row " + std::to_string(row) + " holds column " + std::to_string(Q.ci[(size_t)a]) + " more than once";
        check_refused(Q, 0, want.c_str(), "repeated column");
        std::string err;
        smfv::Ilu0Plan I;
        int one = 0;
        CHECK(!smfv::build_ilu0_plan(-1, &one, nullptr, 0, I, &err), "m = -1 accepted");
        CHECK(!smfv::build_ilu0_plan(1, nullptr, nullptr, 0, I, nullptr), "null row_ptr accepted");
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ilu0_check: OK\n");
    return 0;
}
