// Host walk of the packed launches' placement (csrc/pack.hpp), built and run by test_pack_placement_cpu.py with the host
// sanitizers on: for every S in 1..16 and per-seed workgroup counts drawn from {0, 1, 2, 7, 8, 9, 33} (0: an absent seed),
// place() + locate() must hand every (seed, local) with local < count[seed] to exactly one workgroup of [0, grid) and
// nothing else to any, on the smallest grid the mapping allows; place_members() + locate_grid() must do the same up to
// the caller's own bound on `local` (a superset, and never a seed >= S).  Prints the S whose mapping came out pinned
// (RRL_PACK_PINNED is read once per process: the test runs this program once per setting).  Exit status 0: all held.
#include <stdio.h>

#include <set>
#include <utility>
#include <vector>

#include "pack.hpp"

namespace {

const int kCounts[] = {0, 1, 2, 7, 8, 9, 33};
constexpr int kN = sizeof kCounts / sizeof kCounts[0];
int failures = 0, patterns = 0;

#define REQUIRE(cond, ...)                                \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                printf("FAILED %s: ", #cond);             \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
            return;                                       \
        }                                                 \
    } while (0)

// the smallest grid the mapping of S seeds allows for these per-seed counts
int smallest_grid(int S, const int* count) {
    int sp, p, r, most = 0, sum = 0;
    for (int s = 0; s < S; ++s) {
        most = count[s] > most ? count[s] : most;
        sum += count[s];
    }
    if (!rrl_pack::pinned_mapping(S, sp, p, r)) return sum;
    return S > 8 ? 8 * r * most : 8 * ((most + p - 1) / p);
}

void walk_1d(int S, const std::vector<int>& count) {
    const rrl_pack::Launch l = rrl_pack::place(S, count.data());
    REQUIRE(l.grid == smallest_grid(S, count.data()), "S=%d grid=%d", S, l.grid);
    std::set<std::pair<int, int>> seen;
    for (int b = 0; b < l.grid; ++b) {
        int s = -1, local = -1;
        if (!rrl_pack::locate(l.ix, b, s, local)) continue;
        REQUIRE(s >= 0 && s < S && local >= 0 && local < count[s], "S=%d b=%d -> (%d, %d)", S, b, s, local);
        REQUIRE(seen.insert({s, local}).second, "S=%d b=%d: (%d, %d) twice", S, b, s, local);
    }
    size_t want = 0;
    for (int s = 0; s < S; ++s) want += count[s];
    REQUIRE(seen.size() == want, "S=%d: %zu of %zu (seed, local) served", S, seen.size(), want);
}

void walk_2d(int S, const std::vector<int>& most) {
    const rrl_pack::Launch l = rrl_pack::place_members(S, most.data());
    std::vector<int> row(S);
    for (int s = 0; s < S; ++s) row[s] = most[s] > 0 ? most[s] : 1;          // a member row has at least one workgroup
    REQUIRE(l.grid == smallest_grid(S, row.data()), "2-D S=%d grid=%d", S, l.grid);
    std::set<std::pair<int, int>> seen;
    for (int b = 0; b < l.grid; ++b) {
        int s = -1, local = -1;
        if (!rrl_pack::locate_grid(l.ix, b, s, local)) continue;
        REQUIRE(s >= 0 && s < S && local >= 0, "2-D S=%d b=%d -> (%d, %d)", S, b, s, local);
        REQUIRE(seen.insert({s, local}).second, "2-D S=%d b=%d: (%d, %d) twice", S, b, s, local);
    }
    for (int s = 0; s < S; ++s)
        for (int local = 0; local < most[s]; ++local)
            REQUIRE(seen.count({s, local}) == 1, "2-D S=%d: (%d, %d) not served", S, s, local);
}

void check(int S, const std::vector<int>& count) {
    ++patterns;
    walk_1d(S, count);
    walk_2d(S, count);
}

}  // namespace

int main() {
    unsigned lcg = 12345u;
    printf("pinned:");
    for (int S = 1; S <= rrl_pack::kMaxSeeds; ++S) {
        int sp, p, r;
        if (rrl_pack::pinned_mapping(S, sp, p, r)) printf(" %d", S);
        for (int v : kCounts) check(S, std::vector<int>(S, v));                       // all equal (all absent included)
        for (int small : {0, 1, 2})                                                   // one large, the rest small
            for (int at : {0, S / 2, S - 1}) {
                std::vector<int> c(S, small);
                c[at] = 33;
                check(S, c);
            }
        std::vector<int> up(S), down(S);                // strictly increasing (as far as seven values go, then again) / decreasing
        for (int s = 0; s < S; ++s) {
            up[s] = kCounts[s % kN];
            down[s] = kCounts[(S - 1 - s) % kN];
        }
        check(S, up);
        check(S, down);
        for (int k = 0; k < 8; ++k) {                                                 // and mixed draws from the set
            std::vector<int> c(S);
            for (int& v : c) {
                lcg = lcg * 1664525u + 1013904223u;
                v = kCounts[(lcg >> 16) % kN];
            }
            check(S, c);
        }
    }
    printf("\npatterns: %d\nfailures: %d\n", patterns, failures);
    return failures ? 1 : 0;
}
