"""psx::discrete_draw (pipsort_amd/csrc/psx_sample.h), the SSS walk's neighbour
draw, against libstdc++'s std::discrete_distribution, which the reference
calls (sss_postcal.cpp:296-343): the same index for every draw and the same
generator state afterwards, on weight vectors of the walk's kind (exp(lk - max)
with ties, zeros, underflow, one and two entries).  And the rest of the walk's
host logic in that header: the neighbourhood's geometry and order
(psx::sss_geometry, psx::sss_neighbour; sss_postcal.cpp:20-99, 166-186) against
its literal construction, and the draw of the next configuration
(psx::sss_sample_next) against the reference's statement of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
#include "psx_sample.h"

int main() {
    std::mt19937 wgen(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::mt19937 ga(12345), gb(12345);
    const size_t sizes[] = {1, 2, 3, 4, 17, 200, 975, 1000, 4096};
    long draws = 0, bad = 0;
    for (int rep = 0; rep < 400; rep++) {
        for (size_t n : sizes) {
            std::vector<double> lk(n);
            const int kind = rep % 5;
            for (size_t i = 0; i < n; i++) {
                double x = -U(wgen) * (kind == 0 ? 5.0 : kind == 1 ? 50.0 : 800.0);
                if (kind == 3 && i % 3 == 0) x = 0.0;             // ties at the max
                if (kind == 4 && i % 2 == 1) x = -1e308;          // exact zeros after exp
                lk[i] = x;
            }
            const double mx = *std::max_element(lk.begin(), lk.end());
            std::vector<double> pr(n);
            double s = 0.0;
            for (size_t i = 0; i < n; i++) s += (pr[i] = std::exp(lk[i] - mx));
            std::discrete_distribution<size_t> dist(pr.begin(), pr.end());
            for (int d = 0; d < 5; d++) {
                const size_t a = dist(ga);
                const size_t b = psx::discrete_draw(pr.data(), n, s, gb);
                draws++;
                if (a != b) bad++;
            }
            if (std::accumulate(pr.begin(), pr.end(), 0.0) != s) bad++;
        }
    }
    const bool same_state = ga == gb;
    std::printf("%ld %ld %d\n", draws, bad, same_state ? 1 : 0);
    return 0;
}
"""


# The walk's host logic (psx_sample.h) against the reference's construction.
# -DROWS: sss_geometry / sss_neighbour against the neighbourhood built with
# std::set; otherwise sss_sample_next against sss_postcal.cpp:296-343 restated.
WALK_HARNESS = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include <vector>
#include "psx_sample.h"

constexpr int KB = psx::kSssMaxK;
typedef std::vector<int> Set;

// the neighbourhood of cur (ascending) in the order swap ++ minus ++ plus
// (sss_postcal.cpp:20-99, 166-186), each neighbour by removing from and
// inserting into a std::set
static std::vector<Set> literal_nbd(const Set& cur, int U, int C, int counts[3]) {
    const int k = (int)cur.size();
    Set outside;
    for (int s = 0; s < U; s++)
        if (!std::count(cur.begin(), cur.end(), s)) outside.push_back(s);
    std::vector<Set> nbd;
    for (int x : outside)            // swap i: slot i % k out, the (i / k)-th outside SNP in
        for (int v = 0; v < k; v++) {
            std::set<int> s(cur.begin(), cur.end());
            s.erase(cur[v]);
            s.insert(x);
            nbd.push_back(Set(s.begin(), s.end()));
        }
    counts[0] = (int)nbd.size();
    for (int v = 0; v < k; v++) {    // minus: slot v out
        std::set<int> s(cur.begin(), cur.end());
        s.erase(cur[v]);
        nbd.push_back(Set(s.begin(), s.end()));
    }
    counts[1] = k;
    counts[2] = 0;
    if (k < C)
        for (int x : outside) {      // plus: an outside SNP in
            std::set<int> s(cur.begin(), cur.end());
            s.insert(x);
            nbd.push_back(Set(s.begin(), s.end()));
            counts[2]++;
        }
    return nbd;
}

static Set random_set(int U, int k, std::mt19937& g) {
    Set all(U);
    std::iota(all.begin(), all.end(), 0);
    std::shuffle(all.begin(), all.end(), g);
    Set s(all.begin(), all.begin() + k);
    std::sort(s.begin(), s.end());
    return s;
}

#ifdef ROWS
int main() {
    std::mt19937 sg(11);
    long pairs = 0, fewest = 1 << 30, rows = 0, bad = 0;
    for (int U = 1; U <= 9; U++)
        for (int C = 0; C <= std::min(U, 10); C++) {
            std::vector<Set> curs;
            for (int k = 0; k <= C; k++) {  // all-low and all-high (k = 0 and k = C among them)
                Set lo(k), hi(k);
                std::iota(lo.begin(), lo.end(), 0);
                std::iota(hi.begin(), hi.end(), U - k);
                curs.push_back(lo);
                curs.push_back(hi);
            }
            for (int r = 0; r < 200; r++) curs.push_back(random_set(U, (int)(sg() % (unsigned)(C + 1)), sg));
            pairs++;
            fewest = std::min(fewest, (long)curs.size());
            for (const Set& cur : curs) {
                const int k = (int)cur.size();
                int cnt[3];
                const std::vector<Set> nbd = literal_nbd(cur, U, C, cnt);
                const psx::SssGeom g = psx::sss_geometry(k, U, C);
                if (g.num_zero != cnt[0] || g.num_minus != cnt[1] || g.num_plus != cnt[2] ||
                    g.n_nbd != (int)nbd.size() || g.num_zero != (U - k) * k)
                    bad++;
                for (int i = 0; i < g.n_nbd && i < (int)nbd.size(); i++) {
                    int out[KB + 1];
                    std::fill(out, out + KB + 1, -7);
                    const int n = psx::sss_neighbour(cur.data(), k, g, i, out);
                    rows++;
                    if (n != (int)nbd[i].size() || !std::equal(nbd[i].begin(), nbd[i].end(), out) ||
                        !std::is_sorted(out, out + n) || out[n] != -7)
                        bad++;
                }
            }
        }
    std::printf("%ld %ld %ld %ld\n", pairs, fewest, rows, bad);
    return 0;
}
#else
// The walk's draw with the standard library's distribution (what
// sss_postcal.cpp:296-343 computes): for each non-empty group, in the order
// swap, minus, plus, one draw among exp(lk - the group's max) and the sum of
// those weights (accumulated from 0.0); then one draw among the three sums
// (an empty group's is 0.0) names the group whose draw is taken.
static Set oracle_next(const std::vector<double>& lk, const std::vector<Set>& nbd, const int cnt[3],
                       std::mt19937& gen) {
    size_t pick[3] = {0, 0, 0};
    std::vector<double> mass(3, 0.0);
    size_t first = 0;  // the group's first neighbour
    for (int grp = 0; grp < 3; first += (size_t)cnt[grp], grp++) {
        if (cnt[grp] == 0) continue;
        const auto lo = lk.begin() + first, hi = lo + cnt[grp];
        const double top = *std::max_element(lo, hi);
        std::vector<double> w(lo, hi);
        for (double& x : w) x = std::exp(x - top);
        pick[grp] = first + std::discrete_distribution<size_t>(w.begin(), w.end())(gen);
        mass[grp] = std::accumulate(w.begin(), w.end(), 0.0);
    }
    return nbd[pick[std::discrete_distribution<size_t>(mass.begin(), mass.end())(gen)]];
}

int main() {
    std::mt19937 wgen(7);
    std::uniform_real_distribution<double> R(0.0, 1.0);
    std::mt19937 ga(12345), gb(12345);
    const int chains[5][2] = {{3, 3}, {9, 1}, {12, 3}, {40, 6}, {25, 10}};  // (U, C)
    long steps = 0, bad = 0, empty_steps = 0;
    std::vector<double> pr;
    for (const auto& uc : chains) {
        const int U = uc[0], C = uc[1];
        Set ref;  // the walk starts at the null configuration
        int cur[KB] = {0}, k = 0;
        for (int step = 0; step < 1000; step++) {
            int cnt[3];
            const std::vector<Set> nbd = literal_nbd(ref, U, C, cnt);
            const size_t n = nbd.size();
            std::vector<double> lk(n);
            const int kind = step % 5;
            for (size_t i = 0; i < n; i++) {
                double x = -R(wgen) * (kind == 0 ? 5.0 : kind == 1 ? 50.0 : 800.0);
                if (kind == 3 && i % 3 == 0) x = 0.0;     // ties at the max
                if (kind == 4 && i % 2 == 1) x = -1e308;  // exact zeros after exp
                lk[i] = x;
            }
            empty_steps += cnt[0] == 0 || cnt[1] == 0 || cnt[2] == 0;
            ref = oracle_next(lk, nbd, cnt, ga);
            psx::sss_sample_next(lk.data(), psx::sss_geometry(k, U, C), gb, pr, cur, k);
            steps++;
            if (k != (int)ref.size() || !std::equal(ref.begin(), ref.end(), cur) || !(ga == gb)) bad++;
        }
    }
    std::printf("%ld %ld %ld %d\n", steps, bad, empty_steps, ga == gb ? 1 : 0);
    return 0;
}
#endif
"""


CLANG = "/opt/rocm/llvm/bin/clang++"  # hipcc's host compiler (the engine's host code)


def build_and_run(tmp_path, cxx, harness, extra=()):
    if not os.path.exists(cxx[0]) and os.sep in cxx[0]:
        pytest.skip(f"{cxx[0]} absent")
    src = tmp_path / "h.cpp"
    src.write_text(harness)
    exe = tmp_path / "h"
    r = subprocess.run(cxx + ["-std=c++17", *extra, "-I", os.path.join(ROOT, "pipsort_amd", "csrc"), str(src),
                              "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()


COMPILERS = pytest.mark.parametrize("cxx", [["g++", "-O2"], [CLANG, "-O3"]], ids=["gcc", "rocm-clang"])


@COMPILERS
def test_discrete_draw_matches_libstdcxx(tmp_path, cxx):
    out = build_and_run(tmp_path, cxx, HARNESS)
    draws, bad, same_state = int(out[0]), int(out[1]), int(out[2])
    assert draws == 400 * 9 * 5
    assert bad == 0
    assert same_state == 1


@COMPILERS
def test_neighbour_rows_match_literal_construction(tmp_path, cxx):
    """psx::sss_geometry / psx::sss_neighbour against the neighbourhood built
    with std::set, every neighbour of >= 200 configurations per (U, C)."""
    out = build_and_run(tmp_path, cxx, WALK_HARNESS, ["-DROWS"])
    pairs, fewest, rows, bad = (int(x) for x in out)
    assert pairs == sum(min(U, 10) + 1 for U in range(1, 10))
    assert fewest >= 200
    assert rows > 100000
    assert bad == 0


@COMPILERS
def test_sample_next_matches_reference_restatement(tmp_path, cxx):
    """psx::sss_sample_next against sss_postcal.cpp:296-343 restated with
    std::discrete_distribution and the explicit neighbour list: the same next
    configuration at every step of chained walks and the same generator after."""
    out = build_and_run(tmp_path, cxx, WALK_HARNESS)
    steps, bad, empty_steps, same_state = (int(x) for x in out)
    assert steps == 5 * 1000
    assert bad == 0
    assert empty_steps > 0  # steps with an empty group (k = 0, k = C) were among them
    assert same_state == 1
