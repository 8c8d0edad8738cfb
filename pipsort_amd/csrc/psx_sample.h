// psx_sample.h — the SSS walk's neighbour draw (sss_postcal.cpp:296-343) without
// std::discrete_distribution's two vectors.
//
// The reference draws with std::discrete_distribution<size_t>(w.begin(), w.end())
// (gen) under libstdc++ (bits/random.tcc: param_type::_M_initialize and
// operator()): fewer than two weights give the one-outcome distribution, which
// returns 0 without touching the generator; otherwise sum = accumulate(w, 0.0),
// p_i = w_i / sum, cp = partial_sum(p) with its last entry set to 1.0, one
// generate_canonical<double, 53> draw u, and the index of the first cp_i >= u
// (lower_bound).  discrete_draw does the same divisions and additions in the
// same order, so every partial sum is bit-identical, and scans them until the
// first one >= u (the same index: the sequence is non-decreasing and its last
// entry, 1.0, is >= u < 1).  The caller passes sum = accumulate(w, 0.0), which
// the walk needs anyway.  Checked against std::discrete_distribution by
// tests/test_sample_cpu.py.
//
// Also here, and pinned by the same test: an iteration's neighbourhood geometry
// and order (sss_postcal.cpp:166-186) and the whole draw of the next
// configuration (sss_sample_next).  An error in either makes a different walk,
// not a numerical error.  No HIP headers: this compiles with plain g++ / clang++.
#ifndef PSX_SAMPLE_H
#define PSX_SAMPLE_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <random>
#include <vector>

namespace psx {

// The neighbourhood of a configuration of k of U SNPs under max_causal C:
// num_zero swaps, num_minus removals, num_plus additions, in that order.
struct SssGeom {
    int num_zero, num_minus, num_plus, n_nbd;
};
inline SssGeom sss_geometry(int k, int U, int C) {
    SssGeom g;
    g.num_zero = (U - k) * k;
    g.num_minus = k;
    g.num_plus = k < C ? U - k : 0;
    g.n_nbd = g.num_zero + g.num_minus + g.num_plus;
    return g;
}

// Neighbour i (0 .. n_nbd) of cur[0 .. k) (ascending): its ascending members
// to out, its size returned.  Swap i puts the (i / k)-th SNP outside cur in
// place of slot i % k (member slot fastest), minus i drops slot i - num_zero,
// plus i adds the (i - num_zero - num_minus)-th SNP outside cur.  out holds
// k + 1 entries.  The host's statement of the kernels' nbd_row / nbd_entry.
inline int sss_neighbour(const int* cur, int k, const SssGeom& g, int i, int* out) {
    int x = -1, skip = -1;
    if (i < g.num_zero) {  // (cur \ {c_v}) + {x}
        skip = i % k;
        x = i / k;
    } else if (i < g.num_zero + g.num_minus) {  // cur \ {c_v}
        skip = i - g.num_zero;
    } else {  // cur + {x}
        x = i - g.num_zero - g.num_minus;
    }
    if (x >= 0)  // the x-th SNP not in cur
        for (int j = 0; j < k; j++)
            if (cur[j] <= x) x++;
    int n = 0;
    bool put = x < 0;
    for (int j = 0; j < k; j++) {
        if (j == skip) continue;
        if (!put && x < cur[j]) {
            out[n++] = x;
            put = true;
        }
        out[n++] = cur[j];
    }
    if (!put) out[n++] = x;
    return n;
}

template <class G>
inline size_t discrete_draw(const double* w, size_t n, double sum, G& gen) {
    if (n < 2) return 0;
    const double u = std::generate_canonical<double, std::numeric_limits<double>::digits>(gen);
    double cp = w[0] / sum;
    if (!(cp < u)) return 0;
    for (size_t i = 1; i + 1 < n; i++) {
        cp = cp + w[i] / sum;
        if (!(cp < u)) return i;
    }
    return n - 1;
}

// The next configuration: one neighbour drawn from every neighbour's score
// lk[0 .. n_nbd) (swap ++ minus ++ plus) with the reference's draws in the
// reference's order (sss_postcal.cpp:296-343), put in cur[0 .. k) (ascending).
// pr: scratch.  max_causal <= kSssMaxK.
constexpr int kSssMaxK = 10;  // the most members of a configuration (PSX_KWIDE)
template <class G>
inline void sss_sample_next(const double* lk, const SssGeom& g, G& gen, std::vector<double>& pr, int* cur, int& k) {
    double wz = 0, wm = 0, wp = 0;
    size_t zs = g.n_nbd, ms = g.n_nbd, ps = g.n_nbd;
    // each group: discrete_distribution(exp(lk - max))(gen) and the weights'
    // sum (accumulate), the draw restated without the distribution's vectors
    auto group = [&](int b, int en, double& wsum, size_t& smp) {
        pr.resize((size_t)(en - b));
        double mx = *std::max_element(lk + b, lk + en);
        // (slicing these exps over spinning host threads measured slower: the
        // serial loop takes ~5 us at 1,000 neighbours, profiles/archive/r03v_sss_threads.txt)
        double s = 0.0;
        for (int ii = b; ii < en; ii++) s += (pr[ii - b] = std::exp(lk[ii] - mx));
        smp = discrete_draw(pr.data(), pr.size(), s, gen);
        wsum = s;
    };
    if (g.num_zero != 0) group(0, g.num_zero, wz, zs);                               // :296-306
    if (g.num_minus != 0) group(g.num_zero, g.num_zero + g.num_minus, wm, ms);       // :307-317
    if (g.num_plus != 0) group(g.num_zero + g.num_minus, g.n_nbd, wp, ps);           // :318-328
    const double w3[3] = {wz, wm, wp};                                               // :330-343
    size_t idx = discrete_draw(w3, 3, (0.0 + wz + wm) + wp, gen), fin = 0;
    switch (idx) {
        case 0: fin = zs; break;
        case 1: fin = ms + g.num_zero; break;
        case 2: fin = ps + g.num_zero + g.num_minus; break;
    }
    int nxt[kSssMaxK];  // (no neighbour has more than max_causal members: num_plus is 0 at k = max_causal)
    const int n = sss_neighbour(cur, k, g, (int)fin, nxt);
    std::copy(nxt, nxt + n, cur);
    k = n;
}

}  // namespace psx

#endif
