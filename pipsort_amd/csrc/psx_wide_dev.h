// psx_wide_dev.h — device code of the wide-set evaluator, shared by the translation
// units that instantiate it: psx_wide.hip (exhaustive levels and user batches of
// 7 .. PSX_KWIDE members) and psx_sss_wide.hip (the SSS walk of max_causal 7 .. 10).
//
// One 256-thread workgroup per set.  The set's operands go to LDS in one round
// trip; the 2 * 2^k (study, subset) LDL^T factorisations run one per thread per
// pass with eval_compute's arithmetic (psx_engine.hip) and leave (mu, n, f) per
// subset in LDS, weight 0 / f = +inf for a subset outside the study's presence
// mask, so that assignments the studies cannot hold vanish by themselves.
//
// The sums over the 3^k assignments (c0, c1) are bilinear forms in the k-fold
// Kronecker power of the per-member prior matrix M = [[0, a], [a, b]]
// (postcal.cpp:27-41; M1 = [[0, 1], [1, 1]] for the raw-likelihood columns):
// k in-place butterfly passes over the 2^k weights of study 1 instead of a walk
// over 3^k patterns.  For member j the transform runs over every axis but j, so
// axis j still indexes c1_j and the halves c with / without j of both studies'
// weights never mix: each half carries its own exponent reference
// (n_s[S_s], n_s[S_s \ j]), which is what keeps nsll[j] alive when member j's
// gain puts it more than a double's range under the set's maximum.  The score is
// the same butterfly in (min, +) over f.
//
// Butterfly slots: 1024 = 4 per thread.  A set of k members uses 2^Ke slots per
// transform, Ke = max(k, 7) (axes >= k are left alone: their upper halves are
// zero), and 2^(10 - Ke) members' leave-one-out transforms run side by side in
// the slot groups.  Layout A (slot = 4 thread + register) has axes 0, 1 in
// registers and axes 2 .. Ke - 3 across the lanes of a wave (DPP quad_perm,
// ds_swizzle, v_permlane32_swap); one pass through LDS then re-deals the slots
// so that axes Ke - 2, Ke - 1 (which cross the waves at k >= 9) are in
// registers (layout B), where the masked dot products with study 0 are taken.
#ifndef PSX_WIDE_DEV_H
#define PSX_WIDE_DEV_H

#include <cmath>

#include "psx_wave.h"
#include "psx_wide.h"

namespace psx {
namespace {

constexpr int KW = PSX_KWIDE;
constexpr int kThreads = 256;
constexpr int kSlots = 4 * kThreads;
constexpr int kKeMin = 7;  // fewest butterfly axes: a slot group is at least half a wave

template <int KM>
struct WideShm {
    static constexpr int NS = 1 << KM;
    double mu[2][NS], f[2][NS];  // per (study, subset): weight 2^n mu, ln weight
    int n[2][NS];
    double xch[2][2][kSlots];    // layout A -> B hand-off, double buffered: (M, M1) transforms
    double g[2][KW][KW], ad[2][KW], y[2][KW];
    double red[KW][8][6];        // per member, per 32-lane part of its slot group: the six dot products
    double smin[kThreads / 64];
    int mem[KW];
    unsigned pr[KW];
    int k, ok;
};

// the value of lane (l ^ (1 << B))
template <int B>
__device__ __forceinline__ double lane_xor(double x) {
    static_assert(B >= 0 && B <= 5, "lane bit");
    if constexpr (B == 0) {
        return dpp_f64<0xB1>(x);  // quad_perm:[1,0,3,2]
    } else if constexpr (B == 1) {
        return dpp_f64<0x4E>(x);  // quad_perm:[2,3,0,1]
    } else if constexpr (B <= 4) {
        constexpr int pat = ((1 << B) << 10) | 0x1f;  // bit mode: and 0x1f, or 0, xor 1 << B
        const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), pat);
        const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), pat);
        return __hiloint2double(hi, lo);
    } else {
        double p = x, q = x;  // after the swap: p = lanes 0-31 twice, q = lanes 32-63 twice
        swap32_f64(p, q);
        return (threadIdx.x & 32) ? p : q;
    }
}

// one axis of the Kronecker transform on the pair (x0, x1) = (bit clear, bit set)
struct SumOp {
    double a, b;
    __device__ __forceinline__ void pair(double& x0, double& x1) const {
        const double t = a * x1;
        x1 = fma(a, x0, b * x1);
        x0 = t;
    }
    // p: the partner's value; hi: this lane holds the bit-set entry
    __device__ __forceinline__ double cross(double p, double x, bool hi) const {
        return fma(a, p, hi ? b * x : 0.0);
    }
};
struct MinOp {  // (min, +) with [[+inf, la], [la, lb]]
    double la, lb;
    __device__ __forceinline__ void pair(double& x0, double& x1) const {
        const double t = la + x1;
        x1 = fmin(la + x0, lb + x1);
        x0 = t;
    }
    __device__ __forceinline__ double cross(double p, double x, bool hi) const {
        return hi ? fmin(la + p, lb + x) : la + p;
    }
};

template <int B, class Op>
__device__ __forceinline__ void lane_axis(double (&x)[4], int kA, int skip, int lane, const Op& op) {
    if (2 + B < kA) {  // (uniform: every lane takes part in the exchange)
        const bool hi = (lane >> B) & 1, keep = skip == 2 + B;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double v = op.cross(lane_xor<B>(x[r]), x[r], hi);
            x[r] = keep ? x[r] : v;
        }
    }
}
// layout A: axes 0 .. kA - 1 but `skip`
template <class Op>
__device__ __forceinline__ void axes_a(double (&x)[4], int kA, int skip, int lane, const Op& op) {
    if (0 < kA && skip != 0) { op.pair(x[0], x[1]); op.pair(x[2], x[3]); }
    if (1 < kA && skip != 1) { op.pair(x[0], x[2]); op.pair(x[1], x[3]); }
    lane_axis<0>(x, kA, skip, lane, op);
    lane_axis<1>(x, kA, skip, lane, op);
    lane_axis<2>(x, kA, skip, lane, op);
    lane_axis<3>(x, kA, skip, lane, op);
    lane_axis<4>(x, kA, skip, lane, op);
    lane_axis<5>(x, kA, skip, lane, op);
}
// layout B: axes Ke - 2, Ke - 1 (those below k) but `skip`
template <class Op>
__device__ __forceinline__ void axes_b(double (&x)[4], int Ke, int k, int skip, const Op& op) {
    if (Ke - 2 < k && skip != Ke - 2) { op.pair(x[0], x[1]); op.pair(x[2], x[3]); }
    if (Ke - 1 < k && skip != Ke - 1) { op.pair(x[0], x[2]); op.pair(x[1], x[3]); }
}

// The set sh.mem[0 .. sh.k) (1 <= k <= KM, ascending union indices), by the
// whole workgroup after a barrier: set record, member records, score.
template <int KM>
__device__ void eval_wide_staged(const WideProb& W, WideShm<KM>& sh, SetRec* __restrict__ so, Acc5* __restrict__ mo,
                                 double* __restrict__ sc, unsigned long long* __restrict__ tr);

// A set's operands in two halves, as eval_gather / eval_stage of the one-wave
// evaluator: wide_gather issues this thread's global loads (the (<= 2 * 45)
// lower-triangle Sigma~ entries, A_d, y, presence — one round trip), wide_stage
// waits for them and writes LDS.  A caller may put other loads between the two
// (k_sss_eval_wide's map probe) or drop the operands (a set already seen).
struct WideOps {
    double a, b;  // by the thread's role: a Sigma~ entry | (A_d, y) | ...
    unsigned pr;  // ... | presence bits
    int i, e;     // where they go: sh.g[s][i][e] | sh.ad[s][i], sh.y[s][i] | sh.pr[i]; i < 0: nothing
};
template <int KM>
__device__ __forceinline__ WideOps wide_gather(const WideProb& W, const WideShm<KM>& sh) {
    const int t = threadIdx.x, k = sh.k;
    WideOps o;
    o.a = o.b = 0.0;
    o.pr = 0;
    o.i = -1;
    o.e = 0;
    const double *G0 = W.G[0], *G1 = W.G[1], *A0 = W.Ad[0], *A1 = W.Ad[1], *Y0 = W.y[0], *Y1 = W.y[1];
    constexpr int NT = KW * (KW - 1) / 2;
    if (t < 2 * NT) {
        const int s = t / NT;
        int e = t % NT, i = 1;
        while (e >= i) { e -= i; i++; }
        if (i < k) {
            o.a = (s ? G1 : G0)[(size_t)sh.mem[i] * W.ldg + sh.mem[e]];
            o.i = i;
            o.e = e;
        }
    } else if (t >= 96 && t < 96 + 2 * KW) {
        const int s = (t - 96) / KW, i = (t - 96) % KW;
        if (i < k) {
            const int m = sh.mem[i];
            o.a = (s ? A1 : A0)[m];
            o.b = (s ? Y1 : Y0)[m];
            o.i = i;
        }
    } else if (t >= 128 && t < 128 + KW) {
        if (t - 128 < k) {
            o.pr = W.pres[sh.mem[t - 128]];
            o.i = t - 128;
        }
    }
    return o;
}
template <int KM>
__device__ __forceinline__ void wide_stage(const WideOps& o, WideShm<KM>& sh) {
    const int t = threadIdx.x;
    constexpr int NT = KW * (KW - 1) / 2;
    if (o.i < 0) return;
    if (t < 2 * NT) {
        sh.g[t / NT][o.i][o.e] = o.a;
    } else if (t < 128) {
        sh.ad[(t - 96) / KW][o.i] = o.a;
        sh.y[(t - 96) / KW][o.i] = o.b;
    } else {
        sh.pr[o.i] = o.pr;
    }
}

template <int KM>
__device__ void eval_wide(const WideProb& W, WideShm<KM>& sh, SetRec* __restrict__ so, Acc5* __restrict__ mo,
                          double* __restrict__ sc, unsigned long long* __restrict__ tr) {
    const WideOps o = wide_gather<KM>(W, sh);
    wide_stage<KM>(o, sh);
    __syncthreads();
    eval_wide_staged<KM>(W, sh, so, mo, sc, tr);
}

// ... with the operands staged (wide_stage) and a barrier after them
template <int KM>
__device__ void eval_wide_staged(const WideProb& W, WideShm<KM>& sh, SetRec* __restrict__ so, Acc5* __restrict__ mo,
                                 double* __restrict__ sc, unsigned long long* __restrict__ tr) {
    static_assert(KM >= kKeMin && KM <= KW, "members per set");
    const int t = threadIdx.x, lane = t & 63;
    const int k = sh.k;
    int S0 = 0, S1 = 0;
#pragma unroll
    for (int j = 0; j < KM; j++)
        if (j < k) {
            const unsigned pr = sh.pr[j];
            S0 |= (int)(pr & 1u) << j;
            S1 |= (int)((pr >> 1) & 1u) << j;
        }
    const int Ke = k > kKeMin ? k : kKeMin, nE = 1 << Ke;
    // one (study, subset) per thread per pass; slots past 2^k and subsets the
    // study cannot hold: weight 0, f = +inf
    for (int wk = t; wk < 2 * nE; wk += kThreads) {
        const int s = wk >> Ke, sub = wk & (nE - 1);
        double mu = 0.0, fv = INFINITY;
        int n = 0;
        if (!(sub & ~(s ? S1 : S0))) {
            double L[KM][KM], D[KM], Rd[KM], w[KM];
            double q = 0.0, Pd = 1.0;
            const double dv = s ? W.dval[1] : W.dval[0];
#pragma unroll
            for (int i = 0; i < KM; i++) {
                const bool in = i < k && ((sub >> i) & 1);
                double di = 1.0, wi = 0.0;
#pragma unroll
                for (int j = 0; j < i; j++) {
                    double acc = sh.g[s][i][j];
#pragma unroll
                    for (int m = 0; m < j; m++) acc -= L[i][m] * L[j][m] * D[m];
                    // L[j][*] = 0 and D[j] = 1 for j outside the subset
                    L[i][j] = in && ((sub >> j) & 1) ? acc * Rd[j] : 0.0;
                }
                if (in) {
                    di = sh.ad[s][i];
                    wi = sh.y[s][i];
#pragma unroll
                    for (int m = 0; m < i; m++) {
                        di -= L[i][m] * L[i][m] * D[m];
                        wi -= L[i][m] * w[m];
                    }
                }
                Rd[i] = 1.0 / di;  // one division per pivot (ldlt_terms' rounding)
                if (in) {
                    q += wi * wi * Rd[i];
                    Pd *= dv * di;
                }
                D[i] = di;
                w[i] = wi;
            }
            split_exp(0.5 * q * PSX_LOG2E, 1.0 / sqrt(Pd), n, mu);
            fv = 0.5 * q - 0.5 * log(Pd);
        }
        sh.mu[s][sub] = mu;
        sh.n[s][sub] = n;
        sh.f[s][sub] = fv;
    }
    __syncthreads();
    if (tr && blockIdx.x == 0 && t == 0) tr[1] = wall_clock64();

    const int kA = k < Ke - 2 ? k : Ke - 2;  // axes of layout A
    const int grp = t >> (Ke - 2);           // the thread's slot group (the same in both layouts)
    const int ngrp = kSlots >> Ke;
    int eB[4];                               // the thread's layout-B slots, as subsets
#pragma unroll
    for (int r = 0; r < 4; r++) eB[r] = ((r << (Ke - 2)) | (t & ((1 << (Ke - 2)) - 1)));

    // score: (min, +) over every axis, the same in every slot group
    double smin;
    {
        const MinOp op{W.la, W.lb};
        double x[4];
#pragma unroll
        for (int r = 0; r < 4; r++) x[r] = sh.f[1][(4 * t + r) & (nE - 1)];
        axes_a(x, kA, -1, lane, op);
#pragma unroll
        for (int r = 0; r < 4; r++) sh.xch[0][0][4 * t + r] = x[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) x[r] = sh.xch[0][0][(grp << Ke) | eB[r]];
        axes_b(x, Ke, k, -1, op);
        smin = INFINITY;
#pragma unroll
        for (int r = 0; r < 4; r++) smin = fmin(smin, sh.f[0][eB[r]] + x[r]);
        smin = fmin(smin, lane_xor<0>(smin));
        smin = fmin(smin, lane_xor<1>(smin));
        smin = fmin(smin, lane_xor<2>(smin));
        smin = fmin(smin, lane_xor<3>(smin));
        smin = fmin(smin, lane_xor<4>(smin));
        smin = fmin(smin, lane_xor<5>(smin));
        if (lane == 0) sh.smin[t >> 6] = smin;
    }

    // leave-one-out transforms, ngrp members per round
    const int n0S = sh.n[0][S0], n1S = sh.n[1][S1];
    const SumOp opM{W.a, W.b}, op1{1.0, 1.0};
    const int nh = 1 << (Ke - kKeMin);  // 32-lane parts of a slot group
    for (int rd = 0; rd * ngrp < k; rd++) {
        const int buf = (rd + 1) & 1;
        const int j = rd * ngrp + grp;
        const bool act = j < k;
        const int jj = act ? j : 0, bj = 1 << jj, skip = act ? j : 31;
        const int n0Sj = sh.n[0][S0 & ~bj], n1Sj = sh.n[1][S1 & ~bj];
        double xw[4], x1[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c = (4 * t + r) & (nE - 1);
            const double v = ldexp(sh.mu[1][c], sh.n[1][c] - ((c & bj) ? n1S : n1Sj));
            xw[r] = x1[r] = act ? v : 0.0;
        }
        axes_a(xw, kA, skip, lane, opM);
        axes_a(x1, kA, skip, lane, op1);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sh.xch[buf][0][4 * t + r] = xw[r];
            sh.xch[buf][1][4 * t + r] = x1[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            xw[r] = sh.xch[buf][0][(grp << Ke) | eB[r]];
            x1[r] = sh.xch[buf][1][(grp << Ke) | eB[r]];
        }
        axes_b(xw, Ke, k, skip, opM);
        axes_b(x1, Ke, k, skip, op1);
        // the (c0_j, c1_j) pieces: entry c holds c1_j = bit j of c and meets
        // study 0's weights of c with bit j set (c0_j = 1) and clear (c0_j = 0)
        double d[6] = {0, 0, 0, 0, 0, 0};  // M: P10 P01 P11, M1: X10 X01 X11
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c = eB[r], ch = c | bj, cl = c & ~bj;
            const double u1 = ldexp(sh.mu[0][ch], sh.n[0][ch] - n0S);
            const double u0 = ldexp(sh.mu[0][cl], sh.n[0][cl] - n0Sj);
            if (c & bj) {
                d[1] = fma(u0, xw[r], d[1]);
                d[2] = fma(u1, xw[r], d[2]);
                d[4] = fma(u0, x1[r], d[4]);
                d[5] = fma(u1, x1[r], d[5]);
            } else {
                d[0] = fma(u1, xw[r], d[0]);
                d[3] = fma(u1, x1[r], d[3]);
            }
        }
#pragma unroll
        for (int q = 0; q < 6; q++) {
            d[q] += lane_xor<0>(d[q]);
            d[q] += lane_xor<1>(d[q]);
            d[q] += lane_xor<2>(d[q]);
            d[q] += lane_xor<3>(d[q]);
            d[q] += lane_xor<4>(d[q]);
        }
        if (act && (t & 31) == 0) {
            const int h = (t >> 5) & (nh - 1);
#pragma unroll
            for (int q = 0; q < 6; q++) sh.red[j][h][q] = d[q];
        }
    }
    __syncthreads();
    if (tr && blockIdx.x == 0 && t == 0) tr[2] = wall_clock64();

    const int Ck = W.Ck[k];
    const double base = W.base[k];
    const int Gll = n0S + n1S + 2, GS = Gll + Ck;
    if (t < k) {
        const int bj = 1 << t;
        double d[6] = {0, 0, 0, 0, 0, 0};
        for (int h = 0; h < nh; h++)
#pragma unroll
            for (int q = 0; q < 6; q++) d[q] += sh.red[t][h][q];
        // shifts of the pieces: P11 on n0S + n1S, P10 on g1, P01 on g2
        const int g1 = n0S + sh.n[1][S1 & ~bj], g2 = sh.n[0][S0 & ~bj] + n1S;
        const int GN = imax(g1, g2) + 2;
        const double p10 = W.a * ldexp(d[0], g1 - Gll), p01 = W.a * ldexp(d[1], g2 - Gll);
        const double p11 = W.b * ldexp(d[2], -2);
        if (mo) {
            Acc5 a;
            a.mP = GS;
            a.mS = Gll;
            a.mN = GN;
            a.pad = 0;
            a.post0 = base * (p10 + p11);
            a.post1 = base * (p01 + p11);
            a.shared = base * p11;  // (not post0 + post1 - tot: that cancels when sharing is rare)
            a.sll = ldexp(d[5], -2);
            a.nsll = ldexp(d[3], g1 - GN) + ldexp(d[4], g2 - GN);
            mo[t] = a;
        }
        if (t == 0) {
            const int full = (1 << k) - 1;
            double ak = base, npat = 1.0;
            for (int j = 0; j < k; j++) {
                ak *= W.a;
                if (sh.pr[j] == 3u) npat *= 3.0;
            }
            double sm = sh.smin[0];
            for (int w = 1; w < kThreads / 64; w++) sm = fmin(sm, sh.smin[w]);
            sm += W.lnc[k];
            SetRec rr = set_zero();
            rr.m = GS;
            rr.m0 = n1S + Ck;
            rr.m1 = n0S + Ck;
            rr.tot = base * (p10 + p01 + p11);
            // noCausal[s]: study s empty, the other one full — one assignment each
            rr.nc0 = S1 == full ? ldexp(sh.mu[0][0] * sh.mu[1][full] * ak, sh.n[0][0]) : 0.0;
            rr.nc1 = S0 == full ? ldexp(sh.mu[0][full] * sh.mu[1][0] * ak, sh.n[1][0]) : 0.0;
            rr.score = sm;
            rr.npat = npat;
            *so = rr;
            if (sc) *sc = sm;
        }
    }
}

}  // namespace
}  // namespace psx
#endif
