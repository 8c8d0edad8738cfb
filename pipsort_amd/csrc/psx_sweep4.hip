// psx_sweep4.hip — tiled exhaustive sweep over union sets of four SNPs.
//
// A set is p < q < b < c.  A unit is (p, [q0, q1), B, T): one wave, p and the
// q range wave-uniform, lane t owns b = 64B + t, and the wave walks the 64 x 64
// (b, c) tile of T diagonally as sweep_unit does (psx_sweep_unit.h): at step j
// lane t takes c = 64T + ((t + j) & 63), reads G_bc from the skewed tiles and
// folds its c contribution into a per-wave LDS slot array whose ownership
// rotates with the step.  The b, q and p contributions are lane-owned LDS
// accumulators, wave-reduced once per unit (b: not at all), q and p.
//
// Every subset weight of {p, q, b, c} is formed once, at the outermost loop
// that fixes it (the incremental LDL^T of DESIGN section 3, member order
// p, q, b, c), per study:
//   per unit          {p}
//   per q             {q}, {p,q} and their factor rows: computed by lane q - q0
//                     for the whole q range at once and staged in LDS, so the q
//                     loop reads them back with no dependent global load
//   per q and lane    {b}, {p,b} (per unit), {q,b}, {p,q,b}
//   per step          {c} from muS / nS, and the seven extensions by the c row
//                     ({b,c}, {p,c}, {q,c}, {p,q,c}, {p,b,c}, {q,b,c},
//                     {p,q,b,c}): one pivot, one rsqrt_nr and one split2 each.
//                     G_pc / G_qc are rows p / q of Sigma~, staged per unit / per
//                     q in LDS and read at the step's c.
//
// Assignment sums.  The fast variant does not walk the 81 assignments.  With
// the prior multiplicative in the shared members (pit[n] = pit[0] rho^n) the
// sum over assignments is sum_{C0} E0[C0] (M x M x M x M E1)[C0], M = [0 1; 1 rho]
// per member (rows: the member's bit in C0, columns: in C1), so the per-member
// sums come from in-register butterflies over study 1's 16 weights with one
// member left out each (k_eval_wide's form, on the lane's own registers).  The
// EXACT variant is fold_set_patterns<4, true>, which keeps the per-group
// rescaling of notSharedLL; the fast variant raises the flag under the same
// 900-bit rule and the host re-sweeps the level.
#include <hip/hip_runtime.h>

#include "psx_sweep.h"
#include "psx_sweep_dev.h"
#include "psx_sweep_unit.h"

namespace psx {

namespace {

// wave-uniform scalars of one q of the unit and one study
struct QUni {
    double iA, y, h, rPs;       // {q}: 1 / A_qq, y_q, q log2(e) / 2, (d A_qq)^{-1/2} d^{-1/2}
    double Gpq, Lqp, iD, w;     // row q of the (p, q) factor: G_pq, G_pq / A_pp, 1 / D_q|p, w_q|p
    double hpq, rPpqs;          // {p,q}: q log2(e) / 2 and P^{-1/2} d^{-1/2}
    double mu1, mu3;            // split weights of {q} and {p,q}
    int n1, n3;
};

struct Sweep4Smem {
    Acc5 slot[64];     // c accumulators, ownership rotates every step
    Acc5 sacc[3][64];  // p, q, b accumulators, lane-owned
    QUni qu[kMaxChunkQ4][2];
    double pu[2][4];    // {p}: 1 / A_pp, y_p, q log2(e) / 2, P^{-1/2} d^{-1/2}
    double gpc[2][64];  // G_pc over the tile's 64 c
    double gqc[2][64];  // G_qc
};
static_assert(sizeof(Sweep4Smem) <= 160 * 1024 / 8, "two waves per SIMD: eight one-wave blocks share a CU's LDS");

// weight of parent + {c}: pivot D and residual w of the c row, the parent's
// q log2(e) / 2 and P^{-1/2} d^{-1/2}
__device__ __forceinline__ void ext_weight(double D, double w, double hpar, double rPs, int& n, double& mu) {
    const double r = rsqrt_nr(D);
    const double t = w * r;
    split2(fma(t * t, 0.5 * PSX_LOG2E, hpar), rPs * r, n, mu);
}

// one member's 2 x 2 factor applied along bit bj: x0' = x1, x1' = x0 + rho x1
template <bool UNIT>
__device__ __forceinline__ void kron_stage(double (&X)[16], int bj, double rho) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (i & bj) continue;
        const double x0 = X[i], x1 = X[i | bj];
        X[i] = x1;
        X[i | bj] = UNIT ? x0 + x1 : fma(rho, x1, x0);
    }
}

// S[j][x]: the sum over assignments with member j in study 0 only (x = 0),
// study 1 only (1) or both (2) of E0[C0] E1[C1] rho^shared (UNIT: rho = 1).
// Member j's sums apply the three other members to E1.
template <bool UNIT>
__device__ __forceinline__ void kron_sums(const double (&E0)[16], const double (&E1)[16], double rho,
                                          double (&S)[4][3]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int bj = 1 << j;
        // the pair without j (recomputed for j's partner: one product live at a time), then j's partner
        double F[16];
#pragma unroll
        for (int i = 0; i < 16; i++) F[i] = E1[i];
        kron_stage<UNIT>(F, (j < 2) ? 4 : 1, rho);
        kron_stage<UNIT>(F, (j < 2) ? 8 : 2, rho);
        kron_stage<UNIT>(F, 1 << (j ^ 1), rho);
        // bit j of F's index is still C1's, the other bits are C0's
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i & bj) continue;
            s0 = fma(E0[i | bj], F[i], s0);
            s1 = fma(E0[i], F[i | bj], s1);
            s2 = fma(E0[i | bj], F[i | bj], s2);
        }
        S[j][0] = s0;
        S[j][1] = s1;
        S[j][2] = UNIT ? s2 : rho * s2;
    }
}

// fold_set_patterns<4, false> without the walk over the 81 assignments
__device__ __forceinline__ void fold_set_kron4(const TileArgs& A, double rho, const int (&nn)[2][16],
                                               const double (&mu)[2][16], int Sm0, int Sm1, double wcount, int* flag,
                                               Acc5 (&out)[4], SetRec& sr) {
    const int nb0 = nn[0][15], nb1 = nn[1][15];
    double E0[16], E1[16];
#pragma unroll
    for (int T = 0; T < 16; T++) {
        E0[T] = ((T & ~Sm0) == 0) ? ldexp(mu[0][T], nn[0][T] - nb0) : 0.0;
        E1[T] = ((T & ~Sm1) == 0) ? ldexp(mu[1][T], nn[1][T] - nb1) : 0.0;
    }
    double Sw[4][3], Sl[4][3];
    kron_sums<false>(E0, E1, rho, Sw);
    kron_sums<true>(E0, E1, 1.0, Sl);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int x = 0; x < 3; x++) Sw[j][x] *= A.pit[0];
    fold_set_finish<4, false>(A, nn, mu, Sm0, Sm1, E0, E1, Sw, Sl, wcount, flag, out, sr);
}

}  // namespace

// units: {p, q0, q1, B | T << 16}; records unit-major at slot i (0..63 c,
// 64..127 b, 128 p, 129 + (q - q0) q)
template <bool EXACT>
__global__ __launch_bounds__(64, 2) void k_sweep4(TileArgs A, double rho, const int4* __restrict__ units,
                                                  Acc5* __restrict__ rec, SetRec* __restrict__ srec, int rec_stride,
                                                  int* __restrict__ flag) {
    __shared__ Sweep4Smem sm;
    const int t = threadIdx.x;
    const int unit = blockIdx.x;
    const int4 un = units[unit];
    const int p = un.x, q0 = un.y, nq = un.z - un.y, B = un.w & 0xffff, T = un.w >> 16;
    const int b = 64 * B + t;
    const bool bvalid = b < A.U;
    const int tile = T * (T + 1) / 2 + B;
    const int ldg = A.ldg;
    sm.slot[t] = acc_zero();
    sm.sacc[0][t] = acc_zero();
    sm.sacc[2][t] = acc_zero();
    SetRec accs = set_zero();
    accs.m = accs.m0 = accs.m1 = EMPTY;
    const unsigned pp = A.pres[p];
    const unsigned pb = bvalid ? A.pres[b] : 0u;
    double mu[2][16];
    int nn[2][16];
    // ---- per unit: {p}, {b}, {p,b}; the q range's uniform scalars into LDS ----------------
    double iApp[2], yp[2], hp[2], rPps[2];
    double Abb[2], iAbb[2], yb[2], hb[2], rPbs[2];
    double Gpb[2], Dbp[2], iDbp[2], wbp[2], hpb[2], rPpbs[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        mu[s][0] = 1.0;
        nn[s][0] = 0;
        const double rp = rsqrt_nr(A.Ad[s][p]);
        iApp[s] = rp * rp;
        yp[s] = A.y[s][p];
        hp[s] = 0.5 * PSX_LOG2E * yp[s] * yp[s] * iApp[s];
        const double rPp = rp * A.rsd[s];
        rPps[s] = rPp * A.rsd[s];
        split2(hp[s], rPp, nn[s][1], mu[s][1]);
        if (t == 0) {
            sm.pu[s][0] = iApp[s]; sm.pu[s][1] = yp[s]; sm.pu[s][2] = hp[s]; sm.pu[s][3] = rPps[s];
        }
        Abb[s] = A.Ad[s][b];
        const double rb = rsqrt_nr(Abb[s]);
        iAbb[s] = rb * rb;
        yb[s] = A.y[s][b];
        hb[s] = 0.5 * PSX_LOG2E * yb[s] * yb[s] * iAbb[s];
        const double rPb = rb * A.rsd[s];
        rPbs[s] = rPb * A.rsd[s];
        split2(hb[s], rPb, nn[s][4], mu[s][4]);
        Gpb[s] = A.G[s][(size_t)p * ldg + b];
        const double l = Gpb[s] * iApp[s];
        Dbp[s] = Abb[s] - l * Gpb[s];
        const double rbp = rsqrt_nr(Dbp[s]);
        iDbp[s] = rbp * rbp;
        wbp[s] = yb[s] - l * yp[s];
        hpb[s] = fma(wbp[s] * wbp[s] * iDbp[s], 0.5 * PSX_LOG2E, hp[s]);
        const double rPpb = rPps[s] * rbp;
        rPpbs[s] = rPpb * A.rsd[s];
        split2(hpb[s], rPpb, nn[s][5], mu[s][5]);
        sm.gpc[s][t] = A.G[s][(size_t)p * ldg + 64 * T + t];
        if (t < nq) {  // lane t: the scalars of q = q0 + t
            const int q = q0 + t;
            QUni u;
            const double Aqq = A.Ad[s][q];
            const double rq = rsqrt_nr(Aqq);
            u.iA = rq * rq;
            u.y = A.y[s][q];
            u.h = 0.5 * PSX_LOG2E * u.y * u.y * u.iA;
            const double rPq = rq * A.rsd[s];
            u.rPs = rPq * A.rsd[s];
            split2(u.h, rPq, u.n1, u.mu1);
            u.Gpq = A.G[s][(size_t)p * ldg + q];
            u.Lqp = u.Gpq * iApp[s];
            const double Dqp = Aqq - u.Lqp * u.Gpq;
            const double rqp = rsqrt_nr(Dqp);
            u.iD = rqp * rqp;
            u.w = u.y - u.Lqp * yp[s];
            u.hpq = fma(u.w * u.w * u.iD, 0.5 * PSX_LOG2E, hp[s]);
            const double rPpq = rPps[s] * rqp;
            u.rPpqs = rPpq * A.rsd[s];
            split2(u.hpq, rPpq, u.n3, u.mu3);
            sm.qu[t][s] = u;
        }
    }
    __syncthreads();
    for (int qi = 0; qi < nq; qi++) {
        const int q = q0 + qi;
        const unsigned pq = A.pres[q];
        sm.sacc[1][t] = acc_zero();
        // ---- per q and lane: {q}, {p,q} from LDS; {q,b}, {p,q,b} ----------------------------
        double Gqb[2], iDbq[2], wbq[2], hqb[2], rPqbs[2];
        double hbq[2], iDbpq[2], wbpq[2], hpqb[2], rPpqbs[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const QUni& u = sm.qu[qi][s];
            const double iAqq = u.iA, yq = u.y, hq = u.h, rPqs = u.rPs, iDqp = u.iD, wqp = u.w, hpq = u.hpq,
                         rPpqs = u.rPpqs;
            mu[s][2] = u.mu1; nn[s][2] = u.n1;
            mu[s][3] = u.mu3; nn[s][3] = u.n3;
            sm.gqc[s][t] = A.G[s][(size_t)q * ldg + 64 * T + t];
            Gqb[s] = A.G[s][(size_t)q * ldg + b];
            // {q,b}
            const double l = Gqb[s] * iAqq;
            const double Dbq = Abb[s] - l * Gqb[s];
            const double rbq = rsqrt_nr(Dbq);
            iDbq[s] = rbq * rbq;
            wbq[s] = yb[s] - l * yq;
            hqb[s] = fma(wbq[s] * wbq[s] * iDbq[s], 0.5 * PSX_LOG2E, hq);
            const double rPqb = rPqs * rbq;
            rPqbs[s] = rPqb * A.rsd[s];
            split2(hqb[s], rPqb, nn[s][6], mu[s][6]);
            // {p,q,b}: extend the (p, q) factor by the b row
            hbq[s] = Gqb[s] - u.Lqp * Gpb[s];
            const double l2 = hbq[s] * iDqp;
            const double Dbpq = Dbp[s] - l2 * hbq[s];
            const double rbpq = rsqrt_nr(Dbpq);
            iDbpq[s] = rbpq * rbpq;
            wbpq[s] = wbp[s] - l2 * wqp;
            hpqb[s] = fma(wbpq[s] * wbpq[s] * iDbpq[s], 0.5 * PSX_LOG2E, hpq);
            const double rPpqb = rPpqs * rbpq;
            rPpqbs[s] = rPpqb * A.rsd[s];
            split2(hpqb[s], rPpqb, nn[s][7], mu[s][7]);
        }
        const bool qbvalid = bvalid && q < b;
        const double wpqb = memb_weight(pp) * memb_weight(pq) * memb_weight(pb);
        __syncthreads();  // gqc
        for (int j = 0; j < 64; j++) {
            const int cc = (t + j) & 63;
            const int c = 64 * T + cc;
            const bool act = qbvalid && c < A.U && (B < T || cc > t);
            if (act) {
                const unsigned pc = A.pres[c];
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const double Acc_ = A.Ad[s][c];
                    const double yc = A.y[s][c];
                    const double Gbc = A.skew[s][(size_t)tile * 4096 + j * 64 + t];
                    const double Gpc = sm.gpc[s][cc];
                    const double Gqc = sm.gqc[s][cc];
                    // the wave-uniform scalars stay in LDS (broadcast reads), not in registers
                    const QUni& u = sm.qu[qi][s];
                    const double iApp = sm.pu[s][0], yp = sm.pu[s][1], hp = sm.pu[s][2], rPps = sm.pu[s][3];
                    const double iAqq = u.iA, yq = u.y, hq = u.h, rPqs = u.rPs, Gpq = u.Gpq, iDqp = u.iD, wqp = u.w,
                                 hpq = u.hpq, rPpqs = u.rPpqs;
                    mu[s][8] = A.muS[s][c];  // {c}: precomputed per SNP
                    nn[s][8] = A.nS[s][c];
                    // {b,c}
                    const double lb = Gbc * iAbb[s];
                    ext_weight(Acc_ - lb * Gbc, yc - lb * yb[s], hb[s], rPbs[s], nn[s][12], mu[s][12]);
                    // {p,c}
                    const double lp = Gpc * iApp;
                    const double Dpc = Acc_ - lp * Gpc;
                    const double wpc = yc - lp * yp;
                    ext_weight(Dpc, wpc, hp, rPps, nn[s][9], mu[s][9]);
                    // {q,c}
                    const double lq = Gqc * iAqq;
                    const double Dqc = Acc_ - lq * Gqc;
                    const double wqc = yc - lq * yq;
                    ext_weight(Dqc, wqc, hq, rPqs, nn[s][10], mu[s][10]);
                    // {p,q,c}: the (p, q) factor extended by the c row
                    const double h1 = Gqc - lp * Gpq;
                    const double l1 = h1 * iDqp;
                    const double Dpqc = Dpc - l1 * h1;
                    const double wpqc = wpc - l1 * wqp;
                    ext_weight(Dpqc, wpqc, hpq, rPpqs, nn[s][11], mu[s][11]);
                    // {p,b,c}
                    const double h2 = Gbc - lp * Gpb[s];
                    const double l2 = h2 * iDbp[s];
                    ext_weight(Dpc - l2 * h2, wpc - l2 * wbp[s], hpb[s], rPpbs[s], nn[s][13], mu[s][13]);
                    // {q,b,c}
                    const double h3 = Gbc - lq * Gqb[s];
                    const double l3 = h3 * iDbq[s];
                    ext_weight(Dqc - l3 * h3, wqc - l3 * wbq[s], hqb[s], rPqbs[s], nn[s][14], mu[s][14]);
                    // {p,q,b,c}: the (p, q, b) factor extended by the c row
                    const double h4 = h2 - l1 * hbq[s];
                    const double l4 = h4 * iDbpq[s];
                    ext_weight(Dpqc - l4 * h4, wpqc - l4 * wbpq[s], hpqb[s], rPpqbs[s], nn[s][15], mu[s][15]);
                }
                const unsigned m0 = (pp & 1) | ((pq & 1) << 1) | ((pb & 1) << 2) | ((pc & 1) << 3);
                const unsigned m1 = ((pp >> 1) & 1) | (((pq >> 1) & 1) << 1) | (((pb >> 1) & 1) << 2) |
                                    (((pc >> 1) & 1) << 3);
                Acc5 out[4];
                SetRec sr;
                if (EXACT)
                    fold_set_patterns<4, true>(A, nn, mu, (int)m0, (int)m1, wpqb * memb_weight(pc), flag, out, sr);
                else
                    fold_set_kron4(A, rho, nn, mu, (int)m0, (int)m1, wpqb * memb_weight(pc), flag, out, sr);
                ffold1(accs.m, accs.tot, sr.m, sr.tot);
                ffold1(accs.m0, accs.nc0, sr.m0, sr.nc0);
                ffold1(accs.m1, accs.nc1, sr.m1, sr.nc1);
                accs.npat += sr.npat;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    Acc5 x = sm.sacc[i][t];
                    ffold_acc(x, out[i]);
                    sm.sacc[i][t] = x;
                }
                Acc5 sl = sm.slot[cc];
                ffold_acc(sl, out[3]);
                sm.slot[cc] = sl;
            }
            __syncthreads();  // slot[] ownership rotates across lanes every step
        }
        Acc5 accq = sm.sacc[1][t];
        wave_fold_acc(accq);
        if (t == 0) store_rec(rec + (size_t)unit * rec_stride + 129 + qi, accq);
    }
    __syncthreads();
    store_rec(rec + (size_t)unit * rec_stride + t, sm.slot[t]);
    store_rec(rec + (size_t)unit * rec_stride + 64 + t, sm.sacc[2][t]);
    Acc5 accp = sm.sacc[0][t];
    wave_fold_acc(accp);
    if (t == 0) store_rec(rec + (size_t)unit * rec_stride + 128, accp);
    wave_fold_set(accs);
    if (t == 0) store_rec(srec + unit, accs);
}

// the SNP of every record slot (-1: none), once per plan
__global__ void k_keys4(const int4* __restrict__ units, long n, int rec_stride, int U, int* __restrict__ keys) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 un = units[i / rec_stride];
    const int s = (int)(i % rec_stride);
    int key;
    if (s < 64) key = 64 * (un.w >> 16) + s;
    else if (s < 128) key = 64 * (un.w & 0xffff) + s - 64;
    else if (s == 128) key = un.x;
    else key = un.y + s - 129 < un.z ? un.y + s - 129 : -1;
    keys[i] = key < U ? key : -1;
}

int launch_keys4(const int4* units, int n_units, int rec_stride, int U, int* keys, hipStream_t st) {
    const long n = (long)n_units * rec_stride;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_keys4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, units, n, rec_stride, U, keys);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sweep4(bool exact, const TileArgs& A, int n_units, const int4* units, Acc5* rec, SetRec* srec,
                  int rec_stride, int* flag, hipStream_t st) {
    if (n_units <= 0) return 0;
    // the Kronecker sums need pit[n] = pit[0] rho^n; a prior with no unshared
    // weight (pit[0] = 0) takes the pattern walk, which reads the table itself
    const bool walk = exact || !(A.pit[0] > 0.0);
    const double rho = walk ? 0.0 : A.pit[1] / A.pit[0];
    if (walk)
        hipLaunchKernelGGL(k_sweep4<true>, dim3(n_units), dim3(64), 0, st, A, rho, units, rec, srec, rec_stride, flag);
    else
        hipLaunchKernelGGL(k_sweep4<false>, dim3(n_units), dim3(64), 0, st, A, rho, units, rec, srec, rec_stride,
                           flag);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// load this translation unit's device code on the current device (psx_warmup_for)
int warm_module_sweep4() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_keys4) == hipSuccess ? 0 : -1;
}

}  // namespace psx
