// psx_sss_wide.hip — the SSS walk (sss_postcal.cpp:102-380) for max_causal 7 ..
// PSX_KWIDE on gfx950: one iteration is two launches, as in the narrow walk
// (psx_engine.hip), around the wide-set evaluator (psx_wide_dev.h).
//
//   k_sss_eval_wide<KM>  one 256-thread workgroup per item (the current
//       configuration, then the neighbourhood swap ++ minus ++ plus in the
//       reference's order).  Wave 0 builds the item's row straight from the
//       iteration geometry, one member per lane, and packs its key with lane
//       reads; after one barrier every thread issues its operand loads and wave
//       0 probes the set map while they are in flight.  A seen or null item
//       writes zero records and drops the loads; an unseen set of any size
//       1 .. KM runs eval_wide_staged<KM> (sets of fewer than 7 members on 7
//       butterfly axes: only a walk's first iterations have them, and a second
//       launch per iteration for the one-wave evaluator would cost every one).
//   k_sss_post_wide      a block per union SNP folds its records, one block the
//       set records and null configurations, the rest insert the new scores
//       into the map.
//
// Every neighbour's weight and mark go to pinned host memory from the eval by
// plain stores, and the host waits on the eval's stop event before it reads
// them (it samples the next configuration while the post runs): an eval takes
// a few hundred microseconds, so there is no mark-word polling here.
#include "psx_sss_wide.h"

#include "psx_sweep_dev.h"
#include "psx_wide_dev.h"

extern "C" __device__ __attribute__((const)) int __ockl_wfred_add_i32(int);

namespace psx {
namespace {

static_assert(3 * 4 >= KW, "four key words hold PSX_KWIDE fields");

__device__ inline unsigned long long wmap_slot(const unsigned long long (&w)[4], unsigned long long mask) {
    unsigned long long h = 0;
#pragma unroll
    for (int q = 3; q >= 0; q--) h = mix64(w[q] ^ (h + 0x9e3779b97f4a7c15ULL));
    return h & mask;
}
// Lookup by a whole wave, as map_find_wave of the narrow walk: 64 consecutive
// probe slots per round trip; the key's slot is the first in probe order that
// is empty or matches.  Result in every lane.
__device__ inline bool wmap_find_wave(const WideMapEntry* T, unsigned long long mask,
                                      const unsigned long long (&w)[4], double& v) {
    const int lane = threadIdx.x & 63;
    const unsigned long long base = wmap_slot(w, mask);
    for (unsigned long long off = 0;; off += 64) {
        const WideMapEntry& e = T[(base + off + lane) & mask];
        const bool empty = e.state == 0;
        const bool match = !empty && e.w[0] == w[0] && e.w[1] == w[1] && e.w[2] == w[2] && e.w[3] == w[3];
        const unsigned long long me = __ballot(empty), mm = __ballot(match);
        const unsigned long long before = me ? (me & (0ull - me)) - 1ull : ~0ull;  // lanes below the first empty
        if (mm & before) {
            v = __shfl(e.score, __ffsll((long long)(mm & before)) - 1);
            return true;
        }
        if (me) return false;
    }
}
// keys inserted by one launch are distinct and no lookup runs beside an insert
__device__ inline void wmap_insert(WideMapEntry* T, unsigned long long mask, const unsigned long long (&w)[4],
                                   double v) {
    for (unsigned long long i = wmap_slot(w, mask);; i = (i + 1) & mask)
        if (atomicCAS(&T[i].state, 0, 1) == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) T[i].w[q] = w[q];
            T[i].score = v;
            return;
        }
}

// entry c of the current configuration (c uniform or per lane; cur is in scalar registers)
__device__ __forceinline__ int cur_at(const SssWideIter& it, int c) {
    int v = -1;
#pragma unroll
    for (int j = 0; j < KW; j++) v = c == j ? it.cur[j] : v;
    return v;
}
// the x-th SNP outside the current configuration
__device__ __forceinline__ int outside(const SssWideIter& it, int x) {
#pragma unroll
    for (int j = 0; j < KW; j++)
        if (j < it.k && it.cur[j] <= x) x++;
    return x;
}

// Entry j of the sorted row of neighbour i (i == -1: the current configuration),
// -1 from its size n on: cur without slot `skip`, with SNP x put in its place
// in order.  No per-thread row array: each lane takes its entry from the
// geometry, so nothing here can go to scratch.
__device__ __forceinline__ int nbd_entry(const SssWideIter& it, int i, int j, int& n) {
    const int k = it.k;
    int x = -1, skip = KW;
    if (i < 0) {
        n = k;
    } else if (i < it.num_zero) {  // (cur \ {c_v}) + {x}
        skip = i % k;
        x = i / k;
        n = k;
    } else if (i < it.num_zero + it.num_minus) {  // cur \ {c_v}
        skip = i - it.num_zero;
        n = k - 1;
    } else {  // cur + {x}
        x = i - it.num_zero - it.num_minus;
        n = k + 1;
    }
    int pos = KW + 1;  // x's place among the kept members
    if (x >= 0) {
        x = outside(it, x);
        pos = 0;
#pragma unroll
        for (int c = 0; c < KW; c++) pos += c < k && c != skip && it.cur[c] < x;
    }
    const int b = j - (j > pos);  // index among the kept members, which skip slot `skip`
    const int v = j == pos ? x : cur_at(it, b + (b >= skip));
    return j < n ? v : -1;
}

template <int KM>
__global__ __launch_bounds__(kThreads) void k_sss_eval_wide(WideProb W, SssWideIter it,
                                                            const WideMapEntry* __restrict__ T,
                                                            unsigned long long mask, int* __restrict__ mark,
                                                            int* __restrict__ cnt,
                                                            unsigned long long* __restrict__ keys,
                                                            double* __restrict__ lk_host,
                                                            int* __restrict__ mark_host, SetRec* __restrict__ srec,
                                                            Acc5* __restrict__ mrec, double* __restrict__ score) {
    __shared__ WideShm<KM> sh;
    const int p = blockIdx.x, i = p - 1, t = threadIdx.x;
    unsigned long long w[4] = {0, 0, 0, 0};
    if (t < 64) {
        int n = 0;
        const int v = nbd_entry(it, i, t, n);  // (-1 in the lanes past the row)
        if (t < KW) sh.mem[t] = v;
        if (t == 0) sh.k = n;
        // the key: field t of word t / 3; lanes past the members hold 0
        const unsigned long long fld = (unsigned long long)(v + 1) << (kKeyBits * (t % 3));
#pragma unroll
        for (int q = 0; q < 4; q++)
            w[q] = __shfl(fld, 3 * q) | __shfl(fld, 3 * q + 1) | __shfl(fld, 3 * q + 2);
    }
    __syncthreads();
    // the operands are requested before the map probe and consumed after it
    const WideOps ops = wide_gather<KM>(W, sh);
    if (t < 64) {
        const int n = sh.k;
        double v = 0.0;
        const int seen = wmap_find_wave(T, mask, w, v) ? 1 : 0;
        if (i >= 0) {
            if (t < 4) keys[4 * (size_t)i + t] = t == 0 ? w[0] : t == 1 ? w[1] : t == 2 ? w[2] : w[3];
            if (t == 0) {
                const int mk = seen ? -1 : (n == 0 ? -2 : p);
                mark[i] = mk;
                mark_host[i] = mk;
                if (mk != p) lk_host[i] = seen ? v : it.null_score;  // (an unseen set's after its evaluation)
            }
        } else if (t == 0) {
            cnt[kCurPos] = (seen || n == 0) ? -1 : 0;  // a null current configuration is counted, not evaluated
            cnt[kCurNull] = (!seen && n == 0) ? 1 : 0;
        }
        if (t == 0) sh.ok = !seen && n > 0;
    }
    __syncthreads();
    if (!sh.ok) {
        // zero records (a fold of a zero record is exactly a no-op): the post folds
        // every item without looking at marks
        if (t < it.stride) mrec[(size_t)p * it.stride + t] = acc_zero();
        if (t == 0) srec[p] = set_zero();
        return;
    }
    wide_stage<KM>(ops, sh);
    __syncthreads();
    eval_wide_staged<KM>(W, sh, srec + p, mrec + (size_t)p * it.stride, score + p, nullptr);
    if (t == 0 && i >= 0) lk_host[i] = score[p];  // the thread that wrote it
}

// blocks [0, U): per-SNP record folds; block U: the scalars; blocks > U: the
// map inserts
__global__ __launch_bounds__(256) void k_sss_post_wide(SssWideIter it, const int* __restrict__ mark,
                                                       const int* __restrict__ cnt,
                                                       const unsigned long long* __restrict__ keys,
                                                       const Acc5* __restrict__ mrec,
                                                       const SetRec* __restrict__ srec,
                                                       const double* __restrict__ score, SetRec null1,
                                                       Acc5* __restrict__ acc, SetRec* __restrict__ sacc,
                                                       SetRec* __restrict__ sacc_host, int* __restrict__ cnt_host,
                                                       WideMapEntry* __restrict__ T, unsigned long long mask) {
    const int b = blockIdx.x, t = threadIdx.x;
    // Every item p has records at mrec[p * stride + j] (zero records where
    // k_sss_eval_wide did not evaluate it), and a member's position j in item
    // p's row follows from the iteration geometry.
    const int k = it.k, n_items = it.n_nbd + 1;
    if (b < it.U) {
        const int u = b;
        int ju = -1, less = 0;  // u's slot in cur (or -1); members of cur below u
#pragma unroll
        for (int j = 0; j < KW; j++) {
            ju = j < k && it.cur[j] == u ? j : ju;
            less += j < k && it.cur[j] < u;
        }
        Acc5 a = acc_zero();
        if (ju >= 0) {
            // in (nearly) every item: the items in item order
            constexpr int kR = 4;  // record loads in flight per thread
            for (int p0 = t; p0 < n_items; p0 += 256 * kR) {
                Acc5 r[kR];
#pragma unroll
                for (int q = 0; q < kR; q++) {
                    const int p = p0 + 256 * q;
                    int j = -1;
                    if (p < n_items) {
                        const int i = p - 1;
                        if (i < 0) {
                            j = ju;
                        } else if (i < it.num_zero + it.num_minus) {  // swap / minus: slot v dropped
                            const int v = i < it.num_zero ? i % k : i - it.num_zero;
                            if (v != ju) {
                                j = ju - (v < ju);
                                if (i < it.num_zero) j += outside(it, i / k) < u;  // + that SNP outside cur
                            }
                        } else {  // plus
                            j = ju + (outside(it, i - it.num_zero - it.num_minus) < u);
                        }
                    }
                    r[q] = j >= 0 ? mrec[(size_t)p * it.stride + j] : acc_zero();
                }
#pragma unroll
                for (int q = 0; q < kR; q++) fold_acc(a, r[q]);
            }
            __shared__ Acc5 sh[4];
            wave_fold_acc(a);
            if ((t & 63) == 0) sh[t >> 6] = a;
            __syncthreads();
            if (t == 0) {
                Acc5 g = acc[u];
                for (int q = 0; q < 4; q++) fold_acc(g, sh[q]);
                acc[u] = g;
            }
            return;
        }
        if (t >= 64) return;
        // u is the ri-th SNP outside cur: items ri * k + v (cur with slot v swapped
        // for u: u's position is `less`, one fewer when cur[v] < u), then its plus
        // set; one record per lane of wave 0
        const int ri = u - less;
        int i = -1, j = 0;
        if (t < k) {
            i = ri * k + t;
            j = less - (cur_at(it, t) < u);
        } else if (t == k && it.num_plus) {
            i = it.num_zero + it.num_minus + ri;
            j = less;
        }
        if (i >= 0) a = mrec[(size_t)(i + 1) * it.stride + j];
        wave_fold_acc(a);
        if (t == 0 && (a.post0 != 0.0 || a.post1 != 0.0 || a.shared != 0.0 || a.sll != 0.0 || a.nsll != 0.0)) {
            Acc5 g = acc[u];
            fold_acc(g, a);
            acc[u] = g;
        }
        return;
    }
    if (b == it.U) {  // the scalars: the set records, then the null configurations
        SetRec a = set_zero();
        int nu = 0, nz = 0;  // unseen neighbours, unseen null neighbours
        for (int p = t; p < n_items; p += 256) fold_set(a, srec[p]);
        for (int i = t; i < it.n_nbd; i += 256) {
            const int mk = mark[i];
            nu += mk != -1;
            nz += mk == -2;
        }
        __shared__ SetRec ss[4];
        __shared__ int sc[2][4];
        wave_fold_set(a);
        nu = __ockl_wfred_add_i32(nu);
        nz = __ockl_wfred_add_i32(nz);
        if ((t & 63) == 0) {
            ss[t >> 6] = a;
            sc[0][t >> 6] = nu;
            sc[1][t >> 6] = nz;
        }
        __syncthreads();
        if (t == 0) {
            SetRec g = *sacc;
            for (int q = 0; q < 4; q++) fold_set(g, ss[q]);
            const int unseen = sc[0][0] + sc[0][1] + sc[0][2] + sc[0][3];
            const int nn = sc[1][0] + sc[1][1] + sc[1][2] + sc[1][3] + cnt[kCurNull];
            if (nn > 0) {
                SetRec x = null1;  // null1 scaled to nn null configurations
                x.tot *= nn;
                x.nc0 *= nn;
                x.nc1 *= nn;
                x.npat *= nn;
                fold_set(g, x);
            }
            *sacc = g;
            *sacc_host = g;
            cnt_host[kUnseen] = unseen;
            cnt_host[kNulls] = nn;
            cnt_host[kCurPos] = cnt[kCurPos];
            cnt_host[kCurNull] = cnt[kCurNull];
        }
        return;
    }
    const int i = (b - it.U - 1) * 256 + t;
    if (i >= it.n_nbd) return;
    const int mk = mark[i];
    if (mk == -1) return;  // seen
    const double v = mk == -2 ? it.null_score : score[mk];
    unsigned long long w[4];
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = keys[4 * (size_t)i + q];
    wmap_insert(T, mask, w, v);
}

// the map at a larger capacity: re-insert every entry
__global__ void k_wmap_rehash(const WideMapEntry* __restrict__ old, size_t n, WideMapEntry* __restrict__ T,
                              unsigned long long mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !old[i].state) return;
    unsigned long long w[4];
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = old[i].w[q];
    wmap_insert(T, mask, w, old[i].score);
}

}  // namespace

int launch_sss_eval_wide(const WideProb& W, const SssWideIter& it, const WideMapEntry* T, unsigned long long mask,
                         int* mark, int* cnt, unsigned long long* keys, double* lk_host, int* mark_host, SetRec* srec,
                         Acc5* mrec, double* score, hipStream_t st) {
    const dim3 grid((unsigned)(it.n_nbd + 1)), block(kThreads);
#define PSX_SSS_WIDE_CASE(KM)                                                                                    \
    case KM:                                                                                                     \
        hipLaunchKernelGGL(k_sss_eval_wide<KM>, grid, block, 0, st, W, it, T, mask, mark, cnt, keys, lk_host,       \
                           mark_host, srec, mrec, score);                                                        \
        break;
    switch (it.stride) {
        PSX_SSS_WIDE_CASE(7)
        PSX_SSS_WIDE_CASE(8)
        PSX_SSS_WIDE_CASE(9)
        PSX_SSS_WIDE_CASE(10)
        default: return -1;
    }
#undef PSX_SSS_WIDE_CASE
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sss_post_wide(const SssWideIter& it, const int* mark, const int* cnt, const unsigned long long* keys,
                         const Acc5* mrec, const SetRec* srec, const double* score, SetRec null1, Acc5* acc,
                         SetRec* sacc, SetRec* sacc_host, int* cnt_host, WideMapEntry* T, unsigned long long mask,
                         hipStream_t st) {
    const unsigned blocks = (unsigned)(it.U + 1 + (it.n_nbd + 255) / 256);
    hipLaunchKernelGGL(k_sss_post_wide, dim3(blocks), dim3(256), 0, st, it, mark, cnt, keys, mrec, srec, score, null1,
                       acc, sacc, sacc_host, cnt_host, T, mask);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wide_map_rehash(const WideMapEntry* old, size_t n, WideMapEntry* T, unsigned long long mask,
                           hipStream_t st) {
    hipLaunchKernelGGL(k_wmap_rehash, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, old, n, T, mask);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int warm_module_sss_wide() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_sss_eval_wide<PSX_KWIDE>) == hipSuccess ? 0 : -1;
}

}  // namespace psx
