// psx_wide.hip — wide-set evaluator for gfx950: union sets of PSX_KMAX + 1 ..
// PSX_KWIDE members (exhaustive levels 7..10, user batches of stride 7..10).
//
// The evaluator itself (eval_wide, its LDS image and the butterfly helpers) is
// in psx_wide_dev.h; here are the kernels that feed it canonical and user rows.
#include "psx_wide_dev.h"

namespace psx {
namespace {

// the row of the workgroup into sh.mem (members compacted, -1 after them) and
// sh.k, by wave 0; user rows are validated (sh.ok) and written back compacted
template <int KM>
__device__ __forceinline__ void stage_row(const int* in, int* out, int stride, int U, WideShm<KM>& sh) {
    const int t = threadIdx.x;
    if (t < 64) {
        const int v = t < stride ? in[t] : -1;
        __builtin_amdgcn_wave_barrier();  // (in may alias out: every lane has read its entry)
        const unsigned long long m = __ballot(v >= 0);
        const unsigned long long below = m & ((1ull << t) - 1ull);
        const int pos = __popcll(below);
        const int pl = below ? 63 - __clzll(below) : 0;  // the previous member's lane
        const int pv = __shfl(v, pl);
        const bool bad_lane = v >= 0 && (v >= U || (below != 0ull && v <= pv));
        const bool ok = __ballot(bad_lane) == 0ull;
        if (t < KW) sh.mem[t] = -1;
        __builtin_amdgcn_wave_barrier();
        if (ok && v >= 0) sh.mem[pos] = v;
        __builtin_amdgcn_wave_barrier();
        if (out && t < stride) out[t] = sh.mem[t];
        if (t == 0) {
            sh.k = __popcll(m);
            sh.ok = ok;
        }
    }
    __syncthreads();
}

template <int KM>
__global__ __launch_bounds__(kThreads) void k_eval_wide_sets(WideProb W, const int* __restrict__ sets, int stride,
                                                             SetRec* __restrict__ srec, Acc5* __restrict__ mrec,
                                                             double* __restrict__ score,
                                                             const int* __restrict__ span,
                                                             unsigned long long* __restrict__ tr) {
    __shared__ WideShm<KM> sh;
    const int set = blockIdx.x;
    int base = 0;
    if (span) {
        base = span[0];
        if (set >= span[1] - base) return;
    }
    if (tr && set == 0 && threadIdx.x == 0) tr[0] = wall_clock64();
    stage_row<KM>(sets + (size_t)(base + set) * stride, nullptr, stride, W.U, sh);
    if (!sh.ok || sh.k == 0) return;  // (canonical rows are valid and not empty)
    eval_wide<KM>(W, sh, srec + set, mrec ? mrec + (size_t)set * stride : nullptr, score ? score + set : nullptr,
                  tr);
}

template <int KM>
__global__ __launch_bounds__(kThreads) void k_eval_wide_batch(WideProb W, const int* in, int* out, int stride,
                                                              SetRec null1, double L0, unsigned long long badv,
                                                              unsigned long long* __restrict__ bad,
                                                              unsigned long long* __restrict__ hbad,
                                                              SetRec* __restrict__ srec, Acc5* __restrict__ mrec,
                                                              double* __restrict__ score,
                                                              unsigned long long* __restrict__ tstamp,
                                                              unsigned long long* __restrict__ tr) {
    __shared__ WideShm<KM> sh;
    const int set = blockIdx.x;
    if (set == 0 && threadIdx.x == 0) {
        const unsigned long long c = wall_clock64();
        if (tstamp) *tstamp = c;
        if (tr) tr[0] = c;
    }
    stage_row<KM>(in + (size_t)set * stride, out + (size_t)set * stride, stride, W.U, sh);
    const bool ok = sh.ok;
    if (!ok || sh.k == 0) {
        if (threadIdx.x == 0) {
            if (!ok) {
                *bad = badv;
                *hbad = badv;
            }
            srec[set] = ok ? null1 : set_zero();
            if (score) score[set] = ok ? L0 : 0.0;
        }
        return;
    }
    eval_wide<KM>(W, sh, srec + set, mrec + (size_t)set * stride, score ? score + set : nullptr, tr);
}

}  // namespace

void wide_prior(WideProb& W, int U, double gamma, double sharing_param) {
    const bool sh = sharing_param != 0;  // as log_prior: no sharing term when p == 0
    W.a = sh ? (1 - sharing_param) * 0.5 : 1.0;
    W.b = sh ? sharing_param : 1.0;
    W.la = sh ? std::log((1 - sharing_param) * 0.5) : 0.0;
    W.lb = sh ? std::log(sharing_param) : 0.0;
    for (int k = 0; k <= KW; k++) {
        const double pc = k * std::log(gamma) + (U - k) * std::log(1 - gamma);
        const double l2 = pc * PSX_LOG2E;
        W.lnc[k] = pc;
        W.Ck[k] = std::isfinite(l2) ? (int)std::ceil(l2) : 0;
        W.base[k] = std::isfinite(l2) ? std::exp2(l2 - W.Ck[k]) : 0.0;
    }
}

#define PSX_WIDE_DISPATCH(KERNEL, ...)                                                                   \
    switch (stride) {                                                                                     \
        case 7: hipLaunchKernelGGL(KERNEL<7>, dim3((unsigned)nsets), dim3(kThreads), 0, st, __VA_ARGS__); break; \
        case 8: hipLaunchKernelGGL(KERNEL<8>, dim3((unsigned)nsets), dim3(kThreads), 0, st, __VA_ARGS__); break; \
        case 9: hipLaunchKernelGGL(KERNEL<9>, dim3((unsigned)nsets), dim3(kThreads), 0, st, __VA_ARGS__); break; \
        case 10: hipLaunchKernelGGL(KERNEL<10>, dim3((unsigned)nsets), dim3(kThreads), 0, st, __VA_ARGS__); break; \
        default: return -1;                                                                               \
    }

int launch_eval_wide_sets(const WideProb& W, const int* sets, int stride, size_t nsets, SetRec* srec, Acc5* mrec,
                          double* score, const int* span, unsigned long long* trace, hipStream_t st) {
    if (nsets == 0) return 0;
    PSX_WIDE_DISPATCH(k_eval_wide_sets, W, sets, stride, srec, mrec, score, span, trace)
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_eval_wide_batch(const WideProb& W, const int* in, int* out, int stride, size_t nsets, SetRec null1,
                           double L0, unsigned long long badv, unsigned long long* bad, unsigned long long* hbad,
                           SetRec* srec, Acc5* mrec, double* score, unsigned long long* tstamp,
                           unsigned long long* trace, hipStream_t st) {
    if (nsets == 0) return 0;
    PSX_WIDE_DISPATCH(k_eval_wide_batch, W, in, out, stride, null1, L0, badv, bad, hbad, srec, mrec, score, tstamp,
                      trace)
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
#undef PSX_WIDE_DISPATCH

int warm_module_wide() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_eval_wide_sets<PSX_KWIDE>) == hipSuccess ? 0 : -1;
}

}  // namespace psx
