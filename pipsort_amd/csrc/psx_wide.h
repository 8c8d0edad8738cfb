// psx_wide.h — the wide-set evaluator (psx_wide.hip): union sets of up to
// PSX_KWIDE members, one 256-thread workgroup per set, assignment sums by
// Kronecker butterflies.  The one-wave evaluator of psx_engine.hip keeps every
// set of at most PSX_KMAX members.
#ifndef PSX_WIDE_H
#define PSX_WIDE_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "psx_math.h"

#define PSX_KWIDE 10  // largest union set of the wide evaluator (2^10 subsets per study)

namespace psx {

// What the wide kernels read: the device problem (the engine's pointers, union
// coordinates) and the prior as a product over members (postcal.cpp:27-41):
//   prior(k, nsh) = lnc[k] + nsh lb + (k - nsh) la,  2^{lnc[k] log2e} = 2^{Ck[k]} base[k]
struct WideProb {
    int U, ldg;
    const double* G[2];
    const double* Ad[2];
    const double* y[2];
    const unsigned char* pres;
    double dval[2];
    double a, b;    // a member causal in one study / in both: (1 - p) / 2 and p (1, 1 when p == 0)
    double la, lb;  // their logarithms (nats)
    int Ck[PSX_KWIDE + 1];
    double base[PSX_KWIDE + 1];  // in (1/2, 1]
    double lnc[PSX_KWIDE + 1];   // k ln gamma + (U - k) ln(1 - gamma)
};

// the prior fields of W for a locus of U union SNPs
void wide_prior(WideProb& W, int U, double gamma, double sharing_param);

// Canonical rows ([set][stride], members first, -1 after them), as k_eval_sets:
// record j of a set is its j-th member; span (optional, device [lo, hi)) as there.
// trace (optional, pinned host, 3 words): block 0's clocks at its start, after
// the factorisations and at its end.  7 <= stride <= PSX_KWIDE; -1 on a launch error.
int launch_eval_wide_sets(const WideProb& W, const int* sets, int stride, size_t nsets, SetRec* srec, Acc5* mrec,
                          double* score, const int* span, unsigned long long* trace, hipStream_t st);

// User rows, as k_eval_batch: validated (members strictly ascending, < U; else
// *bad = *hbad = badv and the row adds nothing), compacted from `in` to `out`
// (may be the same rows), an empty row the null configuration (null1, L0).
int launch_eval_wide_batch(const WideProb& W, const int* in, int* out, int stride, size_t nsets, SetRec null1,
                           double L0, unsigned long long badv, unsigned long long* bad, unsigned long long* hbad,
                           SetRec* srec, Acc5* mrec, double* score, unsigned long long* tstamp,
                           unsigned long long* trace, hipStream_t st);

int warm_module_wide();  // load this translation unit's device code (psx_warmup)

}  // namespace psx
#endif
