// psx_sss_wide.h — the SSS walk's device side for max_causal 7 .. PSX_KWIDE
// (psx_sss_wide.hip): the wide set map, one iteration's evaluation of the
// current configuration and its neighbourhood on the wide-set evaluator, and
// the post stage; and what both walks' device code shares (the set keys' field
// width, the hash mixer, the iteration counters).  The host walk is in
// psx_engine.hip (run_sss_wide, on the helpers it shares with run_sss); the
// neighbourhood geometry, the neighbour order and the draw of the next
// configuration are in psx_sample.h.
#ifndef PSX_SSS_WIDE_H
#define PSX_SSS_WIDE_H

#include "psx_wide.h"

namespace psx {

// a sorted set as words of three (index + 1) fields: two words for the narrow
// walk's sets of <= PSX_KMAX members, four for <= PSX_KWIDE
constexpr int kKeyBits = 21;

__host__ __device__ inline unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// A sorted set of up to PSX_KWIDE members as four words of three (index + 1)
// fields of 21 bits (the narrow walk's packing, extended), its score, and the
// slot's state (0: empty).  Open addressing, linear probing, load <= 1/2.
struct WideMapEntry {
    unsigned long long w[4];
    double score;
    int state, pad;
};
static_assert(sizeof(WideMapEntry) == 48, "wide map entry");

// one iteration's neighbourhood geometry (sss_postcal.cpp:166-186): item 0 is
// the current configuration, item i + 1 neighbour i in the order swap (member
// slot fastest) ++ minus ++ plus
struct SssWideIter {
    int cur[PSX_KWIDE];  // ascending, -1 after the k members
    int k, U, stride, num_zero, num_minus, num_plus, n_nbd;
    double null_score;   // K + L0: a null configuration's L
};

// The iteration counters (device cnt[]): the eval's block 0 writes the current
// configuration's two (kCurPos: 0 if it is evaluated, else -1; kCurNull: 1 if
// it is an unseen null configuration), the post's scalar block counts the
// unseen neighbours and null configurations from mark[] (no contended atomics
// in the eval) and copies all four to pinned host memory.
enum { kUnseen = 0, kNulls = 1, kCurPos = 2, kCurNull = 3, kNCnt = 4 };

// Items 0 .. n_nbd: row, key, probe of T, and the evaluation of every unseen
// set of 1 .. stride members (stride = max_causal, 7 .. PSX_KWIDE).  Per item p:
// srec[p], mrec[p * stride + j] (zero records for a seen or null item),
// score[p]; per neighbour i: mark[i] (-1 seen, -2 unseen null, else i + 1),
// keys[4 i ..] (its packed set) and, in pinned host memory for the host to
// read after the launch has completed, its weight lk_host[i] and mark_host[i].
int launch_sss_eval_wide(const WideProb& W, const SssWideIter& it, const WideMapEntry* T, unsigned long long mask,
                         int* mark, int* cnt, unsigned long long* keys, double* lk_host, int* mark_host, SetRec* srec,
                         Acc5* mrec, double* score, hipStream_t st);

// Folds the iteration's records into acc[U] / *sacc (with the null
// configurations, null1 each), copies the scalars and counters to host memory
// and inserts every unseen neighbour's score into T.
int launch_sss_post_wide(const SssWideIter& it, const int* mark, const int* cnt, const unsigned long long* keys,
                         const Acc5* mrec, const SetRec* srec, const double* score, SetRec null1, Acc5* acc,
                         SetRec* sacc, SetRec* sacc_host, int* cnt_host, WideMapEntry* T, unsigned long long mask,
                         hipStream_t st);

// every entry of old[0 .. n) into the (cleared) table T of mask + 1 slots
int launch_wide_map_rehash(const WideMapEntry* old, size_t n, WideMapEntry* T, unsigned long long mask,
                           hipStream_t st);

int warm_module_sss_wide();  // load this translation unit's device code (psx_warmup_for)

}  // namespace psx
#endif
