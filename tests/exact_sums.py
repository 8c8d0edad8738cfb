"""Flat loci and exact per-accumulator sums of the oracle's per-pattern values.

A flat locus has null z-scores (z_s = chol(Sigma_s) eps, no planted effect) and
a raised gamma, so every causal level and every study assignment holds a
comparable share of every accumulator it enters: a single dropped, duplicated
or mis-paired configuration moves some log accumulator by far more than the
f64 rounding floor.  The exact sums are max-shifted long-double log-sum-exps of
oracle.eval_patterns' (L, ll), routed into the six outputs as the reference
routes them (postcal.cpp:981-1030, restated by oracle_member_sums), and the
engine is held to them at an ABSOLUTE log tolerance of 16 x the serial f64
oracle's own largest deviation from them (FLOOR below, asserted by
tests/test_exact_sums_cpu.py).  Imported by the tests like tests/loci.py.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import os

import numpy as np

import loci
from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth

SAMPLE_SIZES = (10000, 8000)
SHARING = 0.25
FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")

# The live loci: flat_locus arguments (M0, M1, shared, seed), max_causal, gamma.
LOCI = {
    "u72c3": dict(shape=(66, 66, 60, 5), c=3, gamma=0.2),    # mixed, U = 72 (56 pad slots)
    "u72c2": dict(shape=(66, 66, 60, 5), c=2, gamma=0.2),
    "u72c1": dict(shape=(66, 66, 60, 5), c=1, gamma=0.2),
    "u65c3": dict(shape=(65, 65, 65, 5), c=3, gamma=0.2),    # all shared, U = 65 (63 pad slots)
    "u64c3": dict(shape=(64, 64, 64, 5), c=3, gamma=0.2),    # all shared, U = 64 (no pad)
    "u24c4": dict(shape=(20, 20, 16, 5), c=4, gamma=0.3),    # generic level 4
    "u16c5": dict(shape=(12, 12, 8, 5), c=5, gamma=0.4),     # generic levels 4, 5
    "u12c6": dict(shape=(10, 10, 8, 5), c=6, gamma=0.45),    # generic levels 4 .. 6
    "u16c3": dict(shape=(12, 12, 8, 5), c=3, gamma=0.2),     # the configs-file route
}
# The golden locus (tests/golden/flat/): three 64-blocks, 62 pad slots, 8.3M
# configurations.  Tuned to meet the 20-tolerances condition: at p = 0.25 an
# all-shared level-3 pattern is ~80 x rarer a priori than an all-single one and
# the smallest share (1.1e-9) sits at the tolerance; p = 0.6 balances the two
# (p d^-1 ~ (1 - p) / 2 d^-1/2 with d ~ 8) and raises it to 1.8e-8.  The floor is
# the serial oracle's drift of `total` over 8.3M additions, 1e-11 .. 9e-11 by
# z seed (the per-SNP outputs stay at 5e-12): seed 7 has 1.03e-11.
GOLDEN_LOCUS = dict(shape=(126, 124, 120, 7), c=3, gamma=0.2, p=0.6)
GOLDEN_FILE = os.path.join(loci.GOLDEN, "flat", "flat130c3_sums.txt")

# Largest |O.postcal - exact sums| over the six outputs of each live locus (log
# units), as tests/test_exact_sums_cpu.py recomputes it: the serial f64
# accumulation's own error.  A constant may not be below the recomputed floor.
# Measured with the oracle built by oracle/Makefile (g++ -O2, glibc's exp / log)
# on x86-64 and rounded up to two digits; the serial drift follows the build's
# exp / log rounding, so another toolchain may move a floor by some per cent.
# If test_floor_and_sensitivity's `floor <= FLOOR` trips with no change to the
# oracle or the loci, re-measure (the test prints each floor), raise the
# constant to the new value and keep the 20-tolerances condition, retuning the
# locus if it no longer holds; the engine tolerance follows the constant.
FLOOR = {
    "u72c3": 3.2e-12, "u72c2": 2.2e-13, "u72c1": 1.8e-14, "u65c3": 1.5e-12, "u64c3": 4.5e-12,
    "u24c4": 6.6e-13, "u16c5": 4.5e-13, "u12c6": 5.4e-13, "u16c3": 1.2e-13,
}
# Plan and pool settings for child runs of the GPU exact tests (each is read once
# per process).  With the default knobs the k = 3 a-chunk is 1 below U = 460, so
# the U = 72 / U = 130 plans hold single-a units only and PSX_K3_TAIL (which cuts
# multi-a units) has nothing to cut: PSX_K3_ROUNDS, the dispatch rounds the
# a-chunk is sized for, is lowered to give these plans the a-chunks of 2 and 4 of
# a full-size locus (tests/test_exact_sums_cpu.py::test_plan_coverage).
_ROUNDS = {"PSX_K3_ROUNDS": "0.004"}
VARIANTS = {
    "rounds": dict(_ROUNDS),                                 # multi-a units, the default 5 % tail cut
    "rounds-tail-0": dict(_ROUNDS, PSX_K3_TAIL="0"),         # every multi-a unit kept whole
    "rounds-tail-1": dict(_ROUNDS, PSX_K3_TAIL="1"),         # the whole plan cut into single-a units, tail order
    "rounds-diag-div-2": dict(_ROUNDS, PSX_K3_DIAG_DIV="2"),  # diagonal chunks half the off-diagonal ones
    "rec-csr-1": {"PSX_REC_CSR": "1"},                       # records at their CSR positions at world 1 too
    "rec-csr-0": {"PSX_REC_CSR": "0"},                       # records unit-major at world > 1 too
    "pool-poison": {"PSX_POOL_POISON": "1"},                 # recycled blocks arrive filled with 0xFF bytes
}
CACHE_ENV = "FLAT_EXACT_CACHE"  # a directory: live_exact's sums are kept there across processes

TOL_FACTOR = 16   # engine tolerance = TOL_FACTOR x FLOOR (absolute, log units)
MIN_SHARE_OVER_TOL = 20  # the smallest single-pattern share must be at least this many tolerances


def tol_of(name: str) -> float:
    return TOL_FACTOR * FLOOR[name]


def flat_locus(M0: int, M1: int, shared: int, seed: int):
    """(ld[2], z[2], union_to_local) with synth.mixed_locus's LD and snp map and
    null z-scores z_s = chol(ld_s) @ default_rng(seed + 1000 + s).standard_normal(M_s).
    shared == M0 == M1 gives the all-shared variant."""
    ld, _, _, _, u2l = synth.mixed_locus(M0, M1, shared, seed=seed)
    z = [np.linalg.cholesky(ld[s]) @ np.random.default_rng(seed + 1000 + s).standard_normal(ld[s].shape[0])
         for s in range(2)]
    return ld, z, u2l


def seam_of(spec: dict) -> E.Seam:
    ld, z, u2l = flat_locus(*spec["shape"])
    return E.seam_from_arrays(ld, z, u2l, SAMPLE_SIZES, max_causal=spec["c"],
                              sharing_param=spec.get("p", SHARING), gamma=spec["gamma"])


@dataclasses.dataclass
class Patterns:
    """Every configuration of an exhaustive sweep but the null one: row i is the
    union set sets[i] (ascending, -1 padded to c columns) with the assignment
    x[i] (1 = causal in study 0 only, 2 = study 1 only, 3 = both; 0 padded) and
    the oracle's L (likelihood + prior) and ll (likelihood) of it."""
    sets: np.ndarray   # int32 [n, c]
    x: np.ndarray      # int8 [n, c]
    L: np.ndarray      # float64 [n]
    ll: np.ndarray     # float64 [n]
    null_L: float      # the null configuration's L

    def take(self, keep) -> "Patterns":
        return Patterns(self.sets[keep], self.x[keep], self.L[keep], self.ll[keep], self.null_L)


def enumerate_patterns(seam: E.Seam) -> Patterns:
    """For k = 1..c every union k-set and every one of its 3^k study assignments
    that passes the presence check (postcal.cpp:907-955), evaluated by
    oracle.eval_patterns in one call per (k, assignment)."""
    u2l = np.asarray(seam.union_to_local)
    U, c = u2l.shape[1], int(seam.max_causal)
    present = np.stack([u2l[0] >= 0, u2l[1] >= 0])  # [2, U]
    S, X, Ls, lls = [], [], [], []
    for k in range(1, c + 1):
        sets = np.array(list(itertools.combinations(range(U), k)), dtype=np.int32).reshape(-1, k)
        for xs in itertools.product((1, 2, 3), repeat=k):
            ok = np.ones(len(sets), dtype=bool)
            for j, v in enumerate(xs):
                for s in range(2):
                    if (v >> s) & 1:
                        ok &= present[s, sets[:, j]]
            if not ok.any():
                continue
            sub = sets[ok]
            bits = np.array([[v & 1 for v in xs], [(v >> 1) & 1 for v in xs]], dtype=np.int32)
            L, ll = O.eval_patterns(seam, sub, np.broadcast_to(bits, (len(sub), 2, k)))
            pad = np.full((len(sub), c), -1, dtype=np.int32)
            pad[:, :k] = sub
            xx = np.zeros((len(sub), c), dtype=np.int8)
            xx[:, :k] = xs
            S.append(pad)
            X.append(xx)
            Ls.append(L)
            lls.append(ll)
    null_L = O.postcal(dataclasses.replace(seam, max_causal=0))["total"]
    return Patterns(np.concatenate(S), np.concatenate(X), np.concatenate(Ls), np.concatenate(lls), float(null_L))


def _lse(values) -> np.longdouble:
    """Max-shifted long-double log-sum-exp of a non-empty array."""
    v = np.asarray(values, dtype=np.longdouble)
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def _lse_by(idx, values, n) -> np.ndarray:
    """Per-index max-shifted long-double log-sum-exp: out[i] over values[idx == i], 0 where empty."""
    out = np.zeros(n, dtype=np.longdouble)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    i, v = np.asarray(idx)[order], np.asarray(values, dtype=np.longdouble)[order]
    starts = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])
    mx = np.maximum.reduceat(v, starts)
    lens = np.diff(np.r_[starts, len(i)])
    s = np.add.reduceat(np.exp(v - np.repeat(mx, lens)), starts)
    out[i[starts]] = mx + np.log(s)
    return out


def _member_sums(seam, pat: Patterns, out: dict, members=None):
    """Fill the per-SNP outputs (post, shared, shared_ll, notshared_ll) from the
    patterns; with `members` only those union SNPs' entries, from the patterns
    that contain one of them."""
    u2l = np.asarray(seam.union_to_local)
    U, m0, N = u2l.shape[1], int(seam.m[0]), int(seam.N)
    if members is not None:
        members = np.asarray(sorted(members))
        pat = pat.take(np.isin(pat.sets, members).any(axis=1))
    rows, cols = np.nonzero(pat.sets >= 0)
    u, x = pat.sets[rows, cols], pat.x[rows, cols]
    if members is not None:
        hit = np.isin(u, members)
        rows, u, x = rows[hit], u[hit], x[hit]
    L, ll = pat.L[rows], pat.ll[rows]
    in0, in1 = (x & 1) != 0, (x & 2) != 0
    both = in0 & in1
    new = dict(
        post=_lse_by(np.r_[u2l[0, u[in0]], m0 + u2l[1, u[in1]]], np.r_[L[in0], L[in1]], N),
        shared=_lse_by(u[both], L[both], U),
        shared_ll=_lse_by(u[both], ll[both], U),
        notshared_ll=_lse_by(u[~both], ll[~both], U))
    if members is None:
        out.update(new)
        return
    sel = {"post": np.r_[u2l[0, members][u2l[0, members] >= 0], m0 + u2l[1, members][u2l[1, members] >= 0]]}
    for f, v in new.items():
        at = sel.get(f, members)
        out[f][at] = v[at]


def _set_sums(pat: Patterns, out: dict):
    """total and no_causal: over every pattern and the null configuration."""
    out["total"] = _lse(np.r_[pat.L, pat.null_L])
    out["no_causal"] = np.array([_lse(np.r_[pat.L[~((pat.x >> s) & 1).any(axis=1)], pat.null_L]) for s in range(2)],
                                dtype=np.longdouble)
    out["n_configs"] = len(pat.L) + 1


def exact_accumulators(seam: E.Seam, pat: Patterns) -> dict:
    """The six outputs of the sweep as exact sums of the patterns' values, routed
    as oracle_member_sums routes them: post[N] (L, the SNP causal in that
    study), shared[U] / shared_ll[U] (L / ll, causal in both), notshared_ll[U]
    (ll, causal in one), no_causal[2] (L, no causal SNP in study s, the null
    configuration included), total (every L), and n_configs.  Log values as
    numpy.longdouble; 0 = empty, as in the ABI."""
    out = {}
    _member_sums(seam, pat, out)
    _set_sums(pat, out)
    return out


def update_exact(seam: E.Seam, pat: Patterns, base: dict, members) -> dict:
    """exact_accumulators(seam, pat) where pat differs from base's patterns only
    in patterns containing one of `members`: only those union SNPs' entries,
    total and no_causal are summed again."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    _member_sums(seam, pat, out, members)
    _set_sums(pat, out)
    return out


def smallest_share(pat: Patterns, exact: dict) -> float:
    """exp(min L - max post): the least share any single configuration holds of
    a post sum it enters, i.e. the least a dropped or duplicated configuration
    moves some log accumulator."""
    post = np.asarray(exact["post"], dtype=np.float64)
    return float(np.exp(pat.L.min() - post[post != 0].max()))


def as_accumulators(exact: dict) -> E.Accumulators:
    """Exact sums rounded to the engine's output type (for checks of assert_exact itself)."""
    return E.Accumulators(*(np.asarray(exact[f], dtype=np.float64) for f in FIELDS), float(exact["total"]),
                          int(exact["n_configs"]))


def deviations(got, exact: dict) -> dict:
    """Largest |got - exact| of each output (log units); got an engine
    Accumulators or an oracle.postcal dict.  Empty entries must coincide."""
    dev = {}
    for f in FIELDS + ("total",):
        g = np.atleast_1d(np.asarray(got[f] if isinstance(got, dict) else getattr(got, f), dtype=np.longdouble))
        x = np.atleast_1d(np.asarray(exact[f], dtype=np.longdouble))
        assert g.shape == x.shape, (f, g.shape, x.shape)
        bad = np.flatnonzero((g == 0) != (x == 0))
        assert bad.size == 0, f"{f}[{bad[0]}]: engine {float(g[bad[0]])!r}, exact {float(x[bad[0]])!r} (0 = empty)"
        dev[f] = float(np.abs(g - x).max())
    return dev


def assert_exact(got: E.Accumulators, exact: dict, tol: float) -> dict:
    """Engine accumulators against the exact sums: the same empty entries, the
    same configuration count and every log value within the absolute tolerance.
    Returns the largest deviation per output."""
    assert got.n_configs == exact["n_configs"], f"n_configs: engine {got.n_configs}, exact {exact['n_configs']}"
    dev = deviations(got, exact)
    for f in FIELDS + ("total",):
        if dev[f] > tol:
            g = np.atleast_1d(np.asarray(getattr(got, f), dtype=np.longdouble))
            i = int(np.abs(g - np.atleast_1d(exact[f])).argmax())
            raise AssertionError(f"{f}[{i}]: engine {float(g[i])!r}, exact {float(np.atleast_1d(exact[f])[i])!r}, "
                                 f"deviation {dev[f]:.3e} > tolerance {tol:.3e}")
    return dev


@functools.lru_cache(maxsize=None)
def live(name: str):
    """(seam, patterns, exact sums) of a live locus, computed once per process
    and shared (read-only) by the tests."""
    seam = seam_of(LOCI[name])
    pat = enumerate_patterns(seam)
    return seam, pat, exact_accumulators(seam, pat)


@functools.lru_cache(maxsize=None)
def live_exact(name: str):
    """(seam, exact sums) of a live locus.  Where the environment names a cache
    directory (CACHE_ENV: a parent test's, for its child pytest runs) the sums
    are read from / written to it instead of being summed again per process."""
    d = os.environ.get(CACHE_ENV)
    if not d:
        seam, _, exact = live(name)
        return seam, exact
    path = os.path.join(d, name + ".npz")
    if not os.path.exists(path):
        seam, _, exact = live(name)
        np.savez(path, **exact)
        return seam, exact
    with np.load(path) as z:
        exact = {k: z[k] for k in z.files}
    exact["total"], exact["n_configs"] = exact["total"][()], int(exact["n_configs"])
    return seam_of(LOCI[name]), exact


@functools.lru_cache(maxsize=None)
def golden():
    """(seam, exact sums, floor) of the golden locus from tests/golden/flat/
    (make_flat_sums.py): per-SNP rows `u post0 post1 shared shared_ll
    notshared_ll` under a header `# total nc0 nc1 n_configs floor`."""
    seam = seam_of(GOLDEN_LOCUS)
    with open(GOLDEN_FILE) as f:
        head = [l for l in f if l.startswith("# total")][0].split()
    rows = np.loadtxt(GOLDEN_FILE, comments="#")
    u2l = np.asarray(seam.union_to_local)
    m0 = int(seam.m[0])
    post = np.zeros(seam.N)
    for s in range(2):
        here = u2l[s] >= 0
        post[s * m0 + u2l[s, here]] = rows[here, 1 + s]
    exact = dict(post=post, shared=rows[:, 3], shared_ll=rows[:, 4], notshared_ll=rows[:, 5],
                 no_causal=np.array([float(head[3]), float(head[4])]), total=float(head[2]),
                 n_configs=int(head[5]))
    return seam, exact, float(head[6])
