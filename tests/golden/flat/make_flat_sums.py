#!/usr/bin/env python3
"""Golden exact sums of the three-block flat locus (tests/exact_sums.py
GOLDEN_LOCUS: flat_locus(126, 124, 120, 7), U = 130, 62 pad slots, c = 3,
gamma 0.2, p = 0.6, n = 10000,8000): an off-diagonal k = 3 tile with K >= 1 and
SNPs present in one study only, too large for a live exact sum in a GPU test.

One row per union SNP u with the oracle's exact sums over all union sets
containing u (oracle.member_sums: long-double log-sum-exp): post (study 0,
study 1), sharedPips, sharedLL and notSharedLL as the reference holds them
(postcal.cpp:981-1030, log values, 0 = empty), %.17g.  The header carries the
exact total and no_causal[0..1] (exact_sums.enumerate_patterns, long-double
log-sum-exp over every configuration), the configuration count, the floor (the
serial f64 oracle's, oracle.postcal's, largest deviation from these sums over
the six outputs, from which the GPU test takes its tolerance) and the smallest
single-pattern share, exp(min L - max post).

usage: python tests/golden/flat/make_flat_sums.py   (about a minute of CPU)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import exact_sums as X  # noqa: E402
from oracle import oracle as O  # noqa: E402

seam = X.seam_of(X.GOLDEN_LOCUS)
U, m0 = seam.n_union, int(seam.m[0])
pat = X.enumerate_patterns(seam)
sets = {}
X._set_sums(pat, sets)
rows = []
for u in range(U):
    r = O.member_sums(seam, u)
    rows.append([r["post0"], r["post1"], r["shared"], r["shared_ll"], r["notshared_ll"]])
rows = np.array(rows)
exact = dict(sets, shared=rows[:, 2], shared_ll=rows[:, 3], notshared_ll=rows[:, 4], post=np.zeros(seam.N))
for s in range(2):
    here = seam.union_to_local[s] >= 0
    exact["post"][s * m0 + seam.union_to_local[s, here]] = rows[here, s]
ref = O.postcal(seam)
assert ref["n_configs"] == exact["n_configs"]
floor = max(X.deviations(ref, exact).values())
share = X.smallest_share(pat, exact)
with open(X.GOLDEN_FILE, "w") as f:
    f.write("# flat_locus(126, 124, 120, 7) U=130 c=3 gamma=0.2 p=0.6 n=10000,8000: "
            "u post0 post1 shared shared_ll notshared_ll\n")
    f.write("# header: total no_causal0 no_causal1 n_configs floor smallest_share\n")
    f.write(f"# total {float(exact['total']):.17g} {float(exact['no_causal'][0]):.17g} "
            f"{float(exact['no_causal'][1]):.17g} {exact['n_configs']} {floor:.17g} {share:.17g}\n")
    for u in range(U):
        f.write(f"{u} " + " ".join(f"{v:.17g}" for v in rows[u]) + "\n")
print(f"U={U} configurations={exact['n_configs']} floor={floor:.3e} smallest share={share:.3e} "
      f"share / (20 x 16 x floor) = {share / (320 * floor):.2f}")
