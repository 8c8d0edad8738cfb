"""The exact-sum checker of the flat loci (tests/exact_sums.py) checked on the
CPU: it agrees with the oracle's own per-SNP checker, its tolerances sit on the
serial oracle's measured error, a single wrong configuration on any live locus
is far outside them, the committed golden sums reproduce, and the k = 3 plans
of the GPU loci hold the unit shapes the GPU tests are meant to reach."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_sums as X
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_sums_match_member_sums_checker():
    """exact_accumulators routes as oracle_member_sums does: every union SNP of
    the U = 72 locus to 1e-13 absolute; no_causal and total equal the whole
    oracle within that locus's floor."""
    seam, pat, exact = X.live("u72c3")
    m0 = int(seam.m[0])
    for u in range(seam.n_union):
        r = O.member_sums(seam, u)
        l0, l1 = seam.union_to_local[:, u]
        got = [exact["post"][l0] if l0 >= 0 else 0.0, exact["post"][m0 + l1] if l1 >= 0 else 0.0,
               exact["shared"][u], exact["shared_ll"][u], exact["notshared_ll"][u]]
        want = [r["post0"], r["post1"], r["shared"], r["shared_ll"], r["notshared_ll"]]
        assert [g == 0 for g in got] == [w == 0 for w in want], u
        assert max(abs(float(g) - w) for g, w in zip(got, want)) <= 1e-13, (u, got, want)
    ref = O.postcal(seam)
    assert ref["n_configs"] == exact["n_configs"] == seam.count_configs()
    assert np.abs(np.asarray(ref["no_causal"]) - exact["no_causal"]).max() <= X.FLOOR["u72c3"]
    assert abs(ref["total"] - exact["total"]) <= X.FLOOR["u72c3"]


def _mutations(pat: X.Patterns):
    """Three wrong pattern lists: (name, patterns, union SNPs whose sums change)."""
    c = pat.sets.shape[1]
    i = int(pat.L.argmin())
    keep = np.ones(len(pat.L), dtype=bool)
    keep[i] = False
    yield "smallest-share pattern removed", pat.take(keep), pat.sets[i][pat.sets[i] >= 0]
    top = np.flatnonzero(pat.sets[:, c - 1] >= 0)  # the level-c patterns
    med = int(top[np.argsort(pat.L[top], kind="stable")[len(top) // 2]])
    # the patterns of the sets {a, b, c'} with the median pattern's {a, b} and assignment
    mates = top[(pat.sets[top, :c - 1] == pat.sets[med, :c - 1]).all(axis=1) & (pat.x[top] == pat.x[med]).all(axis=1)
                & (top != med)]
    j = int(mates[np.abs(pat.L[mates] - pat.L[med]).argmax()])
    L = pat.L.copy()
    L[med], L[j] = pat.L[j], pat.L[med]
    yield "L of {a, b, c} and {a, b, c'} swapped", dataclasses.replace(pat, L=L), [pat.sets[med, c - 1],
                                                                                  pat.sets[j, c - 1]]
    L = pat.L.copy()
    L[med] += np.log1p(1e-3)
    yield "a median level-c pattern scaled by 1 + 1e-3", dataclasses.replace(pat, L=L), pat.sets[med]


@pytest.mark.parametrize("name", sorted(X.LOCI))
def test_floor_and_sensitivity(name):
    """Per live locus: the serial f64 oracle's largest deviation from the exact
    sums does not exceed the FLOOR constant the tolerance is taken from; the
    smallest single-pattern share is at least 20 tolerances; and assert_exact,
    at that tolerance, passes the exact sums and flags each of three sums made
    from a pattern list with one wrong configuration."""
    seam, pat, exact = X.live(name)
    ref = O.postcal(seam)
    assert ref["n_configs"] == exact["n_configs"]
    dev = X.deviations(ref, exact)
    floor, tol = max(dev.values()), X.tol_of(name)
    share = X.smallest_share(pat, exact)
    print(f"{name}: {exact['n_configs']} configurations, floor {floor:.3e} (constant {X.FLOOR[name]:.1e}), "
          f"tolerance {tol:.2e}, smallest share {share:.3e} = {share / tol:.0f} tolerances")
    assert floor <= X.FLOOR[name], dev
    assert share >= X.MIN_SHARE_OVER_TOL * tol, (share, tol)
    X.assert_exact(X.as_accumulators(exact), exact, tol)
    for what, wrong, members in _mutations(pat):
        bad = X.update_exact(seam, wrong, exact, [int(u) for u in members])
        bad["n_configs"] = exact["n_configs"]  # the values must flag it, not the count
        with pytest.raises(AssertionError):  # a deviation, or (c = 1) an entry left empty
            X.assert_exact(X.as_accumulators(bad), exact, tol)
            pytest.fail(f"{name}: not flagged: {what}")


def test_update_exact_equals_full_recompute():
    """update_exact (only the touched SNPs summed again) equals exact_accumulators
    of the mutated list."""
    seam, pat, exact = X.live("u16c5")
    for _, wrong, members in _mutations(pat):
        a = X.update_exact(seam, wrong, exact, [int(u) for u in members])
        b = X.exact_accumulators(seam, wrong)
        for f in X.FIELDS + ("total", "n_configs"):
            assert np.array_equal(a[f], b[f]), f


def test_golden_header_sensitivity():
    """The golden locus's tolerance (16 x the floor in its header) is at most
    1/20 of its smallest single-pattern share (also in the header)."""
    with open(X.GOLDEN_FILE) as f:
        head = [l for l in f if l.startswith("# total")][0].split()
    floor, share = float(head[6]), float(head[7])
    assert share >= X.MIN_SHARE_OVER_TOL * X.TOL_FACTOR * floor, (share, floor)


@pytest.mark.parametrize("u", [0, 64, 129])
def test_flat_golden_sums_reproduce(u):
    """The committed golden sums (tests/golden/flat/, made by make_flat_sums.py)
    are the oracle's: recompute three SNPs."""
    seam, exact, _ = X.golden()
    r = O.member_sums(seam, u)
    l0, l1 = seam.union_to_local[:, u]
    m0 = int(seam.m[0])
    want = [exact["post"][l0] if l0 >= 0 else 0.0, exact["post"][m0 + l1] if l1 >= 0 else 0.0,
            exact["shared"][u], exact["shared_ll"][u], exact["notshared_ll"][u]]
    got = [r["post0"], r["post1"], r["shared"], r["shared_ll"], r["notshared_ll"]]
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    assert exact["n_configs"] == seam.count_configs()


_PLAN_CHILD = """
import collections, json, sys
from pipsort_amd import engine as E
out = collections.Counter()
for U, world in ((130, 1), (72, 8), (130, 8)):
    for r in range(world):
        for a0, a1, z, w in E.plan_units_k3(U, r, world):
            K, C = z & 0xFFFF, w & 0xFFFF
            out["%d %s" % (a1 - a0, "diagonal" if K == C else "off-diagonal K>=1" if K >= 1 else "off-diagonal K=0")] += 1
print(json.dumps(out))
"""


def _plan_units(env):
    """{(a1 - a0, unit kind): count} over the k = 3 plans the GPU exact tests run
    (U = 130 at world 1, U = 72 and U = 130 at world 8; host only,
    psx_plan_units_k3), cut in a child process under the plan knobs `env` (the
    knobs are read once per process)."""
    r = subprocess.run([sys.executable, "-c", _PLAN_CHILD], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return {(int(k.split(" ", 1)[0]), k.split(" ", 1)[1]): n for k, n in json.loads(r.stdout).items()}


def test_plan_coverage():
    """The unit shapes the GPU exact tests reach.  With the default knobs the
    a-chunk (sized from the whole plan's work) is 1 on every plan below U = 460,
    so the U = 72 / U = 130 plans hold single-a units only: diagonal ones
    (K == C) and, at U = 130, the off-diagonal tile K = 1, C = 2 (K >= 1; its a
    are the slots 62, 63 of block 0 above the 62 pad slots).  The variants of
    exact_sums.VARIANTS that lower PSX_K3_ROUNDS (the dispatch rounds the
    a-chunk is sized for) bring the multi-a walk of the full-size loci to these
    sizes: a-chunks of 2 and 4 on diagonal and off-diagonal units, PSX_K3_TAIL=1
    then cutting them into single-a units in the tail order, PSX_K3_TAIL=0
    keeping every one whole, PSX_K3_DIAG_DIV=2 halving the diagonal chunk."""
    base = _plan_units({})
    assert set(base) == {(1, "diagonal"), (1, "off-diagonal K>=1")}, base
    by = {name: _plan_units(env) for name, env in X.VARIANTS.items() if "PSX_K3_ROUNDS" in env}
    rounds, whole, cut, div = by["rounds"], by["rounds-tail-0"], by["rounds-tail-1"], by["rounds-diag-div-2"]
    assert {(4, "diagonal"), (2, "diagonal"), (2, "off-diagonal K>=1")} <= set(rounds), rounds
    assert (1, "diagonal") in rounds and (1, "off-diagonal K>=1") in rounds  # the default 5 % tail, cut to single a
    assert set(whole) == {(4, "diagonal"), (2, "diagonal"), (2, "off-diagonal K>=1")}, whole
    # TAIL=1 cuts the whole plan (but a unit or two that the running work sum's rounding leaves whole)
    assert cut[(1, "diagonal")] > 20 * sum(n for (a, _), n in cut.items() if a > 1), cut
    assert cut[(1, "off-diagonal K>=1")] == 2 * whole[(2, "off-diagonal K>=1")], cut
    assert max(a for a, kind in div if kind == "diagonal") == 2 and (2, "off-diagonal K>=1") in div, div
    # every variant's plans hold the same a of the same tiles
    for units in (rounds, whole, cut, div):
        assert sum(a * n for (a, _), n in units.items()) == sum(a * n for (a, _), n in base.items())
