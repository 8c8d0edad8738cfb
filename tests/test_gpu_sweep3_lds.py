"""The k = 3 walk without the {a, b} quadratic form and pivot factor in LDS: the
{a, b, c} weight is the slot's {a, b} weight times c's extension factor, and the
redo test adds the slot's exponent to the extension's.

The loci span three 64-blocks of the padded index space (M = 144: 16 + 64 + 64
SNPs), so the off-diagonal tile (K = 1, C = 2) walks real a's of block 0 through
the pipelined closed-form (SEP) variant; loci of up to 128 SNPs only ever run
diagonal tiles.  The whole-sweep oracle takes ~25 s on the 13.3M configurations
of the all-shared loci, so those pin a dozen SNPs each (every block, both block
borders, the signals) against the oracle's exact per-SNP sums over every union
set holding the SNP (oracle.member_sums; log accumulators at rtol 1e-10, the
suite's bar for the LL columns and tighter than its 1e-9 PIPs); the mixed locus
(5.8M configurations, ~8 s) takes the whole-sweep oracle and assert_parity.
The pins cover the per-SNP accumulators only: the normaliser and noCausal of
the all-shared loci are not compared (those of the mixed locus are, and the
pass-mode test holds them bitwise across modes).

The redo test is guarded by counts: robust_units and exact_rerun of every
locus here, of the bench locus and of test_gpu_parity's three M = 80 loci
equal what the walk gave while it still read the {a, b} form and pivot factor
per step (PARENT, read off that build).  More redone units would only cost
speed, fewer would pass wherever the missed ones happen not to overflow.
Marked gpu; run on an MI355X."""
import numpy as np
import pytest

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import _member_pins, assert_parity

pytestmark = pytest.mark.gpu

M = 144  # pad 48: blocks of 16, 64, 64 SNPs (u 0..15, 16..79, 80..143)
FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")


def _ar1_seam(signals, seed, M=M):
    """Two-study AR(1) locus (the pattern of test_gpu_parity's M = 80 loci);
    signals: {u: (lambda study 0, lambda study 1)}."""
    idx = np.arange(M)
    ld, z = [], []
    for s, rho in enumerate((0.5, 0.3)):
        sig = rho ** np.abs(idx[:, None] - idx[None, :])
        lam = np.zeros(M)
        for u, l in signals.items():
            lam[u] = l[s]
        eps = np.random.default_rng(seed + s).standard_normal(M)
        z.append(sig @ lam + np.linalg.cholesky(sig) @ eps)
        ld.append(sig)
    u2l = np.stack([idx, idx]).astype(np.int32)
    return E.seam_from_arrays(ld, z, u2l, (12000, 9000), max_causal=3, sharing_param=0.3)


def _plain_locus():
    # one moderate signal in each block
    return _ar1_seam({8: (4.0, 3.0), 50: (5.0, 5.0), 110: (4.0, 0.0)}, seed=41)


def _strong_locus(u):
    # z ~ 30 in both studies: ~570 bits per study, beyond kMaxRefGap over both
    return _ar1_seam({u: (30.0, 30.0), (u + 70) % M: (5.0, 0.0)}, seed=51 + u)


def _mixed_locus():
    # 140 union SNPs, 46 of them in one study only
    ld, z, _, _, u2l = synth.mixed_locus(118, 116, 94, seed=13)
    return E.seam_from_arrays(ld, z, u2l, (5000, 9000), max_causal=3, sharing_param=0.4)


def _bench_locus():
    # bench.py's flagship workload: SYN-v1 M = 1000, -c 3 -p 0.25 -n 10000,8000
    ld, z, _, _, u2l = synth.syn_v1(1000)
    return E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=3, sharing_param=0.25)


# test_gpu_parity's M = 80 loci (test_extreme_signal_exact_rerun,
# test_strong_signal_robust_units, test_wide_lane_spread_robust_units)
M80 = {"extreme": lambda: _ar1_seam({20: (45.0, 45.0), 60: (6.0, 0.0)}, seed=9, M=80),
       "strong": lambda: _ar1_seam({50: (30.0, 30.0), 10: (5.0, 0.0)}, seed=19, M=80),
       "wide": lambda: _ar1_seam({70: (20.0, 20.0), 5: (4.0, 0.0)}, seed=29, M=80)}

STRONG = {"strong_b": 50, "strong_a": 8, "strong_c": 110}
# (robust_units, exact_rerun) of the walk before this change
PARENT = {"bench": (0, 0), "extreme": (79, 1), "strong": (79, 0), "wide": (77, 0),
          "plain": (0, 0), "mixed": (0, 0), "strong_b": (159, 0), "strong_a": (143, 0), "strong_c": (159, 0)}


def _counts(t):
    return (t["robust_units"], t["exact_rerun"])
PINS = (0, 8, 15, 16, 17, 50, 51, 79, 80, 110, 120, 143)


def _pins(acc, seam, extra=()):
    assert acc.n_configs == seam.count_configs() == 1 + 3 * M + 9 * (M * (M - 1) // 2) + 27 * (M * (M - 1) * (M - 2) // 6)
    _member_pins(acc, seam, sorted(set(PINS) | set(extra)), rtol=1e-10)


def _run(seam):
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    acc, t = pc.accum(), pc.timing()
    pc.close()
    return acc, t


def _all_finite(acc):
    return all(np.isfinite(getattr(acc, f)).all() for f in FIELDS) and np.isfinite(acc.total)


def test_plain_three_blocks(gpu):
    seam = _plain_locus()
    acc, t = _run(seam)
    print("plain:", t["robust_units"], t["exact_rerun"])
    assert _counts(t) == PARENT["plain"] == (0, 0), t
    assert _all_finite(acc)
    _pins(acc, seam)


@pytest.mark.parametrize("name", sorted(STRONG))
def test_strong_member(gpu, name):
    """z ~ 30 in block 1 (the b of the off-diagonal tile: n_abc - n_ac crosses
    kMaxRefGap), block 0 (an a) or block 2 (a c: the kMaxSpread path)."""
    u = STRONG[name]
    seam = _strong_locus(u)
    acc, t = _run(seam)
    print(name, t["robust_units"], t["exact_rerun"])
    assert t["robust_units"] > 0 and _counts(t) == PARENT[name], t
    assert _all_finite(acc)
    _pins(acc, seam, extra=(u, u - 1, u + 1, (u + 70) % M))


def test_mixed_membership(gpu):
    """A third of the SNPs in one study only (absent b and absent c among the
    walk's members): the ALLPRES = false instantiation."""
    seam = _mixed_locus()
    ref = O.postcal(seam)
    pres = (np.asarray(seam.union_to_local) >= 0)
    assert 40 <= int((pres.sum(axis=0) == 1).sum()) <= 50
    acc, t = _run(seam)
    print("mixed:", t["robust_units"], t["exact_rerun"])
    assert _counts(t) == PARENT["mixed"], t
    assert acc.n_configs == ref["n_configs"] == seam.count_configs()
    assert _all_finite(acc)
    assert_parity(acc, ref, pip_tol=1e-9, ll_rtol=1e-10)


@pytest.mark.parametrize("name", ["bench"] + sorted(M80))
def test_redo_counts_equal_parent(gpu, name):
    """The units redone by the robust variant and the exact-rerun bits on the
    bench locus and the three M = 80 loci (extreme signal, strong signal, wide
    lane spread): as before the change."""
    acc, t = _run(_bench_locus() if name == "bench" else M80[name]())
    print(name, t["robust_units"], t["exact_rerun"])
    assert _counts(t) == PARENT[name], t
    assert _all_finite(acc)


def test_pass_modes_bitwise(gpu):
    """Synchronous, asynchronous and two consecutive asynchronous passes: the
    fold order is the same, so the accumulators are bitwise equal."""
    seam = _plain_locus()
    a, _t = _run(seam)
    for passes in (1, 2):
        pc = E.PostCal(seam)
        for _ in range(passes):
            pc.run_exhaustive_async()
        assert pc.sync() is False
        b = pc.accum()
        pc.close()
        assert b.n_configs == a.n_configs and b.total == a.total
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), (passes, f)
