"""The k = 3 fast walk on ready {b, c} weights: k_bc3_ready stores them relative
to a per-(tile, lane, study) reference exponent, the walk applies one lane scale
2^(ref - Ru) per a instead of one ldexp per step, and a tile in which some lane's
weights span more than kMaxBcSpan = 900 binades runs the robust variant.

M = 144 loci span three 64-blocks of the padded index space (16 + 64 + 64 SNPs),
so the off-diagonal tile (K = 1, C = 2) walks the a's of block 0 through the
pipelined closed-form (SEP) variant, and the diagonal tiles take pipelined and
masked steps.  The reference is the oracle throughout (rtol 1e-10 on the log
accumulators, the suite's bar): oracle.member_sums pins where the whole-sweep
oracle is not needed, the whole sweep where every accumulator is compared.

The wide-tile loci put one strong SNP of block 1 into study 0 only; its z is
chosen from the oracle's own {b, c} weights (eval_patterns of the pair in one
study): per lane c of block 2 the span over the b of block 1, in binades, is
asserted on the host to lie above (z = 38.5: ~920) or under (z = 37.5: ~873)
the threshold.  Marked gpu; run on an MI355X."""
import numpy as np
import pytest

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import _member_pins, assert_parity
from test_gpu_sweep3_lds import M, M80, PINS, _all_finite, _ar1_seam, _bench_locus, _counts, _run

pytestmark = pytest.mark.gpu

K_MAX_BC_SPAN = 900  # psx_sweep3.hip: kMaxBcSpan
# (robust_units, exact_rerun) of the walk before this change (EXPERIMENTS.md section E)
PARENT = {"bench": (0, 0), "extreme": (79, 1), "strong": (79, 0), "wide": (77, 0)}


def _bc_span_bits(seam, bs, cs):
    """[study][c]: log2 of the largest over the smallest {b, c} subset weight of
    study s over b in bs, from the oracle (both members in study s only; the
    prior and the other study's empty set are the same for every pair)."""
    sets = np.array([[b, c] for c in cs for b in bs], dtype=np.int32)
    out = []
    for s in range(2):
        bits = np.zeros((len(sets), 2, 2), dtype=np.int32)
        bits[:, s, :] = 1
        L, _ = O.eval_patterns(seam, sets, bits)
        L = L.reshape(len(cs), len(bs)) / np.log(2.0)
        out.append(L.max(axis=1) - L.min(axis=1))
    return np.array(out)


def test_syn_v1_three_blocks(gpu):
    """All-shared SYN-v1, M = 144: no unit redone, pins of every block."""
    ld, z, _, _, u2l = synth.syn_v1(M)
    seam = E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=3, sharing_param=0.25)
    acc, t = _run(seam)
    print("syn144:", _counts(t))
    assert _counts(t) == (0, 0), t
    assert _all_finite(acc)
    assert acc.n_configs == seam.count_configs()
    _member_pins(acc, seam, sorted(set(PINS) | {M // 4, 3 * M // 4}), rtol=1e-10)


def test_mixed_three_blocks(gpu):
    """Mixed presence, 144 union SNPs (k_sweep3<false>): the whole oracle."""
    ld, z, _, _, u2l = synth.mixed_locus(118, 116, 90, seed=17)
    seam = E.seam_from_arrays(ld, z, u2l, (5000, 9000), max_causal=3, sharing_param=0.4)
    assert np.asarray(seam.union_to_local).shape[1] == M
    ref = O.postcal(seam)
    acc, t = _run(seam)
    print("mixed144:", _counts(t))
    assert acc.n_configs == ref["n_configs"] == seam.count_configs()
    assert _all_finite(acc)
    assert_parity(acc, ref, pip_tol=1e-9, ll_rtol=1e-10)


@pytest.mark.parametrize("name", sorted(M80))
def test_m80_full_accumulators(gpu, name):
    """test_gpu_parity's extreme, strong and wide loci: every accumulator against
    the oracle, and the redone units / exact-rerun bits as before the change."""
    seam = M80[name]()
    acc, t = _run(seam)
    print(name, _counts(t))
    assert _counts(t) == PARENT[name], t
    assert_parity(acc, O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-10)


def test_bench_locus_no_robust_unit(gpu):
    acc, t = _run(_bench_locus())
    print("bench:", _counts(t))
    assert _counts(t) == PARENT["bench"], t
    assert _all_finite(acc)


def _one_study_strong(zb):
    # block 1's u = 50 strong in study 0 only; a moderate signal in block 0
    return _ar1_seam({50: (zb, 0.0), 8: (4.0, 3.0)}, seed=61)


def test_wide_tile_takes_robust_path(gpu):
    seam = _one_study_strong(38.5)
    span = _bc_span_bits(seam, range(16, 80), range(80, 144))
    print("span over the threshold:", span[0].max(), span[1].max())
    assert span[0].max() > K_MAX_BC_SPAN + 4  # (4: the integer binade of a weight is within 1 of its log2)
    acc, t = _run(seam)
    print("wide tile:", _counts(t))
    assert t["robust_units"] > 0, t
    assert_parity(acc, O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-10)


def test_just_under_wide_tile(gpu):
    seam = _one_study_strong(37.5)
    span = _bc_span_bits(seam, range(16, 80), range(80, 144))
    print("span under the threshold:", span[0].max(), span[1].max())
    assert K_MAX_BC_SPAN - 60 < span.max() < K_MAX_BC_SPAN - 4
    acc, t = _run(seam)
    print("under:", _counts(t))
    assert_parity(acc, O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-10)


def test_weak_a_strong_b_and_c(gpu):
    """a of block 0 weak, a b of block 1 and a c of block 2 strong (z = 40 in
    study 0, ~1,150 bits each): the lane's {b, c} reference lies more than
    kMaxRefGap above the wave's {a, c} reference; the unit is redone.  (Such a
    lane's weights also span more than kMaxBcSpan within the tile: a {b, c}
    weight is never far below c's own, so the tile flag sees this locus first.)"""
    seam = _ar1_seam({50: (40.0, 0.0), 110: (40.0, 0.0)}, seed=71)
    acc, t = _run(seam)
    print("weak a:", _counts(t))
    assert t["robust_units"] > 0, t
    assert _all_finite(acc)
    _member_pins(acc, seam, sorted(set(PINS) | {49, 109, 111}), rtol=1e-10)
