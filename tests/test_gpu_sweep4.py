"""Level 4 of the exhaustive pass on the tiled k = 4 sweep (k_sweep4): the
host plan's exact shard counts, oracle parity across the 64-blocks, shards and
the exact notSharedLL variant."""
import dataclasses
from math import comb

import numpy as np
import pytest
import torch  # its HIP runtime first, as the gpu fixture and bench.py load it (the plan test loads the engine)

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import _member_pins, assert_parity

FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")


def _seam(M0, M1, shared):
    ld, z, _, _, u2l = synth.mixed_locus(M0, M1, shared, seed=M0 + M1)
    return E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=4, sharing_param=0.25)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("M0,M1,shared", [(2, 3, 1), (36, 36, 7), (70, 70, 10)])  # U = 4, 65, 130
def test_plan_counts_every_set_once(M0, M1, shared, world):
    seam = _seam(M0, M1, shared)
    U = M0 + M1 - shared
    e = [1.0, 0.0, 0.0, 0.0, 0.0]  # elementary symmetric sums of the pattern weights (3: in both studies)
    for w in np.where((seam.union_to_local >= 0).all(axis=0), 3.0, 1.0):
        for k in range(4, 0, -1):
            e[k] += w * e[k - 1]
    sets = cfg = 0
    for r in range(world):
        E.plan_build_ms(U, 4, r, world)  # raises unless the plan builds
        s, c = seam.shard_stats(4, r, world)
        sets, cfg = sets + s, cfg + c
    assert sets == comb(U, 4) and cfg == e[4]


@pytest.fixture(scope="module")
def crossing(gpu):
    """U = 68: p, q, b and c each cross the 64 boundary, one set lies wholly in
    the second block, most members are absent from one study."""
    seam = _seam(36, 36, 4)
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    return seam, pc, pc.accum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crossing", "all_shared"])
def test_parity_with_oracle(gpu, request, name):
    if name == "crossing":
        seam, pc, a = request.getfixturevalue("crossing")
    else:  # every set has all 81 assignments
        seam = _seam(20, 20, 20)
        pc = E.PostCal(seam)
        pc.run_exhaustive()
        a = pc.accum()
    assert a.n_configs == seam.count_configs() <= 2_000_000
    assert pc.timing()["union_sets"] == comb(seam.union_to_local.shape[1], 4)
    assert_parity(a, O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-9)


@pytest.mark.gpu
def test_three_blocks_against_the_generic_evaluator(gpu):
    """U = 130: three 64-blocks, a q-chunk above one (several q per unit).  The
    oracle's member_sums stops at c = 3 and its whole sweep at 2e6 configurations,
    so SNPs {0, 63, 64, 127, 128, 129} are pinned to it on a c = 3 handle, and
    level 4 is added there set by set through the generic evaluator
    (eval_union_batch, held to the oracle by test_gpu_parity): every SNP's five
    accumulators then agree to rtol 1e-10."""
    seam = _seam(66, 66, 2)
    U = 130
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    a = pc.accum()
    assert a.n_configs == seam.count_configs()
    assert pc.timing()["union_sets"] == comb(U, 4)
    seam3 = dataclasses.replace(seam, max_causal=3)
    ref = E.PostCal(seam3)
    ref.run_exhaustive()
    _member_pins(ref.accum(), seam3, [0, 63, 64, 127, 128, 129], rtol=1e-10)
    # every (a < b) followed by every (c < d) with c > b: pairs are sorted by their first member
    pairs = np.stack(np.triu_indices(U, 1), axis=1)
    lo = np.searchsorted(pairs[:, 0], pairs[:, 1], side="right")
    cnt = len(pairs) - lo
    second = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    sets = np.hstack([np.repeat(pairs, cnt, axis=0), pairs[second]])
    assert sets.shape == (comb(U, 4), 4)
    ref.eval_union_batch(sets, accumulate=True)
    b = ref.accum()
    assert b.n_configs == a.n_configs
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x == 0, y == 0), f
        np.testing.assert_allclose(x, y, rtol=1e-10, atol=0, err_msg=f)
    pc.close()
    ref.close()


@pytest.mark.gpu
def test_three_shards_merge_to_the_single_pass(gpu, crossing):
    seam, one, a = crossing
    nb = one.partials_bytes()
    buf = torch.empty(3 * nb, dtype=torch.uint8, device="cuda")
    for r in range(3):
        pc = E.PostCal(seam)
        pc.set_shard(r, 3)
        pc.run_exhaustive()
        pc.export_partials(buf.data_ptr() + r * nb)
        pc.close()
    torch.cuda.synchronize()
    m = E.PostCal(seam)
    m.merge_partials(buf.data_ptr(), 3)
    b = m.accum()
    assert a.n_configs == b.n_configs == seam.count_configs()
    assert abs(a.total - b.total) <= 1e-12 * abs(a.total)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x == 0, y == 0), f
        np.testing.assert_allclose(x, y, rtol=1e-11, atol=0, err_msg=f)


@pytest.mark.gpu
def test_extreme_signal_exact_variant(gpu):
    """The extreme-signal locus of test_gpu_async._extreme cut to 24 SNPs (the
    signals at M / 4 and 3M / 4 as there): z ~ 45 in both studies, so the level
    is re-swept with k_sweep4<true>."""
    M = 24
    idx = np.arange(M)
    ld, z = [], []
    for s, rho in enumerate((0.5, 0.3)):
        sig = rho ** np.abs(idx[:, None] - idx[None, :])
        lam = np.zeros(M)
        lam[M // 4] = 45.0
        lam[3 * M // 4] = 6.0 if s == 0 else 0.0
        eps = np.random.default_rng(9 + s).standard_normal(M)
        z.append(sig @ lam + np.linalg.cholesky(sig) @ eps)
        ld.append(sig)
    u2l = np.stack([idx, idx]).astype(np.int32)
    seam = E.seam_from_arrays(ld, z, u2l, (12000, 9000), max_causal=4, sharing_param=0.3)
    assert seam.count_configs() <= 2_000_000
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    assert pc.timing()["exact_rerun"] != 0
    assert_parity(pc.accum(), O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-10)
    pc.close()
