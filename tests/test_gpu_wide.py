"""Union sets of 7 to 10 members: the wide-set kernels (psx_wide.hip) against the oracle."""
import numpy as np
import pytest

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")


@pytest.mark.parametrize("M0,M1,shared,c,p", [(8, 7, 6, 8, 0.25), (9, 9, 7, 9, 0.5), (10, 9, 8, 10, 0.25),
                                              (7, 7, 7, 7, 0.0)])
def test_exhaustive_wide_levels(gpu, M0, M1, shared, c, p):
    """Levels 7..c through k_eval_wide_sets, members absent from one study in
    the first three loci; the last is the single 7-set under the prior's p = 0
    branch (no sharing term)."""
    ld, z, _, _, u2l = synth.mixed_locus(M0, M1, shared, seed=M0 + M1)
    seam = E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=c, sharing_param=p)
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    a = pc.accum()
    assert a.n_configs == seam.count_configs()
    assert_parity(a, O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-9)


def test_wide_member_exponent_references(gpu):
    """SNP 2 carries lambda = 60: the oracle's notshared_ll[2] lies 879 nats
    (1,268 bits) under its neighbours, beyond a double's range under one shift
    per set; the halves with and without member j keep their own references."""
    M = 9
    idx = np.arange(M)
    ld, z = [], []
    for s, rho in enumerate((0.5, 0.3)):
        sig = rho ** np.abs(idx[:, None] - idx[None, :])
        lam = np.zeros(M)
        lam[2] = 60.0
        lam[6] = 6.0 if s == 0 else 0.0
        eps = np.random.default_rng(9 + s).standard_normal(M)
        z.append(sig @ lam + np.linalg.cholesky(sig) @ eps)
        ld.append(sig)
    seam = E.seam_from_arrays(ld, z, np.stack([idx, idx]).astype(np.int32), (12000, 9000), max_causal=8,
                              sharing_param=0.3)
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    assert_parity(pc.accum(), O.postcal(seam), pip_tol=1e-9, ll_rtol=1e-10)


def test_wide_user_batches(gpu):
    """A stride-10 batch with rows of every size 0..10 and padding between
    members: scores of the rows of >= 7 members against the oracle's max-|L|
    assignment, the rows of <= 6 members against the narrow kernel at stride 6
    (scores and accumulators); bad rows are refused and add nothing."""
    ld, z, _, _, u2l = synth.syn_v1(40)
    seam = E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=10, sharing_param=0.25)
    rows = np.full((13, 10), -1, np.int32)
    for k in range(11):
        rows[k, :k] = 3 * np.arange(k) + k
    rows[11, [0, 2, 3, 5, 6, 8, 9]] = [1, 5, 6, 11, 20, 30, 39]
    rows[12] = 4 * np.arange(10)
    wide, narrow = E.PostCal(seam), E.PostCal(seam)
    got = wide.eval_union_batch(rows)
    for i, row in enumerate(rows):
        mem = row[row >= 0]
        k = len(mem)
        if k < 7:
            continue
        xs = [[(q // 3 ** j) % 3 + 1 for j in range(k)] for q in range(3 ** k)]
        bits = np.array([[[v & 1 for v in x], [(v >> 1) & 1 for v in x]] for x in xs], dtype=np.int32)
        L, _ = O.eval_patterns(seam, np.repeat(mem[None, :], 3 ** k, axis=0), bits)
        np.testing.assert_allclose(got[i], L[np.argmax(np.abs(L))], rtol=1e-12)
    small = rows[:7]
    sw = wide.eval_union_batch(small, accumulate=True)
    sn = narrow.eval_union_batch(small[:, :6], accumulate=True)
    np.testing.assert_allclose(sw, sn, rtol=1e-12)
    np.testing.assert_allclose(sw, got[:7], rtol=0)
    a, b = wide.accum(), narrow.accum()
    assert a.n_configs == b.n_configs
    assert abs(a.total - b.total) <= 1e-12 * abs(b.total)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f) == 0, getattr(b, f) == 0), f
        np.testing.assert_allclose(getattr(a, f), getattr(b, f), rtol=1e-12, atol=0, err_msg=f)
    for bad in ([0, 1, 2, 3, 4, 5, 6, 9, 8, -1], [0, 1, 2, 3, 4, 5, 6, 7, 8, 40]):
        with pytest.raises(E.EngineError) as ei:
            wide.eval_union_batch(np.concatenate([rows, np.array([bad], np.int32)]), accumulate=True)
        assert ei.value.code == E.PSX_EINVAL
        after = wide.accum()
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(after, f)), f
        assert a.total == after.total and a.n_configs == after.n_configs


def test_sss_stays_narrow(gpu):
    """The SSS walk is sized by PSX_KMAX: a handle of max_causal 8 refuses it."""
    ld, z, _, _, u2l = synth.syn_v1(20)
    pc = E.PostCal(E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=8, sharing_param=0.25))
    with pytest.raises(E.EngineError) as ei:
        pc.run_sss()
    assert ei.value.code == E.PSX_ERANGE
