"""-b configs rows of 7 to 10 union SNPs: the wide path of psx_run_configs
(k_cfg_eval_wide) against the oracle's configs enumerator and the wide sweep."""
import numpy as np
import pytest

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import _sexp, assert_parity

pytestmark = pytest.mark.gpu

G0 = [[0], [1, 2], [4], [6], [7, 8], [10]]
G1 = [[0], [3], [5], [8], [10]]
FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")


def product_seam(p=0.25):
    ld, z, _, _, u2l = synth.mixed_locus(12, 11, 8, seed=23)
    return E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=3, sharing_param=p)


@pytest.mark.parametrize("p", [0.25, 0.0])
def test_product_file(gpu, p):
    """The product of 6 + 5 groups: 4,608 rows of 0..10 union SNPs (18 row
    blocks, every size in every block) on a handle of max_causal 3; then the
    same rows over three shards, merged."""
    import torch
    seam = product_seam(p)
    rows = synth.construct_configs([G0, G1], seam.m)
    assert rows.shape == (4608, 11)
    pc = E.PostCal(seam)
    pc.run_configs(rows)
    got = pc.accum()
    assert got.n_configs == 4608
    assert_parity(got, O.postcal(seam, "configs", rows), pip_tol=1e-9, ll_rtol=1e-9)
    nb = pc.partials_bytes()
    buf = torch.empty(3 * nb, dtype=torch.uint8, device="cuda")
    for r in range(3):
        x = E.PostCal(seam)
        x.set_shard(r, 3)
        x.run_configs(rows)
        x.export_partials(buf.data_ptr() + r * nb)
        x.close()
    torch.cuda.synchronize()
    m = E.PostCal(seam)
    m.merge_partials(buf.data_ptr(), 3)
    g = m.accum()
    assert g.n_configs == got.n_configs
    assert np.abs(_sexp(g.post, g.total) - _sexp(got.post, got.total)).max() <= 1e-12
    pc.close()
    m.close()


def test_every_configuration_c8(gpu):
    """Every configuration of up to 8 causal SNPs as a shuffled -b file: the
    oracle's enumerator, and the wide-set sweep's accumulators (levels 7, 8)."""
    ld, z, _, _, u2l = synth.mixed_locus(7, 6, 5, seed=13)
    seam = E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=8, sharing_param=0.25)
    rows = synth.all_configs_rows(seam.union_to_local, seam.m, 8)
    rows = rows[np.random.default_rng(1).permutation(rows.shape[0])]
    pc, ex = E.PostCal(seam), E.PostCal(seam)
    pc.run_configs(rows)
    got = pc.accum()
    assert got.n_configs == rows.shape[0] == seam.count_configs() == 8192
    assert_parity(got, O.postcal(seam, "configs", rows), pip_tol=1e-9, ll_rtol=1e-9)
    ex.run_exhaustive()
    ref = ex.accum()
    for f in ("post", "no_causal", "shared"):
        assert np.abs(_sexp(getattr(got, f), got.total) - _sexp(getattr(ref, f), ref.total)).max() <= 1e-12, f
    for f in ("shared_ll", "notshared_ll"):
        np.testing.assert_allclose(getattr(got, f), getattr(ref, f), rtol=1e-11, err_msg=f)
    pc.close()
    ex.close()


def _row(s0, s1, m0=12, width=11):
    g = list(s0) + [m0 + j for j in s1]
    return g + [-1] * (width - len(g))


# 11 union SNPs: the six G0 singles and five study-1 SNPs that share no union SNP with them
ELEVEN = _row((0, 1, 4, 6, 7, 10), (2, 3, 6, 8, 10))
EIGHT = _row((0, 1, 4, 6), (3, 5, 8, 10))
DISORDER = [12 + 1, 0] + [-1] * 9  # a study-1 index before a study-0 index


@pytest.mark.parametrize("rows,code", [([ELEVEN], E.PSX_ERANGE), ([EIGHT, DISORDER], E.PSX_EORDER),
                                       ([ELEVEN, DISORDER], E.PSX_ERANGE), ([DISORDER, ELEVEN], E.PSX_EORDER)])
def test_refusals_in_row_order(gpu, rows, code):
    """More than 10 union SNPs is still out of range, under the wide rules the
    first failing row decides, and a refused file leaves the reset state."""
    seam = product_seam()
    pc, fresh = E.PostCal(seam), E.PostCal(seam)
    with pytest.raises(E.EngineError) as ei:
        pc.run_configs(np.array(rows, dtype=np.int16))
    assert ei.value.code == code
    a, b = pc.accum(), fresh.accum()
    assert a.total == b.total and a.n_configs == b.n_configs
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    pc.close()
    fresh.close()
