"""The SSS walk of 7 to 10 causal SNPs (psx_run_sss_wide: k_sss_eval_wide and
k_sss_post_wide around the wide-set evaluator) against the oracle's walk."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from pipsort_amd import engine as E
from pipsort_amd import synth
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

FIELDS = ("post", "no_causal", "shared", "shared_ll", "notshared_ll")

# (M0, M1, n_shared, seed) -> c, the oracle walk's n_configs.  U = 14 in all; the
# walks reach sets of c members (the oracle counts other totals at c - 1); the
# first three have members present in one study only, the last misses one SNP
# in study 1.
CASES = {7: ((12, 12, 10, 7), 265_407), 8: ((13, 12, 11, 1), 1_156_860), 9: ((13, 13, 12, 6), 423_907),
         10: ((14, 13, 13, 3), 1_289_313)}


@functools.lru_cache(maxsize=None)
def _case(c):
    M0, M1, shared, seed = CASES[c][0]
    ld, z, _, _, u2l = synth.mixed_locus(M0, M1, shared, seed)
    seam = O.cholesky_seam(ld, z, u2l, (10000, 8000), max_causal=c, sharing_param=0.25)
    return seam, O.postcal(seam, "sss")


@pytest.mark.parametrize("c", sorted(CASES))
def test_sss_wide_walk_matches_oracle(gpu, c):
    seam, ref = _case(c)
    pc = E.PostCal(seam)
    pc.run_sss_wide()
    a = pc.accum()
    assert a.n_configs == ref["n_configs"] == CASES[c][1]
    assert_parity(a, ref, pip_tol=1e-9, ll_rtol=1e-9)
    pc.close()


def test_sss_wide_second_walk_is_the_same_walk(gpu):
    """The kept wide map is cleared per walk and its workspace reused, with an
    exhaustive pass on the same handle in between."""
    pc = E.PostCal(_case(8)[0])
    it1 = pc.run_sss_wide()
    a = pc.accum()
    pc.run_exhaustive()
    it2 = pc.run_sss_wide()
    b = pc.accum()
    assert it1 == it2 and a.total == b.total and a.n_configs == b.n_configs
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    pc.close()


def test_sss_wide_forwards_narrow_handles(gpu):
    ld, z, _, _, u2l = synth.syn_v1(60)
    seam = E.seam_from_arrays(ld, z, u2l, (10000, 8000), max_causal=5, sharing_param=0.25)
    w, n = E.PostCal(seam), E.PostCal(seam)
    assert w.run_sss_wide() == n.run_sss()
    a, b = w.accum(), n.accum()
    assert a.total == b.total and a.n_configs == b.n_configs
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_sss_wide_cli_matches_oracle_cli(gpu, tmp_path):
    """-q 1 -c 8 through the drop-in executable against the oracle's.  (The
    oracle's executable prints no iteration count: the engine's line is held to
    the library walk's count on the same locus.)"""
    M0, M1, shared, seed = CASES[8][0]
    ld, z, names, rows, _ = synth.mixed_locus(M0, M1, shared, seed)
    args = ["-q", "1", "-c", "8", "-l", "ldfiles.txt", "-z", "zfiles.txt", "-m", "snp_map", "-n", "10000,8000",
            "-p", "0.25", "-o", "out"]
    out = {}
    for name, exe in (("engine", E.PIPSORT_BIN), ("oracle", O.CLI)):
        d = synth.write_locus(str(tmp_path / name), ld, z, names, rows)
        r = subprocess.run([exe] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        post = [np.array([[float(v) for v in l.split()[1:]] for l in open(f"{d}/out_study{s}_post.txt").read()
                          .splitlines()[1:]]) for s in range(2)]
        out[name] = (r.stdout.splitlines(), post)
    pc = E.PostCal(_case(8)[0])
    assert [l for l in out["engine"][0] if l.startswith("sss iterations")] == [f"sss iterations = {pc.run_sss_wide()}"]
    pc.close()
    for g, r in zip(out["engine"][1], out["oracle"][1]):
        np.testing.assert_allclose(g, r, rtol=1e-9, atol=0)
