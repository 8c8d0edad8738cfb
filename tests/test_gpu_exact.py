"""Every route of the engine against exact sums on flat loci (tests/exact_sums.py).

A flat locus has null z-scores and a raised gamma: every configuration holds a
share of every accumulator it enters that is far above the f64 rounding floor,
so one dropped, duplicated, mis-weighted or mis-routed configuration in any
sweep kernel or merge fails here.  The engine's log accumulators are held to
long-double sums of the oracle's per-pattern values at an ABSOLUTE tolerance of
16 x the serial f64 oracle's own largest deviation from those sums (the
per-locus FLOOR constants / the golden file's header; at most 1/20 of the
locus's smallest single-pattern share, tests/test_exact_sums_cpu.py).

Largest engine deviation per locus, measured on an MI355X (log units, over the
six outputs and every route the locus is run through; tolerance in brackets):
  u65c3 9.5e-15 [2.4e-11]    u72c3 9.8e-15 [5.1e-11]    u64c3 1.04e-14 [7.2e-11]
  u130c3 2.8e-14 [1.65e-10]  u72c2 1.46e-14 [3.5e-12]   u72c1 1.53e-14 [2.9e-13]
  u24c4 6.3e-15 [1.06e-11]   u16c5 2.1e-15 [7.2e-12]    u12c6 3.1e-15 [8.6e-12]
  u16c3 (configs rows) 3.4e-15 [1.9e-12]
i.e. one ulp of the log values (magnitudes 17 .. 166) on every route, shards,
host fold, union batch and the plan / pool variants (the multi-a k = 3 units
of lowered PSX_K3_ROUNDS among them) included: the engine's tree
folds sit two to three orders below the serial oracle's own drift.
Marked gpu; run on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_sums as X
from pipsort_amd import engine as E
from pipsort_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = "u130c3"


def _locus(name):
    """(seam, exact sums, tolerance) of a live locus or the golden one."""
    if name == GOLDEN:
        seam, exact, floor = X.golden()
        return seam, exact, X.TOL_FACTOR * floor
    seam, exact = X.live_exact(name)
    return seam, exact, X.tol_of(name)


def _check(label, got, exact, tol):
    """Print the deviations, then hold them to the tolerance."""
    assert got.n_configs == exact["n_configs"], (label, got.n_configs, exact["n_configs"])
    dev = X.deviations(got, exact)
    print(f"\nexact-dev {label}: max {max(dev.values()):.3e} tol {tol:.3e} "
          + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    X.assert_exact(got, exact, tol)


def _fast(t):
    """The fast variants are what ran: no exact rerun, no unit redone by the robust variant."""
    assert t["exact_rerun"] == 0 and t["robust_units"] == 0, t


def _bitwise(a, b):
    assert a.n_configs == b.n_configs and a.total == b.total
    for f in X.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.mark.parametrize("name", ["u65c3", "u72c3", "u64c3", GOLDEN, "u72c2", "u72c1", "u24c4", "u16c5", "u12c6"])
def test_run_exhaustive(gpu, name):
    """c = 3: k_sweep3, k_sweep<2>, level 1 and the record merge, with 63 pad
    slots (U = 65), mixed presence (U = 72), no pad (U = 64) and three blocks
    with an off-diagonal tile (U = 130, golden file); c = 2 and c = 1; the
    generic levels 4 .. 6."""
    seam, exact, tol = _locus(name)
    pc = E.PostCal(seam)
    pc.run_exhaustive()
    _fast(pc.timing())
    _check(name, pc.accum(), exact, tol)
    pc.close()


@pytest.mark.parametrize("name", ["u72c3", "u72c2"])
def test_async_pass(gpu, name):
    """run_exhaustive_async + sync: bitwise the synchronous pass, and exact."""
    seam, exact, tol = _locus(name)
    a, b = E.PostCal(seam), E.PostCal(seam)
    a.run_exhaustive()
    b.run_exhaustive_async()
    assert b.sync() is False
    _fast(b.timing())
    _bitwise(a.accum(), b.accum())
    _check(name + " async", b.accum(), exact, tol)
    a.close()
    b.close()


@pytest.mark.parametrize("name,world", [("u72c3", 2), ("u72c3", 3), ("u72c3", 8), (GOLDEN, 8)])
def test_shards(gpu, name, world):
    """set_shard + export_partials + merge_partials: the merged accumulators are
    held to the exact sums themselves (not to the single pass), and so is the
    host fold of the same images (psx_fold_partials_host), read back through a
    one-image merge."""
    import torch
    seam, exact, tol = _locus(name)
    nb = None
    for r in range(world):
        pc = E.PostCal(seam)
        pc.set_shard(r, world)
        if nb is None:
            nb = pc.partials_bytes()
            buf = torch.empty(nb * world, dtype=torch.uint8, device="cuda")
        pc.run_exhaustive()
        _fast(pc.timing())
        pc.export_partials(buf.data_ptr() + r * nb)
        pc.close()
    torch.cuda.synchronize()
    m = E.PostCal(seam)
    m.merge_partials(buf.data_ptr(), world)
    _check(f"{name} world {world} device merge", m.accum(), exact, tol)
    m.close()
    folded = E.fold_partials_host(buf.cpu().numpy().reshape(world, nb))
    one = torch.from_numpy(folded).cuda()
    torch.cuda.synchronize()
    h = E.PostCal(seam)
    h.merge_partials(one.data_ptr(), 1)
    _check(f"{name} world {world} host fold", h.accum(), exact, tol)
    h.close()


def test_multi_handle(gpu):
    """MultiPostCal over two shards of one device."""
    seam, exact, tol = _locus("u72c3")
    many = E.MultiPostCal(seam, [0, 0])
    many.run_exhaustive()
    _fast(many.timing())  # (any shard's exact flag; the first shard's robust count)
    _check("u72c3 multi [0, 0]", many.accum(), exact, tol)
    many.close()


def test_union_batch_accumulate(gpu):
    """The SSS evaluator's accumulate path and the member merge fed every union
    set of size 1 .. 3 once, plus one all -1 row (the null configuration): its
    accumulators are the exhaustive sweep's exact sums.  One batch (62,269
    rows), and the same rows in chunks of 5,000 (the other merge route)."""
    import itertools
    seam, exact, tol = _locus("u72c3")
    U = seam.n_union
    rows = [[-1, -1, -1]]
    for k in (1, 2, 3):
        rows += [list(s) + [-1] * (3 - k) for s in itertools.combinations(range(U), k)]
    rows = np.array(rows, dtype=np.int32)
    one, many = E.PostCal(seam), E.PostCal(seam)
    one.eval_union_batch(rows, accumulate=True)
    _check("u72c3 union batch", one.accum(), exact, tol)
    for i in range(0, len(rows), 5000):
        many.eval_union_batch(rows[i:i + 5000], accumulate=True)
    _check("u72c3 union batch in chunks of 5000", many.accum(), exact, tol)
    one.close()
    many.close()


def test_run_configs_every_configuration(gpu):
    """A configs file listing every configuration of the U = 16 locus at c = 3,
    shuffled: the exhaustive sweep's exact sums."""
    seam, exact, tol = _locus("u16c3")
    rows = synth.all_configs_rows(seam.union_to_local, seam.m, 3)
    rows = rows[np.random.default_rng(16).permutation(len(rows))]
    pc = E.PostCal(seam)
    pc.run_configs(rows)
    _check("u16c3 configs rows", pc.accum(), exact, tol)
    pc.close()


def test_plan_and_pool_variants(gpu, tmp_path):
    """The c = 3 exhaustive cases and the world-8 shard cases above under each
    plan / pool setting of exact_sums.VARIANTS, which no other test runs: the
    multi-a k = 3 units of a full-size plan (PSX_K3_ROUNDS lowered: a-chunks of
    2 and 4, whole, tail-cut and with halved diagonal chunks), records at CSR
    positions / unit-major at either world size, and a poisoned pool.  One
    child pytest per setting (the settings are read once per process), one
    after the other: the first child that fails ends the test and nothing is
    started after it.  The children read the live loci's exact sums from a
    cache directory instead of summing them again."""
    mod = os.path.join(ROOT, "tests", "test_gpu_exact.py")
    live = ["u72c3", "u65c3", "u64c3"]
    for name in live:
        np.savez(os.path.join(tmp_path, name + ".npz"), **X.live_exact(name)[1])
    ids = [f"{mod}::test_run_exhaustive[{name}]" for name in live + [GOLDEN]]
    ids += [f"{mod}::test_shards[u72c3-8]", f"{mod}::test_shards[{GOLDEN}-8]"]
    for label, var in X.VARIANTS.items():
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider"]
                           + ids, cwd=ROOT, env=dict(os.environ, **var, **{X.CACHE_ENV: str(tmp_path)}),
                           capture_output=True, text=True, timeout=300)
        print(f"variant {label} {var}:\n" + "\n".join(l for l in r.stdout.splitlines() if l.startswith("exact-dev")))
        assert r.returncode == 0, f"{label} {var}:\n" + r.stdout[-3000:] + r.stderr[-2000:]
