"""bench.py as later measurements call it: a plain run prints the line with
`ms_per_step` and none of the --full side measurements, and --dump-outputs
writes the last timed step's accumulators."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(gpu, tmp_path):
    import bench
    from pipsort_amd import engine as E
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PSX_FORCE_DIST"):
        env.pop(k, None)
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", "syn200c2", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["configs_per_step"] / (out["ms_per_step"] / 1e3))
    for k in ("single_pass_ms", "pcie_inclusive", "sss", "configs_file", "example_wall_s", "cpu_baseline",
              "cpu_baseline_example"):
        assert k not in out, k
    # the same locus swept once in this process: the dump is what accum() returns
    pc = E.PostCal(bench.build_inputs("syn200c2"))
    pc.run_exhaustive()
    ref = pc.accum()
    pc.close()
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["n_configs", "no_causal", "notshared_ll", "post", "shared", "shared_ll", "total"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["n_configs"][0] == ref.n_configs == 179_701
    # log-space sums in f64: a different fold order moves the last bits only
    np.testing.assert_allclose(got["total"][0], ref.total, rtol=1e-12)
    for name in ("post", "no_causal", "shared", "shared_ll", "notshared_ll"):
        np.testing.assert_allclose(got[name], getattr(ref, name), rtol=1e-12, atol=1e-12, err_msg=name)
