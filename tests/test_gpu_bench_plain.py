"""MI355X: a plain `bench.py --gpus 1` run (no --full) end to end: exit 0, exactly one JSON line with the
headline fields and none of --full's sections, and --dump-outputs writes the last timed solve's x, which
is the syn_arm_cg_n50000 golden's workload (same seeded theta, observations and b): checked against the
reference's step to the parity bound of the suite (1e-4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_prints_headline_and_dumps_x(tmp_path):
    out = tmp_path / "dump"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 7 and d["warmup"] == 2
    assert d["unit"] == "FVP samples/s" and d["dtype"] == "fp32" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 10 * 50_000 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("extra", "roofline", "cpu_baseline", "parity"):
        assert k not in d, k
    assert [p.name for p in out.iterdir()] == ["x.npy"]
    x = np.load(out / "x.npy")
    assert x.dtype == np.float64 and x.shape == (582,)
    assert cases.rel_l2(x, cases.expected(cases.case("syn_arm_cg_n50000"))) <= 1e-4
