"""bench.py on the GPU: a plain run times --steps steps in one call and prints the headline keys only; --dump-outputs writes
the state its last timed step left -- the same bits from run to run, and the same with --full (the extra measurements come
after the dump and leave the chain's start alone)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from desman_amd.synth import synth_counts
from oracle import cbind

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--V", "2000", "--S", "16", "--G", "4"]


def _bench(extra, out):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra + ["--dump-outputs", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {f[:-4]: np.load(os.path.join(str(out), f)) for f in sorted(os.listdir(str(out)))}


def test_plain_bench_times_its_steps_and_dumps_the_last_one(tmp_path):
    line, a = _bench([], tmp_path / "a")
    assert line["steps"] == 6 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["ms_per_step_repeats"]["n"] == 1 and line["ms_per_step_repeats"]["median"] == line["ms_per_step"]
    assert line["value"] == pytest.approx(2000 * 16 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["unit"] == "V*S updates/s"
    assert not {"roofline", "nmft", "batch", "cpu_baseline"} & set(line)
    # the dumped state is the one the last step's trace entry describes (checked against the oracle's log-likelihood)
    counts, _, _ = synth_counts(2000, 16, 4, seed=1234)
    tau = a["tau"].astype(np.int64)
    assert tau.shape == (2000, 4, 4) and np.all(tau.sum(axis=2) == 1)
    ll = cbind.loglik(cbind.onehot_to_idx(tau), a["gamma"], a["eta"], counts)
    assert abs(a["ll"][0] - ll) <= 1e-12 * abs(ll)
    assert len(a["trace_ll"]) == 6 and a["trace_ll"][-1] == a["ll"][0]
    assert a["lp_star"][0] == line["fit_records"][0]["lp_star"]
    _, b = _bench([], tmp_path / "b")
    line_c, c = _bench(["--full", "--repeats", "1", "--no-cpu-baseline", "--no-pmc", "--batch", "0"], tmp_path / "c")
    assert "roofline" in line_c and line_c["nmft"]["iters"] == 200
    for other in (b, c):
        assert sorted(other) == sorted(a)
        for k in a:
            assert np.array_equal(other[k], a[k]), k
