"""bench.py without a GPU: what --dump-outputs writes (from a stand-in context) and the options a plain run refuses."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Ctx:
    """the two calls dump_outputs makes of a chain context"""

    def __init__(self, V, S, G, seed):
        rng = np.random.default_rng(seed)
        self.tau = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(self.tau, rng.integers(0, 4, size=(V, G))[..., None], 1, axis=2)
        self.gamma = rng.dirichlet(np.ones(G), size=S)
        self.eta = rng.dirichlet(np.ones(4), size=4)

    def get_state(self):
        return self.tau.copy(), self.gamma.copy(), self.eta.copy()


def _dump(path, V=500, S=6, G=3, steps=5):
    ctx = _Ctx(V, S, G, seed=1)
    rng = np.random.default_rng(2)
    tr = dict(ll=rng.normal(size=steps), lp=rng.normal(size=steps), nchange=rng.integers(0, 9, size=steps).astype(np.int32))
    star = dict(tau=np.roll(ctx.tau, 1, axis=0), gamma=ctx.gamma[::-1].copy(), eta=ctx.eta.T.copy(), lp=-12.5, it=3)
    fits = [[float(G), float(G), 0.0, -12.5, 31.0, float(steps)]]
    bench.dump_outputs(str(path), ctx, tr, star, fits)
    return ctx, tr, star, {f[:-4]: np.load(os.path.join(str(path), f)) for f in sorted(os.listdir(str(path)))}


def test_dump_outputs_writes_the_last_step(tmp_path):
    ctx, tr, star, got = _dump(tmp_path)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert "positions" not in got
    assert np.array_equal(got["tau"], ctx.tau) and got["tau"].dtype == np.float32
    assert np.array_equal(got["gamma"], ctx.gamma) and np.array_equal(got["eta"], ctx.eta)
    assert got["ll"].tolist() == tr["ll"][-1:].tolist() and got["lp"].tolist() == tr["lp"][-1:].tolist()
    assert got["nchange"].tolist() == [float(tr["nchange"][-1])]
    assert np.array_equal(got["trace_ll"], tr["ll"]) and np.array_equal(got["trace_lp"], tr["lp"])
    assert np.array_equal(got["tau_star"], star["tau"]) and got["lp_star"].tolist() == [star["lp"]] and got["it_star"].tolist() == [3.0]
    assert got["fit_records"].shape == (1, 6)


def test_dump_outputs_samples_positions_over_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 100000)
    V = 2000
    ctx, _, star, got = _dump(tmp_path / "a", V=V)
    assert sum(a.nbytes for a in got.values()) <= 100000
    rows = got["positions"].astype(np.int64)
    assert 0 < len(rows) < V and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["tau"], ctx.tau[rows]) and np.array_equal(got["tau_star"], star["tau"][rows])
    assert np.array_equal(got["gamma"], ctx.gamma)                     # only the [V, ...] tables are sampled
    _, _, _, again = _dump(tmp_path / "b", V=V)
    assert np.array_equal(again["positions"], got["positions"])        # a fixed sample: two builds compare position for position


def test_plain_run_refuses_what_belongs_to_full():
    for extra in (["--pmc"], ["--pmc-save"], ["--workload", "genes", "--dump-outputs", "x"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "error" in r.stderr and not r.stdout, (extra, r.stderr[-500:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
