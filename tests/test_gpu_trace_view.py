"""The seam every trace reduction shares (desman_amd/csrc/dsm_trace_host.h: trace_view): tau's slot 0 is the state the update call entered
with, so stored iteration t lies in slot t + 1 of the tau trace but in row t of the gamma and eta traces; after a fixed-tau update one
tau row serves every iteration.  A view that is off by one for one of the three traces gives a plausible, wrong result.

A real chain of 8 iterations; each entry point over it0 = 3, n_it = 4 on that context, against the same call over the whole trace of
a second context into which exactly iterations 3..6 were planted (tau from get_tau_at, gamma and eta from get_trace).  Both calls do
the same arithmetic on the same operands in the same order -- the launch plans depend on n_it, not on it0 -- and every family's own
test asserts that a repeated call gives the same bits, so the comparison is bit for bit.  The same on a fixed-tau chain (pool = 0).
trace_ppc keys its uniforms by the absolute iteration, so only its observed side is compared.
V = 40, S = 5, G = 3.  Run on an MI355X with:  python -m pytest tests/test_gpu_trace_view.py -m gpu
"""
import numpy as np
import pytest
from numpy.random import RandomState

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
V, S, G, N, IT0, N_IT = 40, 5, 3, 8, 3, 4


def _reductions(c, perm, **rng):
    """every reduction over the range `rng` of c's trace, as {name: array}"""
    out = {"snd": c.trace_snd(_lib.SND_SELF, **rng), "tau_sum_perm": c.get_tau_sum_perm(perm, it0=rng.get("it0", 0))}
    named = {"batch1": c.trace_batch_stats(1, perm=perm, **rng), "batch2": c.trace_batch_stats(2, perm=perm, **rng),
             "fit": c.trace_fit_stats(**rng), "rb": c.trace_rb_marginals(1, perm=perm, **rng),
             "pred": c.trace_predictive(want=("lppd", "mean", "var", "logz_it"), **rng),
             "ppc": c.trace_ppc(3, want=("obs_sample", "obs_position"), **rng)}
    for name, d in named.items():
        for k, v in d.items():
            out[name + "." + k] = np.asarray(v)
    return out


@pytest.mark.parametrize("fixed", [False, True], ids=["gibbs", "fixed_tau"])
def test_a_range_is_the_planted_range(fixed):
    counts, _, _ = synth_counts(V, S, G, seed=41, depth_scale=0.05)      # a few reads per cell: a flat posterior, a chain that keeps moving
    tau, gamma, eta = random_state(V, S, G, seed=42)
    perm = np.array([RandomState(43 + t).permutation(G) for t in range(N_IT)], dtype=np.uint8)
    chain, twin = _lib.Context(0), _lib.Context(0)
    try:
        chain.set_counts(counts); chain.set_state(tau, gamma, eta); chain.seed(5, ctr_seed=99)
        if fixed:
            chain.gibbs_update_fixed_tau(N, pool=0)
        else:
            chain.gibbs_update(N)
        tr = chain.get_trace()
        rows = slice(IT0, IT0 + N_IT)
        digits = np.stack([np.argmax(chain.get_tau_at(t), axis=2) for t in range(IT0, IT0 + N_IT)])
        if fixed:
            assert (digits == np.argmax(tau, axis=2)).all()
        else:                                                   # the slots next to the range hold something else: an off-by-one would show
            assert not np.array_equal(chain.get_tau_at(IT0 - 1), chain.get_tau_at(IT0)) and not np.array_equal(chain.get_tau_at(IT0 + N_IT - 1), chain.get_tau_at(IT0 + N_IT))
        assert not np.array_equal(tr["gamma"][IT0 - 1], tr["gamma"][IT0]) and not np.array_equal(tr["gamma"][IT0 + N_IT - 1], tr["gamma"][IT0 + N_IT])
        assert not np.array_equal(tr["eta"][IT0 - 1], tr["eta"][IT0])
        twin.set_counts(counts); twin.set_state(tau, gamma, eta); twin.seed(5, ctr_seed=99)
        twin.debug_set_trace(digits)
        twin.debug_set_param_trace(tr["gamma"][rows], tr["eta"][rows])
        got = _reductions(chain, perm, it0=IT0, n_it=N_IT)
        want = _reductions(twin, perm)
        assert set(got) == set(want)
        for k in sorted(got):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        assert got["batch1.B"] == 4 and got["batch2.B"] == 2 and got["fit.n_it"] == N_IT and got["pred.n_used"] == N_IT
        assert got["snd"].any() and got["fit.sample"].any() and np.isfinite(got["pred.lppd"]).all() and got["rb.sum"].any()
    finally:
        chain.close()
        twin.close()
