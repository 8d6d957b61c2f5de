"""The two forms of every stand-alone tool on the MI355X: the device form, fed the caller's int64 table chunk by chunk, and the context
form on the resident int32 tensor run the same launches on the same operands, so every output must agree BIT FOR BIT.  Both forms go
through the entry-point scaffolding of desman_amd/csrc/dsm_host_util.h (device and context selection, count staging, buffers); this file
is its check on the GPU, tests/test_tool_errors_cpu.py the one of its argument rules.  One small shape, 5 positions x 3 samples x G = 2,
with the tool's chunk knob at 2: three position chunks with a ragged last one (the abundance tools chunk the 3 samples: 2 + 1).  The
per-tool suites compare the forms too, at their own shapes (test_gpu_assign.py, test_gpu_assign_sampled.py, test_gpu_abund*.py:
"... entry_points"; test_gpu_predictive.py: test_external_counts); here every tool meets the same table.
Run on an MI355X with:  python -m pytest tests/test_gpu_tool_forms.py -m gpu
"""
import numpy as np
import pytest
from numpy.random import RandomState

from desman_amd import _lib

pytestmark = pytest.mark.gpu
V, S, G = 5, 3, 2


def _table():
    rs = RandomState(77)
    counts = rs.randint(0, 30, size=(V, S, 4)).astype(np.int64)
    counts[1, 2] = 0                                    # a cell without reads
    counts[3, :, 1] = 0
    gamma = rs.dirichlet(np.ones(G), size=S)
    eta = np.ascontiguousarray(0.96 * np.eye(4) + 0.01)
    tau = rs.randint(0, 4, size=(V, G)).astype(np.int64)
    return counts, gamma, eta, tau


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    c.set_counts(_table()[0])
    yield c
    c.close()


def _same_bits(a, b, what):
    assert set(a) == set(b) and len(a) > 0, what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def test_exact_assign(ctx):
    counts, gamma, eta, _ = _table()
    try:
        _lib.assign_debug_set_chunk(2)
        _same_bits(_lib.assign_tau(counts, gamma, eta, seed=9), ctx.assign_tau(gamma, eta, seed=9), "assign_tau")
    finally:
        _lib.assign_debug_set_chunk(0)


def test_sampled_assign(ctx):
    counts, gamma, eta, _ = _table()
    kw = dict(seed=9, burn=2, kept=4)
    try:
        _lib.assign_sampled_debug_set_chunk(2)
        _same_bits(_lib.assign_tau_sampled(counts, gamma, eta, **kw), ctx.assign_tau_sampled(gamma, eta, **kw), "assign_tau_sampled")
    finally:
        _lib.assign_sampled_debug_set_chunk(0)


def test_abundance_tools(ctx):
    counts, _, eta, tau = _table()
    kw = dict(max_iter=20, tol=1e-9)
    try:
        _lib.abund_debug_set_chunk(2)
        fit = _lib.fit_gamma(counts, tau, eta, presence=True, **kw)
        _same_bits(fit, ctx.fit_gamma(eta, tau=tau, presence=True, **kw), "fit_gamma")
        _same_bits(_lib.fit_gamma_interval(counts, tau, eta, fit["gamma"], **kw), ctx.fit_gamma_interval(eta, fit["gamma"], tau=tau, **kw),
                   "fit_gamma_interval")
        _same_bits(_lib.fit_gamma_eta(counts, tau, eta, **kw), ctx.fit_gamma_eta(eta, tau=tau, **kw), "fit_gamma_eta")
    finally:
        _lib.abund_debug_set_chunk(0)


def test_predictive_resident_against_given_counts(ctx):
    """the predictive pass has a context form only: the resident tensor against the same table passed as `counts`"""
    counts, _, eta, tau = _table()
    n = 3
    rs = RandomState(5)
    onehot = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(onehot, tau[..., None], 1, axis=2)
    ctx.set_state(onehot, np.full((S, G), 1.0 / G), eta)
    ctx.debug_set_trace(rs.randint(0, 4, size=(n, V, G)))
    ctx.debug_set_param_trace(rs.dirichlet(np.ones(G), size=(n, S)), 0.9 * np.eye(4) + 0.1 * rs.dirichlet(np.ones(4), size=(n, 4)))
    keys = ("lppd", "mean", "var", "logz_it")
    try:
        _lib.pred_debug_set_chunk(2)
        _lib.pred_debug_set_parts(2)
        _same_bits(ctx.trace_predictive(want=keys), ctx.trace_predictive(counts=counts, want=keys), "trace_predictive")
    finally:
        _lib.pred_debug_set_chunk(0)
        _lib.pred_debug_set_parts(0)
