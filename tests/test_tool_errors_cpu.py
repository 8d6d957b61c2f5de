"""The argument checks of the stand-alone tools' device forms (dsm_assign_tau, dsm_assign_tau_sampled_pairs, dsm_fit_gamma,
dsm_fit_gamma_interval, dsm_fit_gamma_eta) and of the debug knobs: return code and the full text of dsm_last_error() for one fault per
call.  Every call fails before the device is touched, so no GPU is needed.  The expected texts were recorded from the library as it was
before the checks moved into desman_amd/csrc/dsm_host_util.h: that header may not change a word of them."""
import numpy as np
import pytest

from desman_amd import _lib

OK, ERR_ARG, ERR_NODEVICE = 0, -2, -6
N, S, G = 2, 3, 2
TOOLS = ("assign", "sampled", "fit", "interval", "fit_eta")


def _inputs():
    counts = np.arange(1, N * S * 4 + 1, dtype=np.int64).reshape(N, S, 4)
    gamma = np.array([[0.7, 0.3], [0.5, 0.5], [0.2, 0.8]])
    eta = np.ascontiguousarray(0.96 * np.eye(4) + 0.01)
    tau = np.array([[0, 1], [2, 3]], dtype=np.int64)
    return dict(counts=counts, gamma=gamma, eta=eta, tau=tau, device=0)


def _fault(kw, name):
    if name == "negative count":
        kw["counts"][1, 2, 0] = -1
    elif name == "cell of 2^31":
        kw["counts"][1, 2, 3] = 2 ** 31
    elif name == "depth of 2^31":
        kw["counts"][1, 2] = (2 ** 30, 2 ** 30, 0, 0)
    elif name == "negative eta":
        kw["eta"].flat[5] = -0.1
    elif name == "nan eta":
        kw["eta"].flat[5] = np.nan
    elif name == "inf gamma":
        kw["gamma"].flat[4] = np.inf
    elif name == "tau digit 4":
        kw["tau"][1, 0] = 4
    elif name == "device -1":
        kw["device"] = -1
    else:
        raise KeyError(name)


def _call(tool, counts, gamma, eta, tau, device):
    """The raw entry point of `tool`; outputs are real buffers although no call here gets as far as writing one."""
    lib = _lib.load()
    f64 = lambda *shape: np.zeros(shape)
    i32 = lambda *shape: np.zeros(shape, dtype=np.int32)
    u8 = lambda *shape: np.zeros(shape, dtype=np.uint8)
    p = _lib._ptr
    if tool == "assign":
        out = [u8(N, G), f64(N), f64(N), f64(N, G, 4), u8(N, G)]
        return lib.dsm_assign_tau(device, counts, N, S, G, gamma, eta, 1, *[p(a) for a in out])
    if tool == "sampled":
        out = [u8(N, G), f64(N), f64(N), f64(N, G, 4), f64(N), u8(N, G)]
        return lib.dsm_assign_tau_sampled_pairs(device, counts, N, S, G, gamma, eta, 1, 2, 4, 0, *[p(a) for a in out])
    if tool == "fit":
        out = [f64(S, G), f64(S), f64(S), i32(S), i32(S), f64(S, G)]
        return lib.dsm_fit_gamma(device, counts, N, S, G, tau, eta, 10, 1e-9, 0, *[p(a) for a in out])
    if tool == "interval":
        out = [f64(S, G), f64(S, G), i32(S, G)]
        return lib.dsm_fit_gamma_interval(device, counts, N, S, G, tau, eta, gamma, 3.84, 10, 1e-9, 1e-6, *[p(a) for a in out])
    if tool == "fit_eta":
        out = [f64(S, G), f64(4, 4), f64(S), f64(S), f64(S), i32(1), i32(1), i32(1), f64(1)]
        return lib.dsm_fit_gamma_eta(device, counts, N, S, G, tau, eta, 10, 1e-9, *[p(a) for a in out])
    raise KeyError(tool)


# (tool, fault) -> (return code, dsm_last_error()).  The assign tools take no tau; the joint fit takes no gamma; the interval's gamma is
# gamma_hat, which has a rule of its own.
EXPECT = {
    ('assign', 'negative count'): (ERR_ARG, 'assign_tau: count -1 at position 1, sample 2'),
    ('assign', 'cell of 2^31'): (ERR_ARG, 'assign_tau: count 2147483648 at position 1, sample 2'),
    ('assign', 'depth of 2^31'): (ERR_ARG, 'assign_tau: depth above 2^31-1 at position 1, sample 2'),
    ('assign', 'negative eta'): (ERR_ARG, 'assign: eta[5] is negative or not finite'),
    ('assign', 'nan eta'): (ERR_ARG, 'assign: eta[5] is negative or not finite'),
    ('assign', 'inf gamma'): (ERR_ARG, 'assign: gamma[4] is negative or not finite'),
    ('assign', 'device -1'): (ERR_NODEVICE, 'no HIP device visible'),
    ('sampled', 'negative count'): (ERR_ARG, 'assign_tau_sampled: count -1 at position 1, sample 2'),
    ('sampled', 'cell of 2^31'): (ERR_ARG, 'assign_tau_sampled: count 2147483648 at position 1, sample 2'),
    ('sampled', 'depth of 2^31'): (ERR_ARG, 'assign_tau_sampled: depth above 2^31-1 at position 1, sample 2'),
    ('sampled', 'negative eta'): (ERR_ARG, 'assign_sampled: eta[5] is negative or not finite'),
    ('sampled', 'nan eta'): (ERR_ARG, 'assign_sampled: eta[5] is negative or not finite'),
    ('sampled', 'inf gamma'): (ERR_ARG, 'assign_sampled: gamma[4] is negative or not finite'),
    ('sampled', 'device -1'): (ERR_NODEVICE, 'no HIP device visible'),
    ('fit', 'negative count'): (ERR_ARG, 'fit_gamma: count -1 at position 1, sample 2'),
    ('fit', 'cell of 2^31'): (ERR_ARG, 'fit_gamma: count 2147483648 at position 1, sample 2'),
    ('fit', 'depth of 2^31'): (ERR_ARG, 'fit_gamma: depth above 2^31-1 at position 1, sample 2'),
    ('fit', 'negative eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('fit', 'nan eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('fit', 'tau digit 4'): (ERR_ARG, 'fit_gamma: tau[1][0] = 4 is not a base 0..3'),
    ('fit', 'device -1'): (ERR_NODEVICE, 'no HIP device visible'),
    ('interval', 'negative count'): (ERR_ARG, 'fit_gamma: count -1 at position 1, sample 2'),
    ('interval', 'cell of 2^31'): (ERR_ARG, 'fit_gamma: count 2147483648 at position 1, sample 2'),
    ('interval', 'depth of 2^31'): (ERR_ARG, 'fit_gamma: depth above 2^31-1 at position 1, sample 2'),
    ('interval', 'negative eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('interval', 'nan eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('interval', 'inf gamma'): (ERR_ARG, 'fit_gamma_interval: gamma_hat[2][0] = inf is outside [0, 1]'),
    ('interval', 'tau digit 4'): (ERR_ARG, 'fit_gamma: tau[1][0] = 4 is not a base 0..3'),
    ('interval', 'device -1'): (ERR_NODEVICE, 'no HIP device visible'),
    ('fit_eta', 'negative count'): (ERR_ARG, 'fit_gamma: count -1 at position 1, sample 2'),
    ('fit_eta', 'cell of 2^31'): (ERR_ARG, 'fit_gamma: count 2147483648 at position 1, sample 2'),
    ('fit_eta', 'depth of 2^31'): (ERR_ARG, 'fit_gamma: depth above 2^31-1 at position 1, sample 2'),
    ('fit_eta', 'negative eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('fit_eta', 'nan eta'): (ERR_ARG, 'fit_gamma: eta[5] is negative or not finite'),
    ('fit_eta', 'tau digit 4'): (ERR_ARG, 'fit_gamma: tau[1][0] = 4 is not a base 0..3'),
    ('fit_eta', 'device -1'): (ERR_NODEVICE, 'no HIP device visible'),
}

SETTERS = {
    'dsm_abund_debug_set_chunk': 'abund: chunk -1',
    'dsm_abund_debug_set_eta_batch': 'abund: eta batch -1',
    'dsm_assign_debug_set_chunk': 'assign: chunk -1',
    'dsm_assign_sampled_debug_set_chunk': 'assign_sampled: chunk -1',
    'dsm_diag_debug_set_parts': 'diag: parts -1',
    'dsm_fit_debug_set_parts': 'fit: parts -1',
    'dsm_pred_debug_set_chunk': 'pred: chunk -1',
    'dsm_pred_debug_set_parts': 'pred: parts -1',
}


def _run(tool, fault):
    kw = _inputs()
    _fault(kw, fault)
    rc = _call(tool, **kw)
    return rc, _lib.load().dsm_last_error().decode()


@pytest.mark.parametrize("tool,fault", [k for k in EXPECT if k[1] != "device -1"], ids=lambda v: v.replace(" ", "_"))
def test_argument_fault(tool, fault):
    assert _run(tool, fault) == EXPECT[(tool, fault)]


@pytest.mark.parametrize("tool", TOOLS)
def test_no_device(tool):
    if _lib.load().dsm_device_count() > 0:
        pytest.skip("a GPU is visible: device -1 is then out of range, not missing")
    assert _run(tool, "device -1") == EXPECT[(tool, "device -1")]


def test_fault_table_is_complete():
    faults = {"negative count", "cell of 2^31", "depth of 2^31", "negative eta", "nan eta", "device -1"}
    for tool in TOOLS:
        want = set(faults) | ({"tau digit 4"} if tool in ("fit", "interval", "fit_eta") else set())
        want |= {"inf gamma"} if tool in ("assign", "sampled", "interval") else set()
        assert {f for (t, f) in EXPECT if t == tool} == want, tool


@pytest.mark.parametrize("name", sorted(SETTERS))
def test_debug_setter(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    try:
        assert fn(-1) == ERR_ARG and lib.dsm_last_error().decode() == SETTERS[name]
    finally:
        assert fn(0) == OK


# ---- the entry points that read the resident traces (desman_amd/csrc/api_trace.hip, kernels_pred.hip): a null context is refused by the
# check they share before anything else is looked at, so the other arguments may be anything
TRACE_CALLS = {
    "dsm_ctx_trace_snd": (1, None, 0, 0, 1, None),
    "dsm_ctx_get_tau_sum_perm": (None, 0, 1, None),
    "dsm_ctx_trace_batch_stats": (None, 0, 1, 0, None, None, None, None),
    "dsm_ctx_trace_fit_stats": (0, 1, None, None, None),
    "dsm_ctx_trace_rb_marginals": (None, 0, 1, 0, None, None, None),
    "dsm_ctx_trace_ppc": (0, 1, 0, 0, 0, None, None, None, None, None, None),
    "dsm_ctx_trace_predictive": (None, -1, 0, 1, 0, None, None, None, None),
    "dsm_ctx_debug_set_trace": (None, -1),
    "dsm_ctx_debug_set_param_trace": (None, None, -1),
}


@pytest.mark.parametrize("name", sorted(TRACE_CALLS))
def test_trace_entry_point_without_a_context(name):
    lib = _lib.load()
    assert getattr(lib, name)(None, *TRACE_CALLS[name]) == ERR_ARG and lib.dsm_last_error().decode() == "null context"
