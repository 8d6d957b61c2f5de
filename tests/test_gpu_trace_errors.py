"""The argument checks of the seven entry points that read the chain's resident traces (dsm_ctx_trace_snd, dsm_ctx_get_tau_sum_perm,
dsm_ctx_trace_batch_stats, dsm_ctx_trace_fit_stats, dsm_ctx_trace_rb_marginals, dsm_ctx_trace_ppc, dsm_ctx_trace_predictive) and of
the hooks that plant a trace: return code and the full text of dsm_last_error() for one fault per check, through the raw C calls (the
Python wrappers have checks of their own in front of some).  The expected texts were recorded from the library as it was before the
checks moved into desman_amd/csrc/dsm_trace_host.h and the entry points into api_trace.hip: that move may not change a word of them,
nor which of two coinciding faults is reported.  After every fault the context answers the entry point's valid call with the bits it
gave before any fault.
V = 30, S = 4, G = 3 with a planted trace of 6 iterations; a second context with G = 11 for the limit of trace_predictive.
Run on an MI355X with:  python -m pytest tests/test_gpu_trace_errors.py -m gpu
"""
import ctypes as C

import numpy as np
import pytest
from numpy.random import RandomState

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -2, -3, -4
V, S, G, N_IT = 30, 4, 3, 6
ENTRIES = ("trace_snd", "get_tau_sum_perm", "trace_batch_stats", "trace_fit_stats", "trace_rb_marginals", "trace_ppc", "trace_predictive")


def _context(G_, plant):
    c = _lib.Context(0)
    counts, _, _ = synth_counts(V, S, G_, seed=31)
    tau, gamma, eta = random_state(V, S, G_, seed=32)
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    if plant:
        rs = RandomState(33)
        c.debug_set_trace(rs.randint(0, 4, size=(N_IT, V, G_)))
        c.debug_set_param_trace(rs.dirichlet(np.ones(G_), size=(N_IT, S)), np.tile(0.96 * np.eye(4) + 0.01, (N_IT, 1, 1)))
    return c


def _identity(n, G_=G):
    return np.tile(np.arange(G_, dtype=np.uint8), (n, 1))


def _call(c, entry, **kw):
    """the raw entry point with a valid call's arguments except those given; returns (rc, dsm_last_error(), outputs as bytes)"""
    G_ = c.G or G
    a = dict(it0=0, n_it=N_IT, mode=_lib.SND_SELF, ref=None, Gr=0, perm=None, batch_len=1, stride=1, R=2, counts=None, N=0, out=True)
    a.update(kw)
    rows = max(a["n_it"], 0)
    p = lambda x: None if x is None or not a["out"] else x.ctypes.data
    inp = lambda x: None if x is None else x.ctypes.data
    vg4 = (V, G_, 4)
    if entry == "trace_snd":
        outs = [np.zeros((rows, G_, max(a["Gr"], G_)), dtype=np.int32)]
        rc = c.lib.dsm_ctx_trace_snd(c._h, a["mode"], inp(a["ref"]), a["Gr"], a["it0"], a["n_it"], p(outs[0]))
    elif entry == "get_tau_sum_perm":
        perm = _identity(rows, G_) if a["perm"] is None else a["perm"]
        outs = [np.zeros(vg4, dtype=np.int64)]
        rc = c.lib.dsm_ctx_get_tau_sum_perm(c._h, inp(perm) if a.get("with_perm", True) else None, a["it0"], a["n_it"], p(outs[0]))
    elif entry == "trace_batch_stats":
        outs = [np.zeros(vg4, dtype=np.int64) for _ in range(3)] + [np.zeros((V, G_), dtype=np.int32)]
        rc = c.lib.dsm_ctx_trace_batch_stats(c._h, inp(a["perm"]), a["it0"], a["n_it"], a["batch_len"], *[p(o) for o in outs])
    elif entry == "trace_fit_stats":
        outs = [np.zeros((S, 4)), np.zeros((V, 4)), np.zeros((V, S))]
        rc = c.lib.dsm_ctx_trace_fit_stats(c._h, a["it0"], a["n_it"], *[p(o) for o in outs])
    elif entry == "trace_rb_marginals":
        outs = [np.zeros(vg4), np.zeros(vg4)]
        dead = C.c_longlong(-1)
        rc = c.lib.dsm_ctx_trace_rb_marginals(c._h, inp(a["perm"]), a["it0"], a["n_it"], a["batch_len"], *[p(o) for o in outs], C.byref(dead))
        outs.append(np.array([dead.value]))
    elif entry == "trace_ppc":
        outs = [np.zeros(S, dtype=np.int64), np.zeros(V, dtype=np.int64), np.zeros((S, 2)), np.zeros((V, 2)), np.zeros(S), np.zeros(V)]
        rc = c.lib.dsm_ctx_trace_ppc(c._h, a["it0"], a["n_it"], a["stride"], a["R"], C.c_uint64(5), *[p(o) for o in outs])
    elif entry == "trace_predictive":
        n_pos = V if a["counts"] is None else a["N"]
        outs = [np.zeros(max(n_pos, 0)) for _ in range(3)]
        rc = c.lib.dsm_ctx_trace_predictive(c._h, inp(a["counts"]), a["N"], a["it0"], a["n_it"], a["stride"], *[p(o) for o in outs], None)
    else:
        raise KeyError(entry)
    return rc, c.lib.dsm_last_error().decode(), [o.tobytes() for o in outs]


@pytest.fixture(scope="module")
def planted():
    c = _context(G, plant=True)
    good = {}
    for e in ENTRIES:
        rc, _, outs = _call(c, e)
        assert rc == OK, (e, c.lib.dsm_last_error())
        good[e] = outs
    assert all(any(np.frombuffer(o, dtype=np.uint8).any() for o in outs) for outs in good.values())     # the valid calls write something
    yield c, good
    c.close()


@pytest.fixture(scope="module")
def bare():
    c = _context(G, plant=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide():
    c = _context(11, plant=True)
    yield c
    c.close()


def _bad_perm(n, row):
    perm = _identity(n)
    perm[row] = (0, 0, 2)
    return perm


def _bad_counts(cell):
    x = np.full((2, S, 4), 3, dtype=np.int64)
    x[1, 2, 0] = cell
    return x


RANGE = "%s: iterations %d .. %d + %d outside the trace of 6"
PERM = "%s: row %d of perm is not a permutation of 0..2"
# (entry, fault) -> (arguments that differ from the valid call, return code, dsm_last_error())
FAULTS = {}
for _e in ENTRIES:
    FAULTS[(_e, "it0 < 0")] = (dict(it0=-1), ERR_ARG, RANGE % (_e, -1, -1, 6))
    FAULTS[(_e, "range past the trace")] = (dict(it0=4, n_it=3), ERR_ARG, RANGE % (_e, 4, 4, 3))
    FAULTS[(_e, "it0 past the trace")] = (dict(it0=7, n_it=0), ERR_ARG, RANGE % (_e, 7, 7, 0))
    FAULTS[(_e, "n_it < 0")] = (dict(n_it=-1), ERR_ARG, RANGE % (_e, 0, 0, -1))
for _e in ("trace_batch_stats", "trace_rb_marginals"):
    FAULTS[(_e, "batch_len < 1")] = (dict(batch_len=0), ERR_ARG, "%s: batch_len=0, at least 1 is needed" % _e)
    FAULTS[(_e, "fewer than two batches")] = (dict(batch_len=4), ERR_ARG, "%s: 6 iterations are fewer than two batches of 4" % _e)
    # n_it = 5 in batches of 2: B = 2, the first iteration is skipped -- and its row of perm is checked all the same
    FAULTS[(_e, "perm, a used row")] = (dict(n_it=5, batch_len=2, perm=_bad_perm(5, 3)), ERR_ARG, PERM % (_e, 3))
    FAULTS[(_e, "perm, a skipped row")] = (dict(n_it=5, batch_len=2, perm=_bad_perm(5, 0)), ERR_ARG, PERM % (_e, 0))
    FAULTS[(_e, "range and batch_len")] = (dict(it0=-1, batch_len=0), ERR_ARG, RANGE % (_e, -1, -1, 6))
    FAULTS[(_e, "batch_len and perm")] = (dict(batch_len=0, perm=_bad_perm(6, 1)), ERR_ARG, "%s: batch_len=0, at least 1 is needed" % _e)
    FAULTS[(_e, "batches and perm")] = (dict(batch_len=4, perm=_bad_perm(6, 1)), ERR_ARG, "%s: 6 iterations are fewer than two batches of 4" % _e)
FAULTS.update({
    ("get_tau_sum_perm", "perm, a used row"): (dict(perm=_bad_perm(6, 4)), ERR_ARG, PERM % ("get_tau_sum_perm", 4)),
    ("get_tau_sum_perm", "perm, a label of G"): (dict(perm=_identity(6) + np.uint8(1)), ERR_ARG, PERM % ("get_tau_sum_perm", 0)),
    ("get_tau_sum_perm", "no output"): (dict(out=False), ERR_ARG, "get_tau_sum_perm: null pointer"),
    ("get_tau_sum_perm", "no perm"): (dict(with_perm=False), ERR_ARG, "get_tau_sum_perm: null pointer"),
    ("get_tau_sum_perm", "range and no output"): (dict(it0=-1, out=False), ERR_ARG, RANGE % ("get_tau_sum_perm", -1, -1, 6)),
    ("trace_snd", "mode"): (dict(mode=7), ERR_ARG, "trace_snd: mode 7 is none of DSM_SND_STAR / SELF / GIVEN"),
    ("trace_snd", "Gr = 0 given"): (dict(mode=_lib.SND_GIVEN, Gr=0, ref=np.zeros((V, 3), dtype=np.int64)), ERR_ARG, "trace_snd: Gr=0 outside 1..32"),
    ("trace_snd", "Gr = 33 given"): (dict(mode=_lib.SND_GIVEN, Gr=33, ref=np.zeros((V, 33), dtype=np.int64)), ERR_ARG, "trace_snd: Gr=33 outside 1..32"),
    ("trace_snd", "Gr of another mode"): (dict(mode=_lib.SND_STAR, Gr=2), ERR_ARG,
                                         "trace_snd: Gr=2, but this mode's reference has the chain's 3 haplotypes (pass 0 or G)"),
    ("trace_snd", "no reference"): (dict(mode=_lib.SND_GIVEN, Gr=3), ERR_ARG, "trace_snd: DSM_SND_GIVEN without a reference"),
    ("trace_snd", "reference digit"): (dict(mode=_lib.SND_GIVEN, Gr=2, ref=np.array([[0, 1]] * 7 + [[2, 5]] + [[3, 0]] * (V - 8), dtype=np.int64)),
                                      ERR_ARG, "trace_snd: digit 5 at row 7, haplotype 1 is not a base 0..3"),
    ("trace_snd", "no output"): (dict(out=False), ERR_ARG, "trace_snd: no output buffer"),
    ("trace_snd", "range and mode"): (dict(n_it=7, mode=7), ERR_ARG, RANGE % ("trace_snd", 0, 0, 7)),
    ("trace_snd", "mode and no output"): (dict(mode=7, out=False), ERR_ARG, "trace_snd: mode 7 is none of DSM_SND_STAR / SELF / GIVEN"),
    ("trace_ppc", "stride < 1"): (dict(stride=0), ERR_ARG, "trace_ppc: stride=0, R=2: at least 1 is needed"),
    ("trace_ppc", "R < 1"): (dict(R=0), ERR_ARG, "trace_ppc: stride=1, R=0: at least 1 is needed"),
    ("trace_ppc", "R above the limit"): (dict(R=1025), ERR_UNSUPPORTED, "trace_ppc: R=1025 above DSM_PPC_MAX_R=1024"),
    ("trace_ppc", "range and stride"): (dict(it0=4, n_it=3, stride=0), ERR_ARG, RANGE % ("trace_ppc", 4, 4, 3)),
    ("trace_ppc", "stride and R"): (dict(stride=-1, R=1025), ERR_ARG, "trace_ppc: stride=-1, R=1025: at least 1 is needed"),
    ("trace_predictive", "stride < 1"): (dict(stride=0), ERR_ARG, "trace_predictive: stride 0"),
    ("trace_predictive", "N < 0"): (dict(counts=_bad_counts(3), N=-1), ERR_ARG, "trace_predictive: N=-1"),
    ("trace_predictive", "negative count"): (dict(counts=_bad_counts(-1), N=2), ERR_ARG, "trace_predictive: count -1 at position 1, sample 2"),
    ("trace_predictive", "range and stride"): (dict(n_it=-1, stride=0), ERR_ARG, RANGE % ("trace_predictive", 0, 0, -1)),
    ("trace_predictive", "stride and counts"): (dict(stride=0, counts=_bad_counts(-1), N=2), ERR_ARG, "trace_predictive: stride 0"),
})


@pytest.mark.parametrize("entry,fault", sorted(FAULTS), ids=lambda v: v.replace(" ", "_"))
def test_fault(planted, entry, fault):
    c, good = planted
    kw, rc, text = FAULTS[(entry, fault)]
    assert _call(c, entry, **kw)[:2] == (rc, text)
    again = _call(c, entry)
    assert again[0] == OK and again[2] == good[entry]


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_update_has_run(bare, planted, entry):
    assert _call(bare, entry)[:2] == (ERR_STATE, "%s: no update has run" % entry)
    assert _call(bare, entry, it0=-1, n_it=-1, batch_len=0, stride=0, R=0, mode=7)[:2] == (ERR_STATE, "%s: no update has run" % entry)
    c, good = planted                                          # the message is per thread, not per context: another context is not disturbed
    again = _call(c, entry)
    assert again[0] == OK and again[2] == good[entry]


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_counts_no_state(entry):
    c = _lib.Context(0)
    try:
        assert _call(c, entry)[:2] == (ERR_STATE, "no count tensor: call dsm_ctx_set_counts first")
        c.set_counts(synth_counts(V, S, G, seed=31)[0])
        assert _call(c, entry)[:2] == (ERR_STATE, "no chain state: call dsm_ctx_set_state first")
    finally:
        c.close()


def test_predictive_limit_of_G(wide):
    text = "trace_predictive: G=11 exceeds DSM_ASSIGN_MAX_G=10 (all 4^G joint states are evaluated)"
    assert _call(wide, "trace_predictive")[:2] == (ERR_UNSUPPORTED, text)
    assert _call(wide, "trace_predictive", stride=0)[:2] == (ERR_ARG, "trace_predictive: stride 0")                 # looked at before G
    assert _call(wide, "trace_predictive", counts=_bad_counts(-1), N=2)[:2] == (ERR_UNSUPPORTED, text)             # ... and G before the counts
    assert _call(wide, "trace_predictive", it0=7, n_it=0)[:2] == (ERR_ARG, RANGE % ("trace_predictive", 7, 7, 0))
    rc, _, outs = _call(wide, "trace_fit_stats")               # the context goes on serving what has no such limit
    assert rc == OK and np.frombuffer(outs[0]).any()
    assert np.array_equal(wide.trace_snd(_lib.SND_SELF)[:, np.arange(11), np.arange(11)], np.zeros((N_IT, 11), dtype=np.int32))


def test_planting_hooks(planted):
    c, good = planted
    lib = c.lib
    digits = RandomState(34).randint(0, 4, size=(2, V, G)).astype(np.int64)
    digits[1, 2, 1] = 4
    cases = [(lambda: lib.dsm_ctx_debug_set_trace(c._h, digits.ctypes.data, 2), "debug_set_trace: digit 4 at row 32, haplotype 1 is not a base 0..3"),
             (lambda: lib.dsm_ctx_debug_set_trace(c._h, digits.ctypes.data, -1), "debug_set_trace: bad arguments"),
             (lambda: lib.dsm_ctx_debug_set_trace(c._h, None, 2), "debug_set_trace: bad arguments"),
             (lambda: lib.dsm_ctx_debug_set_param_trace(c._h, None, None, 7), "debug_set_param_trace: n=7 outside the trace of 6, or a null pointer"),
             (lambda: lib.dsm_ctx_debug_set_param_trace(c._h, None, None, -1), "debug_set_param_trace: n=-1 outside the trace of 6, or a null pointer"),
             (lambda: lib.dsm_ctx_debug_set_param_trace(c._h, None, digits.ctypes.data, 1),
              "debug_set_param_trace: n=1 outside the trace of 6, or a null pointer")]
    for call, text in cases:
        assert (call(), lib.dsm_last_error().decode()) == (ERR_ARG, text)
        for e in ENTRIES:                                      # a refused hook leaves the trace as it was
            again = _call(c, e)
            assert again[0] == OK and again[2] == good[e], (text, e)


def test_planting_hooks_before_a_trace(bare):
    lib = bare.lib
    one = np.zeros((S, G))
    assert lib.dsm_ctx_debug_set_param_trace(bare._h, one.ctypes.data, one.ctypes.data, 1) == ERR_ARG
    assert lib.dsm_last_error().decode() == "debug_set_param_trace: n=1 outside the trace of 0, or a null pointer"
    assert lib.dsm_ctx_debug_set_param_trace(bare._h, None, None, 0) == OK
    assert _call(bare, "trace_fit_stats")[:2] == (ERR_STATE, "trace_fit_stats: no update has run")


def test_nothing_to_do_touches_no_output(planted):
    """n_it = 0 inside the trace succeeds; the entry points that report sums zero what was asked for, the others write nothing"""
    c, good = planted
    for e in ENTRIES:
        for it0 in (0, 3, N_IT):
            rc, _, outs = _call(c, e, it0=it0, n_it=0)
            assert rc == OK, (e, it0, c.lib.dsm_last_error())
            assert not any(np.frombuffer(o, dtype=np.uint8).any() for o in outs if len(o)), (e, it0)
        assert _call(c, e, it0=2, n_it=0, out=False)[0] == (ERR_ARG if e == "get_tau_sum_perm" else OK)      # no output asked for: none fetched
