"""The device tau sweeps against the reference's OWN compiled sweep (sampletau/c_sample_tau.c, unmodified, in oracle/_ref --
tests/_ref_sweep.py), exactly: tau element by element and nchange, every sweep, no tolerance.  The other GPU suites compare with the
oracle's restatement of that file; tests/test_ref_sweep_cpu.py pins the restatement, this file pins the kernels themselves: the context
sweep at the first and last sample count of every tiling, the Gibbs loop's instantiations, the legacy shim with the reference's call
sequence, and the other `(double)(float)` sites (held sweep, gene sampler).  Needs oracle/_ref only, not the reference tree."""
import numpy as np
import pytest

import _ref_sweep as R
from desman_amd import _lib
from oracle import cbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return R.reference()


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _load(ctx, counts, tau, pi, eta, seed):
    ctx.set_counts(counts)
    ctx.set_state(tau, pi, eta)
    ctx.seed(seed)
    ctx.set_tau_rng(_lib.RNG_MT19937)


def ctx_sweeps(ctx, counts, tau, pi, eta, seed, sweep=None, n=R.N_SWEEPS):
    """n consecutive single sweeps of the context (dsm_ctx_sample_tau, or sweep(ctx)) on one MT19937 stream"""
    _load(ctx, counts, tau, pi, eta, seed)
    out = []
    for _ in range(n):
        nch = ctx.sample_tau() if sweep is None else sweep(ctx)
        out.append((ctx.get_state()[0], nch))
    return out


def shim_sweeps(tau, pi, eta, counts, seed, n=R.N_SWEEPS):
    """the legacy four-call interface, called as tests/_ref_sweep.py: ref_sweeps calls the reference"""
    from desman_amd import sampletau
    sampletau.initRNG()
    if seed is not None:
        sampletau.setRNG(seed)
    t = tau.copy()
    out = []
    with np.errstate(all="ignore"):
        for _ in range(n):
            nch = sampletau.sample_tau(t, pi, eta, counts)
            out.append((t.copy(), nch))
    sampletau.freeRNG()
    return out


# ------------------------------------------------------------------------------------------------------------------- context sweep
@pytest.mark.parametrize("S,G", [(S, 4) for S in (1, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 193, 257, 385, 512)] +
                         [(24, G) for G in (1, 9, 17, 32)])
def test_context_sweep_is_the_reference_sweep(ctx, ref, S, G):
    """dsm_ctx_sample_tau in MT19937 mode, V = 20, three sweeps on one stream, screen on and off -- on a shallow table from a random start
    (flat conditionals: every uniform decides) and on a deep one from the generating state (sharp conditionals: what the screen is for)"""
    V = 20
    for start in ("random", "generating"):
        counts, tau, pi, eta = R.state(V, S, G, start, seed=2000 * S + 10 * G)
        seed = 11 * S + G
        want = R.ref_sweeps(ref, tau, pi, eta, counts, seed)
        for screen in (True, False):
            ctx.set_tau_screen(screen)
            try:
                got = ctx_sweeps(ctx, counts, tau, pi, eta, seed)
            finally:
                ctx.set_tau_screen(True)
            R.assert_same(got, want, "%s start, screen %s:" % (start, "on" if screen else "off"))


# ------------------------------------------------------------------------------------------------------------------- Gibbs loop
@pytest.mark.parametrize("V,S,G", [(150, 64, 8), (150, 96, 12)])
@pytest.mark.parametrize("neartie", [0, 1], ids=["plain", "near-tie"])
def test_gibbs_loop_sweeps_are_the_reference_sweeps(ctx, ref, V, S, G, neartie):
    """The Gibbs loop's instantiation of the sweep, plain and with the near-tie screen forced (dsm_ctx_set_tau_neartie), on a state with two
    haplotypes rare in every sample: the sweep of iteration it of gibbs_update is c_sample_tau on (tau_{it-1}, gamma_it, eta_{it-1}), and
    the sweeps of update_tau -- the same instantiation, as the Gibbs call left it -- are c_sample_tau on the stored (gamma, eta)."""
    counts, tau, pi, eta = R.state(V, S, G, "random", seed=V + S + G, shallow=False)
    rng = np.random.default_rng(G)
    pi = pi.copy()
    pi[:, [1, G - 1]] = rng.uniform(2.0e-4, 2.0e-3, size=(S, 2))
    pi = np.ascontiguousarray(pi / pi.sum(axis=1, keepdims=True))
    n_it = 3
    ctx.set_tau_neartie(neartie)
    try:
        _load(ctx, counts, tau, pi, eta, 4711)
        ctx.seed(4711, ctr_seed=0xFEEDFACE)
        ctx.gibbs_update(n_it)
        tr = ctx.get_trace()
        taus = [ctx.get_tau_at(i) for i in range(n_it)]
        ref.c_initRNG(); ref.c_setRNG(4711)
        t, eta_prev = tau.copy(), eta
        for it in range(n_it):
            n = ref.c_sample_tau(t, np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(eta_prev), counts)
            assert tr["nchange"][it] == n and np.array_equal(taus[it], t), it
            eta_prev = tr["eta"][it]
        ref.c_freeRNG()
        # update_tau: three sweeps with the same gamma and eta are three consecutive c_sample_tau calls
        gs = np.ascontiguousarray(np.broadcast_to(pi, (n_it,) + pi.shape))
        es = np.ascontiguousarray(np.broadcast_to(eta, (n_it, 4, 4)))
        want = R.ref_sweeps(ref, tau, pi, eta, counts, 99, n=n_it)
        _load(ctx, counts, tau, pi, eta, 99)
        ctx.update_tau(gs, es)
        nch = ctx.get_trace()["nchange"]
        R.assert_same([(ctx.get_tau_at(i), int(nch[i])) for i in range(n_it)], want, "update_tau")
    finally:
        ctx.set_tau_neartie(-1)


# ------------------------------------------------------------------------------------------------------------------- legacy shim
def test_legacy_shim_runs_the_reference_call_sequence(ref):
    """dsm_initRNG / dsm_setRNG / dsm_sample_tau through desman_amd.sampletau, the calls the reference's module makes: the stream
    dsm_initRNG leaves (seed 4357), seed 0 (the same stream), a seed, and a reseed in mid-stream; draws carry over between calls"""
    from desman_amd import sampletau
    counts, tau, pi, eta = R.state(30, 17, 5, "random", seed=606)
    for seed in (None, 0, 77):
        R.assert_same(shim_sweeps(tau, pi, eta, counts, seed), R.ref_sweeps(ref, tau, pi, eta, counts, seed), "seed %r:" % (seed,))
    R.assert_same(R.ref_sweeps(ref, tau, pi, eta, counts, 0), R.ref_sweeps(ref, tau, pi, eta, counts, None), "reference, seed 0 against unseeded:")
    ref.c_initRNG(); ref.c_setRNG(5)
    sampletau.initRNG(); sampletau.setRNG(5)
    t, d = tau.copy(), tau.copy()
    for k in range(4):
        if k == 2:
            ref.c_setRNG(5); sampletau.setRNG(5)
        n = ref.c_sample_tau(t, pi, eta, counts)
        assert sampletau.sample_tau(d, pi, eta, counts) == n and np.array_equal(d, t), k
    ref.c_freeRNG(); sampletau.freeRNG()


# ------------------------------------------------------------------------------------------------------------------- (float) cast, degenerate operands
def test_float_cast_table_through_context_and_shim(ctx, ref):
    """the table whose draws the `(float)` cast of c_sample_tau.c:164 decides (tests/_ref_sweep.py: float_cast_table; the CPU file shows
    that exact-double counts draw other bases on it): kernels_gibbs.hip's cast site"""
    counts, tau, pi, eta = R.float_cast_table()
    want = R.ref_sweeps(ref, tau, pi, eta, counts, R.FLOAT_CAST_SEED)
    R.assert_same(ctx_sweeps(ctx, counts, tau, pi, eta, R.FLOAT_CAST_SEED), want, "context:")
    R.assert_same(shim_sweeps(tau, pi, eta, counts, R.FLOAT_CAST_SEED), want, "shim:")


@pytest.mark.parametrize("kind", R.DEGENERATE)
def test_degenerate_operands_through_context_and_shim(ctx, ref, kind):
    """DESIGN.md sec. 4 "Degenerate inputs": -inf and NaN walk through the device sweep as through the reference's plain IEEE code"""
    counts, tau, pi, eta, seed = R.degenerate_table(kind)
    want = R.ref_sweeps(ref, tau, pi, eta, counts, seed)
    R.assert_same(shim_sweeps(tau, pi, eta, counts, seed), want, "shim:")
    R.assert_same(ctx_sweeps(ctx, counts, tau, pi, eta, seed), want, "context:")


# ------------------------------------------------------------------------------------------------------------------- the other cast sites
def test_held_sweep_with_nothing_held(ctx, ref):
    """dsm_ctx_sample_tau_held(0) is a full sweep by the held kernel (kernels_heldtau.hip's cast site), on the float-cast table too"""
    for counts, tau, pi, eta, seed in [R.state(40, 33, 5, "random", seed=707) + (8,), R.float_cast_table() + (R.FLOAT_CAST_SEED,)]:
        want = R.ref_sweeps(ref, tau, pi, eta, counts, seed)
        R.assert_same(ctx_sweeps(ctx, counts, tau, pi, eta, seed, sweep=lambda c: c.sample_tau_held(0)), want, "held sweep:")


def test_gene_sampler_sweep_all(ref):
    """dsm_genes_sweep_all on the GSL stream (genes.hip's cast site): every gene with variants and a non-empty mask, in gene order on one
    stream, is c_sample_tau with the gene's masked abundances (Eta_Sampler.py:355-369: exact zeros) -- three calls in a row"""
    from _genes_util import _case, _device
    from oracle import ref_genes as rg
    k = _case(6, 20, 4, 9, seed=17, mean_lo=0.5, mean_hi=3.0)
    C, G, off = k['C'], k['G'], k['gene_off']
    rng = np.random.default_rng(2)
    eta0 = rng.integers(0, 2, size=(C, G))
    eta0[0, :] = 0                                                    # a gene in no haplotype: skipped, draws nothing
    eta0[1, :] = 0; eta0[1, 2] = 1                                    # a gene in exactly one
    eta0[2:][eta0[2:].sum(axis=1) == 0, 0] = 1
    Vtot = int(off[-1])
    tau0 = cbind.idx_to_onehot(rng.integers(0, 4, size=(Vtot, G)))
    dev, _ = _device(k, eta0, tau0, 2)
    try:
        dev.seed(3)
        ref.c_initRNG(); ref.c_setRNG(3)
        want = tau0.copy()
        for sweep in range(3):
            nch, _, _ = dev.sweep_all(None, sweep=1)
            _, got = dev.get_state()
            swept = 0
            for c in range(C):
                if off[c + 1] == off[c] or eta0[c].sum() == 0:
                    continue
                t = np.ascontiguousarray(want[off[c]:off[c + 1]])
                n = ref.c_sample_tau(t, np.ascontiguousarray(rg.mask_gamma(k['gamma'], eta0[c])), k['eps'], np.ascontiguousarray(k['variants'][c], dtype=np.int64))
                want[off[c]:off[c + 1]] = t
                assert nch[c] == n, (sweep, c)
                swept += 1
            assert swept >= 4 and np.array_equal(got, want), sweep
        ref.c_freeRNG()
    finally:
        dev.close()
