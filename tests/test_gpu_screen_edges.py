"""The device tau sweeps on the adversarial near-edge tables of tests/_screen_edges.py (fixture tests/golden/screen_edges.npz; the CPU
side is tests/test_screen_edges_cpu.py): one step per table has its uniform 1e-2 ... 1e-9 from an edge of its conditional CDF, on either
side.  With the fp32 screens on and off the sweep must be the reference's compiled sweep (oracle/_ref; the oracle's on the Philox
stream), tau and nchange in whole, and the adversarial draw must be the one exact arithmetic makes -- a screen whose rounding budget is
too small certifies the wrong base on a near rung and nowhere else in the suite.

* totals cases run the single sweep (dsm_ctx_sample_tau) and the tau-only loop's instantiation (update_tau), whose finalize step keeps
  the counts of steps left to fp64;
* near-tie cases run tau_kernel_nt, which only the loop reaches: a context whose last gibbs_update chose that instantiation
  (dsm_ctx_set_tau_neartie(1)) runs it in update_tau on exactly the stored gamma and eta;
* the held sweep (dsm_ctx_sample_tau_held(0)) and the gene sampler (dsm_genes_sweep_all) have no screen: their own fp64 steps (table log,
  re-use of the current candidate's total, the gene's masked and re-normalised abundances) run one shape's cases.

Against a vacuous pass: screened, every shape leaves a step to fp64 on its 1e-8 rung, and over all shapes the 1e-2 rung leaves fewer
than the 1e-8 rung -- the screens do decide the far cases and do decline the near ones."""
import numpy as np
import pytest

import _ref_sweep as R
import _screen_edges as E
from desman_amd import _lib
from oracle import cbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return E.load()


@pytest.fixture(scope="module")
def ref():
    return R.reference()


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ntctx():
    """the context of the near-tie shapes (_prime)"""
    c = _lib.Context(0)
    yield c
    c.close()


def _prime(c, table):
    """Make the loop sweeps of context c run tau_kernel_nt.  Which instantiation the loop launches is the context's tau_neartie_on
    (kernels_gibbs.hip: launch_tau), and only a full gibbs_update sets it (api.hip: the call of k_tau_neartie_hint at the head of the
    Gibbs driver; dsm_ctx_update_tau makes none and runs "the same instantiation, as the Gibbs call left it",
    tests/test_gpu_ref_sweep.py).  So every near-tie shape runs one forced gibbs_update on a table of its own S and G first; that it took
    is checked by what the screen then decides (test_neartie_screen_near_an_edge)."""
    counts, tau, gamma, eta = table
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    c.seed(1, ctr_seed=2)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.set_tau_screen(True)
    c.set_tau_neartie(1)
    c.gibbs_update(1)


def _load(c, table, rng, seed, screen):
    counts, tau, gamma, eta = table
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    if rng == E.MT:
        c.seed(seed)
        c.set_tau_rng(_lib.RNG_MT19937)
    else:
        c.seed(123, ctr_seed=seed)
        c.set_tau_rng(_lib.RNG_PHILOX)
    c.set_screen_state(np.zeros(2, dtype=np.uint32))              # no suspension carried over from the table before
    c.set_tau_screen(screen)
    c.sweep_stats(reset=True)


def _want(ref, table, rng, seed):
    """(tau, nchange) of the reference's sweep (MT19937) or of the oracle's on the Philox uniforms"""
    counts, tau, gamma, eta = table
    if rng == E.MT:
        (t, n), = R.ref_sweeps(ref, tau, gamma, eta, counts, seed, n=1)
        return t, n
    t = tau.copy()
    n = cbind.sample_tau_u(t, gamma, eta, counts, E.uniforms(rng, seed, tau.shape[1]))
    return t, n


def _single(c):
    n = c.sample_tau()
    return c.get_state()[0], n


def _held(c):
    n = c.sample_tau_held(0)
    return c.get_state()[0], n


def _loop(c):
    _, gamma, eta = c.get_state()
    c.update_tau(np.ascontiguousarray(gamma[None]), np.ascontiguousarray(eta[None]))
    return c.get_tau_at(0), int(c.get_trace()["nchange"][0])


def _check(c, ref, sh, base, cs, entries, left, screens=(True, False)):
    """every case of a shape through every entry, screened and not; left[delta] += (wavefront-steps, of them left to fp64, cases a
    screen could decide, of them sweeps that left NO step to fp64: the screen did decide the adversarial step) of the screened loop"""
    gs, rng = base["gs"], sh[4]
    try:
        for i, case in enumerate(cs):
            table = E.case_table(base, case)
            t_ref, n_ref = _want(ref, table, rng, case["seed"])
            assert cbind.onehot_to_idx(t_ref)[case["vstar"], gs] == case["draw"]     # (tests/test_screen_edges_cpu.py holds the reference to it)
            for name, run in entries:
                for screen in screens:
                    what = "%s case %d, %s, screen %s: delta %g, u - edge = %.3e" % (E.shape_name(sh), i, name, "on" if screen else "off",
                                                                                    case["delta"], case["dist"])
                    _load(c, table, rng, case["seed"], screen)
                    t, n = run(c)
                    assert cbind.onehot_to_idx(t)[case["vstar"], gs] == case["draw"], what + ": the adversarial step drew another base"
                    assert np.array_equal(t, t_ref) and n == n_ref, what + ": the sweep is not the reference's"
                    if screen and name == "loop":
                        steps, exact = c.sweep_stats()
                        assert steps > 0, what
                        # a totals screen can only ever certify `best`: the cases in which exact arithmetic draws it
                        open_to = sh[0] == E.NEARTIE or case["draw"] == case["b0"]
                        row = left.setdefault(case["delta"], [0, 0, 0, 0])
                        row[0] += steps
                        row[1] += exact
                        row[2] += int(open_to)
                        row[3] += int(open_to and exact == 0)
    finally:
        c.set_tau_screen(True)
        c.set_tau_rng(_lib.RNG_MT19937)


_TOTALS = [i for i, sh in enumerate(E.SHAPES) if sh[0] == E.TOTALS]
_NEARTIE = [i for i, sh in enumerate(E.SHAPES) if sh[0] == E.NEARTIE]


@pytest.fixture(scope="module")
def runs(ctx, ntctx, ref, fix):
    """si -> the counts _check gathers on all cases of shape si, run once per module whichever test asks first"""
    done = {}

    def run(si):
        if si not in done:
            sh, base, cs = fix[si]
            left = {}
            if sh[0] == E.NEARTIE:
                _prime(ntctx, E.case_table(base, cs[0]))
                _check(ntctx, ref, sh, base, cs, [("loop", _loop)], left)
            else:
                _check(ctx, ref, sh, base, cs, [("single", _single), ("loop", _loop)], left)
            print("%-28s per rung, wavefront-steps left to fp64 (sweeps wholly screened / cases a screen could decide): %s" %
                  (E.shape_name(sh), ", ".join("%g: %d/%d (%d/%d)" % ((d, v[1], v[0], v[3], v[2])) for d, v in sorted(left.items(), reverse=True))))
            assert left[1e-8][1] >= 1, "no step of the 1e-8 rung went to fp64: the adversarial step cannot have been screened as built"
            done[si] = left
        return done[si]
    return run


@pytest.mark.parametrize("si", _TOTALS, ids=[E.shape_name(E.SHAPES[i]) for i in _TOTALS])
def test_totals_screen_near_an_edge(runs, si):
    """screen_certify through sweep_screen / sweep_screen32: the single sweep and the loop's instantiation"""
    runs(si)


@pytest.mark.parametrize("si", _NEARTIE, ids=[E.shape_name(E.SHAPES[i]) for i in _NEARTIE])
def test_neartie_screen_near_an_edge(runs, si):
    """sweep_neartie_core through sweep_neartie / sweep_neartie32: tau_kernel_nt in the tau-only loop"""
    left = runs(si)
    assert left[1e-2][1] < left[1e-8][1], "the near-tie screen decided nothing: is tau_kernel_nt running?"


def test_screens_decide_the_far_rungs_and_decline_the_near_ones(runs):
    """over all shapes: fewer steps left to fp64 on the 1e-2 rung than on the 1e-8 rung"""
    left = [runs(si) for si in _TOTALS + _NEARTIE]
    for d in E.LADDER:
        rows = [v[d] for v in left if d in v]
        print("rung %g: %d of %d wavefront-steps left to fp64; sweeps wholly screened %d of the %d a screen could decide" %
              (d, sum(r[1] for r in rows), sum(r[0] for r in rows), sum(r[3] for r in rows), sum(r[2] for r in rows)))
    far, near = sum(v[1e-2][1] for v in left), sum(v[1e-8][1] for v in left)
    assert far < near, (far, near)


def test_held_sweep_near_an_edge(ctx, ref, fix):
    """kernels_heldtau.hip with nothing held: a full sweep by the held kernel, which has no screen -- its fp64 step and draw alone"""
    sh, base, cs = fix[E.SHAPES.index(E.GENE_SHAPE)]
    _check(ctx, ref, sh, base, cs, [("held", _held)], {}, screens=(True,))


def test_gene_sampler_near_an_edge(ref, fix):
    """dsm_genes_sweep_all (genes.hip: its own fp64 step) on one gene that every haplotype carries: the sweep is c_sample_tau on the
    gene's masked, re-normalised abundances (Eta_Sampler.py:355-369; tests/test_screen_edges_cpu.py shows that the re-normalisation
    leaves the 1e-8 and 1e-9 rungs where they are) and the adversarial draw is the exact one"""
    from _genes_util import _device
    sh, base, cs = fix[E.SHAPES.index(E.GENE_SHAPE)]
    S, G, gs = base["S"], base["G"], base["gs"]
    for i, case in E.gene_cases(cs):
        counts, tau, gamma, eta = E.case_table(base, case)
        what = "gene sweep, %s case %d: delta %g, u - edge = %.3e" % (E.shape_name(sh), i, case["delta"], case["dist"])
        (t_ref, n_ref), = R.ref_sweeps(ref, tau, E.masked_gamma(gamma), eta, counts, case["seed"], n=1)
        assert cbind.onehot_to_idx(t_ref)[case["vstar"], gs] == case["draw"]
        k = dict(d=dict(counts=counts), C=1, gene_off=np.array([0, E.V], dtype=np.int32), cov=np.full((1, S), 30.0), gamma=gamma, eps=eta,
                 delta_gs=np.ascontiguousarray((gamma * 30.0).T))
        dev, _ = _device(k, np.ones((1, G), dtype=np.int32), tau, 2)
        try:
            dev.seed(case["seed"])
            nch, _, _ = dev.sweep_all(None, sweep=1)
            _, t = dev.get_state()
        finally:
            dev.close()
        assert cbind.onehot_to_idx(t)[case["vstar"], gs] == case["draw"], what + ": the adversarial step drew another base"
        assert np.array_equal(t, t_ref) and nch[0] == n_ref, what + ": the sweep is not the reference's"
