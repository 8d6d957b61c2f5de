"""The adversarial near-edge tables of tests/_screen_edges.py (fixture tests/golden/screen_edges.npz) on the CPU: the fixture is what the
generator makes, bit for bit; on EVERY case both the oracle's sweep and the reference's own compiled sweep draw what exact arithmetic
(mpmath, 60 digits) draws -- at the adversarial step and at every other step of the table --, which is what lets
tests/test_gpu_screen_edges.py hold the kernels to these cases; and the float32 restatement of screen_certify certifies the far rungs of
every totals shape and not the near ones, so the ladder does straddle the screen's budget."""
import numpy as np
import pytest

import _ref_sweep as R
import _screen_edges as E
from oracle import cbind


@pytest.fixture(scope="module")
def fix():
    return E.load()


@pytest.fixture(scope="module")
def ref():
    return R.reference()


def _ids():
    return [E.shape_name(sh) for sh in E.SHAPES]


@pytest.mark.parametrize("si", [0, 9, 10, 16, 18, 20, 21, 23])
def test_fixture_is_what_the_generator_makes(fix, si):
    """a sample of shapes (every kind, both streams, the smallest and the largest G), the first case, the 1e-8 rung and the last one
    (1e-9) of each regenerated with mpmath: seed, position, the private gamma row, the achieved distance, the exact sweep -- all equal"""
    pytest.importorskip("mpmath")
    sh, base, cs = fix[si]
    b = E.Builder(sh)
    spec = [c for c in E.cases_of(sh) if c[3] not in E.DROPPED.get(E.shape_name(sh), ())]
    assert len(spec) == len(cs)
    at_1e8 = [i for i, c in enumerate(spec) if c[3] == 1e-8]
    for i in (0, at_1e8[0], at_1e8[-1], len(cs) - 1):
        want = b.case(E.cases_of(sh).index(spec[i]))
        got = cs[i]
        for k in ("b0", "k", "side", "delta", "seed", "vstar", "dist", "draw"):
            assert got[k] == want[k], (E.shape_name(sh), i, k, got[k], want[k])
        assert np.array_equal(got["grow"], want["grow"]) and np.array_equal(got["new"], want["new"]), (E.shape_name(sh), i)


def test_every_shape_keeps_the_ladder_down_to_1e_8(fix):
    """both sides of every rung down to 1e-8 for every shape and edge; achieved distances within 1e-3 of the rung"""
    assert len(fix) == len(E.SHAPES)
    for sh, base, cs in fix:
        per_edge = {}
        for c in cs:
            per_edge.setdefault((c["b0"] if sh[0] == E.TOTALS else -1, c["k"]), set()).add((c["delta"], c["side"]))
            assert abs(c["dist"] - c["side"] * c["delta"]) <= 1e-3 * c["delta"]
        assert len(per_edge) == (2 if sh[0] == E.TOTALS else 3)
        for have in per_edge.values():
            assert all((d, s) in have for d in E.LADDER[:-1] for s in (1, -1)), E.shape_name(sh)
        kept = sorted({c["delta"] for c in cs}, reverse=True)
        worst = max(abs(abs(c["dist"]) / c["delta"] - 1.0) for c in cs)
        print("%-28s rungs %s, %d cases, | |u - edge| / delta - 1 | <= %.1e" % (E.shape_name(sh), " ".join("%g" % d for d in kept), len(cs), worst))


@pytest.mark.parametrize("si", range(len(E.SHAPES)), ids=_ids())
def test_oracle_and_reference_draw_the_exact_base(fix, ref, si):
    """every case of the shape: cbind.sample_tau_u and (MT19937 stream) the reference's compiled c_sample_tau give the mpmath sweep, the
    whole of it, and so the recorded draw at (v*, g*)"""
    sh, base, cs = fix[si]
    G, gs, rng = base["G"], base["gs"], sh[4]
    for i, c in enumerate(cs):
        counts, tau, gamma, eta = E.case_table(base, c)
        what = "%s case %d (delta %g, side %+d, u - edge = %.3e)" % (E.shape_name(sh), i, c["delta"], c["side"], c["dist"])
        assert c["new"][c["vstar"], gs] == c["draw"]
        t = tau.copy()
        cbind.sample_tau_u(t, gamma, eta, counts, E.uniforms(rng, c["seed"], G))
        got = cbind.onehot_to_idx(t)
        assert got[c["vstar"], gs] == c["draw"], "oracle, " + what
        assert np.array_equal(got, c["new"]), "oracle, another step of " + what
        if rng == E.MT:
            (tr, _), = R.ref_sweeps(ref, tau, gamma, eta, counts, c["seed"], n=1)
            got = cbind.onehot_to_idx(tr)
            assert got[c["vstar"], gs] == c["draw"], "reference, " + what
            assert np.array_equal(got, c["new"]), "reference, another step of " + what


@pytest.mark.parametrize("si", [i for i, sh in enumerate(E.SHAPES) if sh[0] == E.TOTALS], ids=[E.shape_name(sh) for sh in E.SHAPES if sh[0] == E.TOTALS])
def test_ladder_straddles_the_budget_of_screen_certify(fix, si):
    """screen_certify as written, restated in float32: it certifies on some rung of the shape and declines on another (the ladder reaches
    its budget from both sides), and it never certifies a base that exact arithmetic does not draw"""
    sh, base, cs = fix[si]
    G, gs, S = base["G"], base["gs"], base["S"]
    verdict = {}
    for c in cs:
        counts, tau, gamma, eta = E.case_table(base, c)
        row = cbind.onehot_to_idx(tau)[c["vstar"]]
        uw = int(round(E.uniforms(sh[4], c["seed"], G)[c["vstar"] * G + gs] * 4294967296.0))
        ok, best = E.screen_would_certify(counts[c["vstar"]], row, gs, gamma, eta, uw, S)
        verdict.setdefault(c["delta"], []).append(ok)
        assert not ok or best == c["draw"], (E.shape_name(sh), c["delta"], c["side"])
    print("%-28s certified per rung: %s" % (E.shape_name(sh), ", ".join("%g: %d/%d" % (d, sum(v), len(v)) for d, v in sorted(verdict.items(), reverse=True))))
    flat = [ok for v in verdict.values() for ok in v]
    assert any(flat) and not all(flat)
    assert any(verdict[1e-2])


def test_gene_cases_keep_their_distance_on_the_masked_abundances(fix, ref):
    """the cases the gene sampler runs (tests/test_gpu_screen_edges.py) sweep on gamma re-normalised per sample: the reference's sweep on
    those abundances still gives the recorded sweep, and (mpmath) the adversarial uniform is still the recorded distance from its edge"""
    sh, base, cs = fix[E.SHAPES.index(E.GENE_SHAPE)]
    G, gs = base["G"], base["gs"]
    picked = E.gene_cases(cs)
    assert {(c["delta"], c["side"], c["b0"]) for _, c in picked} == {(d, s, b) for d in (1e-8, 1e-9) for s in (1, -1) for b in (3, 0)}
    for i, c in picked:
        counts, tau, gamma, eta = E.case_table(base, c)
        gm = E.masked_gamma(gamma)
        (tr, _), = R.ref_sweeps(ref, tau, gm, eta, counts, c["seed"], n=1)
        assert np.array_equal(cbind.onehot_to_idx(tr), c["new"]), i
    mp = pytest.importorskip("mpmath")
    for i, c in picked:
        counts, tau, gamma, eta = E.case_table(base, c)
        v = c["vstar"]
        row = np.concatenate([c["new"][v][:gs], cbind.onehot_to_idx(tau)[v][gs:]]).astype(np.int64)
        ed = E.mp_edges(counts[v], row, gs, E.masked_gamma(gamma), eta)
        u = mp.mpf(float(E.uniforms(sh[4], c["seed"], G)[v * G + gs]))
        assert abs(float(u - ed[c["k"]]) - c["side"] * c["delta"]) <= 1e-3 * c["delta"], i
        assert E._draw(ed, u) == c["draw"], i
