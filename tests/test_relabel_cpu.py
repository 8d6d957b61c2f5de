"""Label-switch-aware summaries, host side (desman_amd/relabel.py and the HaploSNP_Sampler methods on it), without a GPU: the
assignment solver against brute force and scipy, the summaries on a hand-built trace with planted switches served by a fake context
that computes the distances in numpy, and the command line's handling of --relabel-ref.  The device side is tests/test_gpu_relabel.py.
"""
import itertools
import os
import re

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, relabel
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler


# ---- 1. the assignment solver ----------------------------------------------------------------------------------------------------------
def _brute(c):
    n = c.shape[0]
    return min(sum(int(c[r, p[r]]) for r in range(n)) for p in itertools.permutations(range(n)))


def _matrices(rs, n):
    yield rs.randint(0, 1000, size=(n, n))
    yield rs.randint(0, 3, size=(n, n))                       # many ties
    yield rs.randint(0, 2, size=(n, n))
    yield np.full((n, n), 7)                                  # all equal: every permutation is optimal
    yield np.zeros((n, n), dtype=np.int64)
    yield rs.randint(-50, 50, size=(n, n))
    m = rs.randint(5, 9, size=(n, n))
    m[np.arange(n), np.arange(n)] = 5                         # the identity ties with others for the minimum
    yield m
    yield rs.randint(0, 300, size=(n, n)).astype(np.int32)    # the dtype trace_snd returns


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_solver_against_brute_force(n):
    rs = RandomState(100 + n)
    for rep in range(12):
        for c in _matrices(rs, n):
            perm, cost = relabel.min_cost_assignment(c)
            assert sorted(perm.tolist()) == list(range(n))
            assert cost == sum(int(c[r, perm[r]]) for r in range(n)) == _brute(c)
            if int(np.trace(c)) == cost:                      # the identity rule
                assert perm.tolist() == list(range(n))


@pytest.mark.parametrize("n", list(range(7, 33)))
def test_solver_against_scipy(n):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rs = RandomState(200 + n)
    for c in _matrices(rs, n):
        perm, cost = relabel.min_cost_assignment(c)
        r, k = lsa(c)
        assert sorted(perm.tolist()) == list(range(n))
        assert cost == sum(int(c[i, perm[i]]) for i in range(n)) == int(c[r, k].sum())
        if int(np.trace(c)) == cost:
            assert perm.tolist() == list(range(n))


def test_solver_refuses_what_it_cannot_solve():
    with pytest.raises(ValueError):
        relabel.min_cost_assignment(np.zeros((2, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        relabel.min_cost_assignment(np.zeros((2, 2)))


# ---- 2. the summaries on a planted trace, distances served by numpy ---------------------------------------------------------------------
class FakeCtx:
    """what the summaries use of _lib.Context, restated in numpy on digits: trace [n, V, G], star [V, G]"""

    def __init__(self, trace, star):
        self.trace, self.star = np.asarray(trace), np.asarray(star)
        self.n_trace, self.V, self.G = self.trace.shape
        self.calls = []

    def set_counts(self, v):
        pass

    def set_priors(self, *a):
        pass

    def trace_snd(self, mode=_lib.SND_STAR, ref=None, it0=0, n_it=None):
        self.calls.append(mode)
        t = self.trace
        if mode == _lib.SND_SELF:
            return (t[:, :, :, None] != t[:, :, None, :]).sum(axis=1).astype(np.int32)
        r = self.star if mode == _lib.SND_STAR else np.asarray(ref)
        return (t[:, :, :, None] != r[None, :, None, :]).sum(axis=1).astype(np.int32)

    def get_tau_sum_perm(self, perm, it0=0):
        out = np.zeros((self.V, self.G, 4), dtype=np.int64)
        for t in range(self.n_trace):
            for g in range(self.G):
                out[np.arange(self.V), perm[t, g], self.trace[t, :, g]] += 1
        return out


V, S, G, N = 150, 5, 4, 24
SWAP = {t: (1, 0, 2, 3) for t in range(6, 11)}
SWAP.update({t: (1, 2, 0, 3) for t in range(17, 24)})


def _planted():
    rs = RandomState(11)
    base = rs.randint(0, 4, size=(V, G))
    sigma = np.array([SWAP.get(t, (0, 1, 2, 3)) for t in range(N)])          # iteration t's haplotype g carries base haplotype sigma[t, g]
    trace = np.stack([base[:, sigma[t]] for t in range(N)])
    flip = rs.random_sample(trace.shape) < 0.03
    trace = np.where(flip, (trace + rs.randint(1, 4, size=trace.shape)) % 4, trace)
    gamma_store = rs.dirichlet(np.ones(G), size=(N, S))
    return base, sigma, trace, gamma_store


@pytest.fixture()
def planted():
    base, sigma, trace, gamma_store = _planted()
    ctx = FakeCtx(trace, base)
    smp = HaploSNP_Sampler(np.ones((V, S, 4), dtype=np.int64), G, RandomState(1), max_iter=N, ctx=ctx)
    smp.gamma_store = gamma_store
    smp.tau_star = HaploSNP_Sampler._onehot(base)
    smp._have_trace = True
    return smp, ctx, base, sigma, trace, gamma_store


def test_relabelling_finds_the_planted_switches_from_one_distance_call(planted):
    smp, ctx, base, sigma, trace, _ = planted
    rel = smp.relabelling()
    assert ctx.calls == [_lib.SND_STAR]                        # one trace_snd call, and the result is kept
    assert smp.relabelling() is rel and ctx.calls == [_lib.SND_STAR]
    assert rel["perm"].dtype == np.uint8 and np.array_equal(rel["perm"], sigma)
    d = (trace[:, :, :, None] != base[None, :, None, :]).sum(axis=1)
    assert np.array_equal(rel["cost_identity"], np.trace(d, axis1=1, axis2=2))
    assert np.array_equal(rel["cost_best"], [d[t, np.arange(G), sigma[t]].sum() for t in range(N)])
    assert (rel["cost_best"] <= rel["cost_identity"]).all()
    assert np.array_equal(smp.traceSND(), d) and np.array_equal(smp.traceSND(ref=base[:, :2]), d[:, :, :2])
    # another reference: the labels follow it
    other = base[:, [2, 0, 1, 3]]
    rel2 = smp.relabelling(ref=other)
    assert np.array_equal(rel2["perm"], np.array([1, 2, 0, 3])[sigma])
    with pytest.raises(ValueError, match="150 positions and 4 haplotypes"):
        smp.relabelling(ref=base[:, :3])


def test_gamma_mean_relabelled(planted):
    smp, _, _, sigma, _, gamma_store = planted
    want = np.zeros((S, G))
    for t in range(N):
        for g in range(G):
            want[:, sigma[t, g]] += gamma_store[t][:, g]
    want /= N
    got = smp.gammaMeanRelabelled()
    assert np.abs(got - want).max() <= 1e-13                  # N <= 1000 values in [0, 1]: summation order only
    assert np.abs(got - smp.gammaMean()).max() > 0.01         # the plain mean mixes the switched columns
    assert np.abs(got.sum(axis=1) - 1.0).max() <= 1e-13


def test_tau_mean_relabelled_counts_under_the_new_labels(planted):
    smp, _, base, sigma, trace, _ = planted
    got = smp.tauMeanRelabelled()
    want = np.zeros((V, G, 4))
    for t in range(N):
        for g in range(G):
            want[np.arange(V), sigma[t, g], trace[t, :, g]] += 1.0
    assert np.array_equal(got, want / N)
    assert np.take_along_axis(got, base[:, :, None], axis=2).min() > 0.5


def test_snd_posterior(planted):
    smp, _, base, sigma, trace, _ = planted
    post = smp.sndPosterior(level=0.9)
    pairs = [(g, h) for g in range(G) for h in range(g + 1, G)]
    assert post["pairs"].tolist() == [list(p) for p in pairs]
    inv = np.argsort(sigma, axis=1)
    for k, (g, h) in enumerate(pairs):
        x = np.array([(trace[t, :, inv[t, g]] != trace[t, :, inv[t, h]]).sum() for t in range(N)], dtype=np.float64)
        assert abs(post["mean"][k] - x.mean()) <= 1e-10 and abs(post["sd"][k] - x.std()) <= 1e-10
        assert post["lo"][k] == np.quantile(x, 0.05) and post["med"][k] == np.quantile(x, 0.5) and post["hi"][k] == np.quantile(x, 0.95)
        assert post["map"][k] == (base[:, g] != base[:, h]).sum()
        assert post["lo"][k] <= post["med"][k] <= post["hi"][k]
    with pytest.raises(ValueError):
        smp.sndPosterior(level=1.0)


def test_snd_posterior_under_a_reference_with_other_labels(planted):
    """with relabel_ref the pairs carry the REFERENCE's labels: every column of a row, map included, speaks of the same two strains"""
    smp, _, base, sigma, trace, _ = planted
    order = np.array([2, 0, 3, 1])
    smp.relabel_ref = np.ascontiguousarray(base[:, order])     # reference label j = base haplotype order[j]; tau_star keeps base's labels
    post = smp.sndPosterior(level=0.9)
    where = np.argsort(sigma, axis=1)                          # where[t, b] = the iteration's haplotype that carries base haplotype b
    dist = lambda a, b: int((base[:, a] != base[:, b]).sum())
    assert len({dist(a, b) for a in range(G) for b in range(a + 1, G)}) == G * (G - 1) // 2     # the pairs can be told apart
    for k, (g, h) in enumerate(post["pairs"].tolist()):
        a, b = order[g], order[h]
        x = np.array([(trace[t, :, where[t, a]] != trace[t, :, where[t, b]]).sum() for t in range(N)], dtype=np.float64)
        assert abs(post["mean"][k] - x.mean()) <= 1e-10 and post["med"][k] == np.quantile(x, 0.5)
        assert post["map"][k] == dist(a, b)
        assert abs(post["mean"][k] - post["map"][k]) < 0.1 * V  # ~3 % flips: the posterior of a pair sits near its own MAP distance
    plain = np.array([dist(g, h) for g, h in post["pairs"].tolist()])
    assert not np.array_equal(post["map"], plain)              # what the unpermuted MAP matrix would have put there
    st = smp.haplotypeStability()
    assert st["max"].max() < 0.15 and np.array_equal(smp.relabelling()["perm"], np.argsort(order)[sigma])


def test_haplotype_stability(planted):
    smp, _, base, sigma, trace, _ = planted
    st = smp.haplotypeStability()
    inv = np.argsort(sigma, axis=1)
    frac = np.array([[(trace[t, :, inv[t, l]] != base[:, l]).mean() for l in range(G)] for t in range(N)])
    assert np.abs(st["mean"] - frac.mean(axis=0)).max() <= 1e-13 and np.array_equal(st["max"], frac.max(axis=0))
    assert st["moved"].tolist() == [12, 12, 7, 0]             # labels 0, 1: both planted blocks; label 2: the 3-cycle only
    assert st["max"].max() < 0.15                             # ~3 % flips: after relabelling every haplotype stays near its own


def test_summaries_need_a_trace():
    ctx = FakeCtx(np.zeros((1, 3, 2), dtype=np.int64), np.zeros((3, 2), dtype=np.int64))
    smp = HaploSNP_Sampler(np.ones((3, 2, 4), dtype=np.int64), 2, RandomState(1), max_iter=1, ctx=ctx)
    with pytest.raises(_lib.DesmanHipError, match="no update"):
        smp.relabelling()


# ---- 3. the library's surface and the command line -------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_snd", "dsm_ctx_get_tau_sum_perm", "dsm_ctx_debug_set_trace"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for k, name in enumerate(("STAR", "SELF", "GIVEN")):
        assert int(re.search(r"#define\s+DSM_SND_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, "SND_" + name) == k
    assert all(callable(getattr(_lib.Context, m)) for m in ("trace_snd", "get_tau_sum_perm", "debug_set_trace"))
    assert lib.dsm_ctx_trace_snd(None, 0, None, 0, 0, 0, None) == -2 and lib.dsm_ctx_get_tau_sum_perm(None, None, 0, 0, None) == -2
    assert lib.dsm_ctx_debug_set_trace(None, None, 0) == -2


def _write_freq(path, counts, positions, contigs):
    Vn, Sn, _ = counts.shape
    cols = ["Position"] + ["S%d-%s" % (s, b) for s in range(Sn) for b in "ACGT"]
    df = pd.DataFrame(np.concatenate([np.asarray(positions)[:, None], counts.reshape(Vn, Sn * 4)], axis=1), index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def _write_tau(path, digits, positions, contigs):
    onehot = HaploSNP_Sampler._onehot(np.asarray(digits))
    df = pd.DataFrame(onehot.reshape(onehot.shape[0], -1), index=list(contigs))
    df.insert(0, "Position", positions)
    df.to_csv(path)


def test_relabel_ref_is_checked_before_any_chain(tmp_path):
    from desman_amd import cli
    Vn, Sn = 30, 3
    rs = RandomState(3)
    counts = rs.randint(20, 60, size=(Vn, Sn, 4))
    positions, contigs = np.arange(Vn) * 5 + 2, ["c%d" % (v // 10) for v in range(Vn)]
    freq = str(tmp_path / "t.freq")
    _write_freq(freq, counts, positions, contigs)
    digits = rs.randint(0, 4, size=(Vn, 3))
    good, wrong_g, wrong_pos, fewer, not_tau = (str(tmp_path / n) for n in ("good.csv", "g.csv", "pos.csv", "fewer.csv", "no.csv"))
    _write_tau(good, digits, positions, contigs)
    _write_tau(wrong_g, digits[:, :2], positions, contigs)
    _write_tau(wrong_pos, digits, positions + 1, contigs)
    _write_tau(fewer, digits[:-1], positions[:-1], contigs[:-1])
    pd.DataFrame(np.ones((Vn, 3)), index=contigs).to_csv(not_tau)
    assert np.array_equal(relabel.read_reference(good, positions, contigs, 3), digits)
    args = [freq, "-g", "3", "-i", "5", "-m", "0", "-o", str(tmp_path / "out")]
    for path, what in ((wrong_g, "holds 2 haplotypes, this run infers 3"), (wrong_pos, "other positions"), (fewer, "other positions"),
                       (not_tau, "not a Filtered_Tau_star.csv"), (str(tmp_path / "missing.csv"), "can't open")):
        with pytest.raises(SystemExit) as e:
            cli.main(args + ["--relabel", "--relabel-ref", path])
        assert "--relabel-ref" in str(e.value) and what in str(e.value), (path, e.value)
    assert not os.path.exists(str(tmp_path / "out" / "fit.txt"))
    opts = cli.build_parser().parse_args(args)
    assert opts.relabel is False and opts.relabel_ref is None
