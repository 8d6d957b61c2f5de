"""Posterior predictive fit, host side (desman_amd/check.py, HaploSNP_Sampler.fitCheck, the `desman --check` writers), without a GPU:
the exact moments of Pearson's X by enumeration, the restatement against Python loops, the recovery of a planted misfit sample at the
generating parameters (the device call served by a numpy stand-in context), the library's surface and the command line's refusals.
The device side is tests/test_gpu_check.py.
"""
import itertools
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, check
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
from desman_amd.Output_Results import Output_Results
from desman_amd.synth import synth_counts

EYE = np.eye(4)
DIG = np.arange(4)[None, :]              # one position, four haplotypes, haplotype g carries base g: with eta = I, p_b = gamma[s][b]


# ---- 1. E and W are the exact mean and variance of X under multinomial(N, p) ----------------------------------------------------------
def pearson_moments_bruteforce(N, p):
    """mean and variance of X over every outcome of multinomial(N, p), X taken from check.cell_terms"""
    support = [b for b in range(4) if p[b] > 0]
    m1 = m2 = total = 0.0
    for parts in itertools.product(range(N + 1), repeat=len(support)):
        if sum(parts) != N:
            continue
        n = np.zeros(4, dtype=np.int64)
        n[support] = parts
        pmf = math.factorial(N)
        for b in support:
            pmf = pmf / math.factorial(int(n[b])) * p[b] ** int(n[b])
        x = float(check.cell_terms(n[None, None, :], DIG, np.asarray(p)[None, :], EYE)["X"][0, 0])
        m1, m2, total = m1 + pmf * x, m2 + pmf * x * x, total + pmf
    assert abs(total - 1.0) < 1e-12
    return m1, m2 - m1 * m1


P_VECTORS = [(0.5, 0.5, 0.0, 0.0), (0.9, 0.0, 0.1, 0.0), (0.0, 0.25, 0.0, 0.75), (0.2, 0.3, 0.5, 0.0), (0.0, 0.6, 0.3, 0.1),
             (0.25, 0.25, 0.25, 0.25), (0.7, 0.1, 0.15, 0.05), (0.96, 0.02, 0.01, 0.01)]


@pytest.mark.parametrize("p", P_VECTORS)
def test_exact_moments_of_pearson_x(p):
    k = sum(1 for x in p if x > 0)
    for N in range(1, 7):
        n = np.zeros((1, 1, 4), dtype=np.int64)
        n[0, 0, [b for b in range(4) if p[b] > 0][0]] = N
        c = check.cell_terms(n, DIG, np.asarray(p)[None, :], EYE)
        E, W = float(c["E"][0, 0]), float(c["W"][0, 0])
        mean, var = pearson_moments_bruteforce(N, p)
        assert E == k - 1 and abs(mean - E) <= 1e-12 and abs(var - W) <= 1e-12 * max(1.0, W), (N, p, mean, E, var, W)


# ---- 2. the restatement against Python loops ---------------------------------------------------------------------------------------
def cell_loops(n, digits, gamma_s, eta):
    """(X, D, E, W) of one cell by the definitions, in Python floats"""
    N = int(sum(n))
    if N == 0:
        return 0.0, 0.0, 0.0, 0.0
    p = [sum(gamma_s[g] * eta[digits[g]][b] for g in range(len(digits))) for b in range(4)]
    k = sum(1 for b in range(4) if p[b] > 0)
    X = D = 0.0
    for b in range(4):
        if p[b] > 0:
            X += (n[b] - N * p[b]) ** 2 / (N * p[b])
            if n[b] > 0:
                D += 2.0 * n[b] * math.log(n[b] / (N * p[b]))
        elif n[b] > 0:
            X = D = math.inf
    W = 2.0 * (k - 1) + (sum(1.0 / x for x in p if x > 0) - k * k - 2 * k + 2) / N
    return X, D, float(k - 1), W


def _degenerate_case():
    """V = 5, S = 4, G = 3 with every special operand: an empty sample (3), an empty position (4), exact zeros in eta (no read of base
    3 is ever produced; base 2 only by true base 2) and in gamma (sample 1 has no haplotype 2), one cell (0, 1) with reads where p = 0"""
    rs = RandomState(5)
    counts = rs.randint(1, 40, size=(5, 4, 4)).astype(np.int64)
    counts[:, :, 3] = 0                                     # p_3 = 0 everywhere and n_3 = 0: contributes exactly 0
    counts[:, 3, :] = 0
    counts[4, :, :] = 0
    digits = np.array([[0, 1, 2], [0, 0, 1], [1, 1, 1], [2, 0, 1], [0, 1, 2]])
    gamma = np.array([[0.5, 0.3, 0.2], [0.6, 0.4, 0.0], [0.1, 0.1, 0.8], [1.0, 0.0, 0.0]])
    eta = np.array([[0.9, 0.1, 0.0, 0.0], [0.1, 0.9, 0.0, 0.0], [0.05, 0.05, 0.9, 0.0], [0.25, 0.25, 0.5, 0.0]])
    counts[1, :, 2] = 0                                     # position 1 carries no true base 2: p_2 = 0, n_2 = 0 -> finite
    counts[2, :, 2] = 0
    counts[0, 1, 2] = 7                                     # sample 1 has gamma_2 = 0, so p_2 = 0 at position 0: this cell is infinite
    counts[3, 1, 2] = 0
    return counts, digits, gamma, eta


def test_cell_terms_against_python_loops():
    for seed in range(3):
        rs = RandomState(seed)
        V, S, G = 7, 5, 4
        counts = rs.randint(0, 30, size=(V, S, 4)).astype(np.int64)
        counts[2, 1] = 0
        digits = rs.randint(0, 4, size=(V, G))
        gamma = rs.dirichlet(np.ones(G), size=S)
        eta = 0.9 * np.eye(4) + 0.1 * rs.dirichlet(np.ones(4), size=4)
        c = check.cell_terms(counts, digits, gamma, eta)
        for v in range(V):
            for s in range(S):
                want = cell_loops(counts[v, s].tolist(), digits[v].tolist(), gamma[s].tolist(), eta.tolist())
                got = [float(c[key][v, s]) for key in "XDEW"]
                assert all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got, want)), (v, s, got, want)
        assert (c["absD"] >= np.abs(c["D"]) * (1 - 1e-15)).all() and np.allclose(c["absX"], c["X"], rtol=1e-15)
        assert not c["X"][2, 1] and not c["W"][2, 1] and not c["E"][2, 1] and not c["D"][2, 1]


def test_degenerate_operands_give_inf_only_where_reads_meet_p_zero():
    counts, digits, gamma, eta = _degenerate_case()
    c = check.cell_terms(counts, digits, gamma, eta)
    assert not any(np.isnan(c[k]).any() for k in c)
    inf = np.zeros((5, 4), dtype=bool)
    inf[0, 1] = True
    assert np.array_equal(np.isinf(c["X"]), inf) and np.array_equal(np.isinf(c["D"]), inf) and np.isfinite(c["W"]).all()
    for v in range(5):
        for s in range(4):
            want = cell_loops(counts[v, s].tolist(), digits[v].tolist(), gamma[s].tolist(), eta.tolist())
            got = [float(c[key][v, s]) for key in "XDEW"]
            assert all(a == b or abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in zip(got, want)), (v, s, got, want)
    assert not c["X"][:, 3].any() and not c["X"][4].any() and not c["E"][4].any()
    sums = check.trace_sums(counts, digits, gamma[None], eta[None])
    assert np.array_equal(np.isinf(sums["sample"][:, 0]), [False, True, False, False])
    assert np.array_equal(np.isinf(sums["position"][:, 1]), [True, False, False, False, False])
    assert np.isfinite(sums["sample"][:, 2:]).all() and np.isfinite(sums["position"][:, 2:]).all()
    sc = check.fit_scores(sums, 1, counts)
    assert np.array_equal(sc["sample"]["cells"], [4, 4, 4, 0]) and np.array_equal(sc["position"]["cells"], [3, 3, 3, 3, 0])
    assert sc["sample"]["z"][1] == np.inf and sc["sample"]["z"][3] == 0 and sc["position"]["z"][4] == 0
    assert not np.isnan(sc["sample"]["z"]).any() and not np.isnan(sc["position"]["z"]).any()


# ---- 3. a planted sample the model does not explain, at the generating parameters --------------------------------------------------------
class FakeCtx:
    """what fitCheck uses of _lib.Context, served by check.trace_sums from planted traces"""

    def __init__(self, counts, digits, gamma, eta):
        self.counts, self.digits, self.gamma, self.eta = counts, digits, gamma, eta
        self.calls = []

    def set_counts(self, v):
        pass

    def set_priors(self, *a):
        pass

    def trace_fit_stats(self, it0=0, n_it=None, want=("sample", "position", "cell")):
        self.calls.append(tuple(want))
        n_it = len(self.gamma) - it0 if n_it is None else n_it
        s = check.trace_sums(self.counts, self.digits[it0:it0 + n_it], self.gamma[it0:it0 + n_it], self.eta[it0:it0 + n_it])
        out = {k: s[k] for k in want}
        out["n_it"] = n_it
        return out


PLANT = dict(V=300, S=12, G=3, seed=2024, sample=7, n=3)


def _planted():
    V, S, G, bad = PLANT["V"], PLANT["S"], PLANT["G"], PLANT["sample"]
    counts, tau, gamma = synth_counts(V, S, G, seed=PLANT["seed"])
    eta = 0.96 * np.eye(4) + 0.01
    rs = RandomState(PLANT["seed"])
    stranger = (tau[:, 0].astype(np.int64) + 1 + rs.randint(0, 3, size=V)) % 4          # differs from haplotype 0 at every position
    depth = counts[:, bad].sum(axis=1)
    counts[:, bad] = np.stack([rs.multinomial(int(depth[v]), eta[stranger[v]]) for v in range(V)])
    n = PLANT["n"]
    ctx = FakeCtx(counts, np.broadcast_to(tau.astype(np.int64), (n, V, G)), np.broadcast_to(gamma, (n, S, G)),
                  np.broadcast_to(eta, (n, 4, 4)))
    smp = HaploSNP_Sampler(counts, G, RandomState(1), max_iter=n, ctx=ctx)
    smp._have_trace = True
    return smp, ctx, counts


def test_planted_sample_is_recovered_and_kept():
    smp, ctx, counts = _planted()
    samples, positions = smp.fitCheck()
    z = samples["z"]
    bad = PLANT["sample"]
    others = np.delete(z, bad)
    print("z planted %.1f, others %.2f .. %.2f" % (z[bad], others.min(), others.max()))
    assert np.argmax(z) == bad and z[bad] > 10 and (others < 5).all()
    assert ctx.calls == [("sample", "position")] and smp.fitCheck()[0] is samples                 # kept: no second device call
    assert (samples["cells"] == (counts.sum(axis=2) > 0).sum(axis=0)).all() and positions["z"].shape == (PLANT["V"],)
    assert np.array_equal(samples["expected"], 3.0 * samples["cells"])                            # k = 4 everywhere: E = 3 per cell
    s2, p2, cell = smp.fitCheck(cells=True)
    assert ctx.calls[-1] == ("sample", "position", "cell") and len(ctx.calls) == 2 and cell.shape == counts.shape[:2]
    assert np.array_equal(s2["z"], z) and np.allclose(cell.sum(axis=0), s2["X2"], rtol=1e-12)
    assert np.argmax(cell.mean(axis=0)) == bad
    assert smp.fitCheck(cells=True)[2] is cell and len(ctx.calls) == 2
    smp._fit = None                                                                                # what the next update does
    assert smp.fitCheck()[0] is not samples


# ---- 4. the files' layout on a stand-in, the refusals, the library's surface ------------------------------------------------------------
def test_files_layout(tmp_path, caplog):
    import logging
    caplog.set_level(logging.INFO)
    smp, ctx, counts = _planted()
    V, S = counts.shape[:2]
    names = ["S%d" % s for s in range(S + 1)]                 # one more sample in the table than was kept
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    table = pd.DataFrame(np.zeros((V + 2, 1 + 4 * (S + 1)), dtype=np.int64), index=["c%d" % (v // 100) for v in range(V + 2)], columns=cols)
    table["Position"] = np.arange(V + 2) * 3 + 1

    class Flt:
        selected_indices = list(range(1, V + 1))
        sample_indices = [s for s in range(S + 1) if s != 2]
    report = Output_Results(str(tmp_path))
    report.set_Variants(table)
    report.set_Variant_Filter(Flt)
    report.haplo_SNP = smp
    samples, positions, cell = smp.fitCheck(cells=True)
    report.output_Fit(samples, positions)
    report.output_Fit_cells(cell)
    fs = pd.read_csv(str(tmp_path / "Fit_samples.csv"), float_precision="round_trip")
    kept = [n for k, n in enumerate(names) if k != 2]
    assert list(fs.columns) == ["sample", "cells", "X2", "expected", "z", "deviance"] and list(fs["sample"]) == kept
    for col, key in (("cells", "cells"), ("X2", "X2"), ("expected", "expected"), ("z", "z"), ("deviance", "deviance")):
        assert np.array_equal(fs[col].to_numpy(), samples[key]), col
    fp = pd.read_csv(str(tmp_path / "Fit_positions.csv"), float_precision="round_trip")
    assert list(fp.columns) == ["Contig", "Position", "cells", "X2", "expected", "z", "deviance"] and len(fp) == V
    assert list(fp["Contig"]) == ["c%d" % (v // 100) for v in range(1, V + 1)] and np.array_equal(fp["Position"], np.arange(1, V + 1) * 3 + 1)
    assert np.array_equal(fp["z"].to_numpy(), positions["z"]) and np.array_equal(fp["cells"].to_numpy(), positions["cells"])
    fc = pd.read_csv(str(tmp_path / "Fit_cells.csv"), float_precision="round_trip")
    assert list(fc.columns) == ["Contig", "Position"] + kept and np.array_equal(fc[kept].to_numpy(), cell)
    assert np.array_equal(fc["Position"], fp["Position"])
    line = "Fit_samples.csv / Fit_positions.csv written: %d of %d samples and %d of %d positions have z > 3" % (
        int((samples["z"] > 3).sum()), S, int((positions["z"] > 3).sum()), V)
    assert caplog.text.count(line) == 1 and int((samples["z"] > 3).sum()) >= 1


def test_check_is_refused_before_any_chain(tmp_path):
    from desman_amd import cli
    Vn, Sn = 30, 3
    counts = RandomState(3).randint(20, 60, size=(Vn, Sn, 4))
    cols = ["Position"] + ["S%d-%s" % (s, b) for s in range(Sn) for b in "ACGT"]
    df = pd.DataFrame(np.concatenate([(np.arange(Vn) * 5 + 2)[:, None], counts.reshape(Vn, Sn * 4)], axis=1),
                      index=["c%d" % (v // 10) for v in range(Vn)], columns=cols)
    df.index.name = "Contig"
    freq = str(tmp_path / "t.freq")
    df.to_csv(freq)
    out = str(tmp_path / "out")
    base = [freq, "-g", "3", "-m", "0", "-o", out]
    for extra, what in ((["--check-cells"], "--check-cells needs --check"), (["-i", "0", "--check"], "at least 1 is needed"),
                        (["-i", "0", "--check", "--check-cells", "--relabel"], "at least 1 is needed")):
        for run in (cli.main, lambda argv: cli.main_replicates([argv])):
            with pytest.raises(SystemExit) as e:
                run(base + extra)
            assert "--check" in str(e.value) and what in str(e.value), (extra, e.value)
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse(base).check is False and parse(base).check_cells is False
    both = parse(base + ["--check", "--check-cells", "--relabel", "--diagnose"])
    assert both.check and both.check_cells and both.relabel and both.diagnose is True
    cli._check_options(both)
    cli._check_options(parse(base + ["--check"]))


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_fit_stats", "dsm_fit_debug_set_parts", "dsm_fit_debug_path", "dsm_ctx_debug_set_param_trace"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert all(callable(getattr(_lib.Context, m)) for m in ("trace_fit_stats", "debug_set_param_trace", "fit_debug_path"))
    assert callable(_lib.fit_debug_set_parts) and callable(HaploSNP_Sampler.fitCheck)
    assert lib.dsm_ctx_trace_fit_stats(None, 0, 0, None, None, None) == -2
    assert lib.dsm_ctx_debug_set_param_trace(None, None, None, 0) == -2 and lib.dsm_fit_debug_path(None, 1, None) == -2
    assert lib.dsm_fit_debug_set_parts(-1) == -2 and lib.dsm_fit_debug_set_parts(3) == 0 and lib.dsm_fit_debug_set_parts(0) == 0
