"""The partly held chain without a GPU: the oracle composition of tests/_heldtau.py against a direct numpy enumeration of the
conditionals, the held iteration from the oracle's pieces, the recovery case that tests/test_gpu_held_tau.py repeats on the device, and
the host logic of `desman-abund --novel` on a numpy-served context."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fixtau as F  # noqa: E402
import _heldtau as H  # noqa: E402

from desman_amd import _lib, abund, held_tau  # noqa: E402
from desman_amd.synth import synth_counts, random_state  # noqa: E402
from oracle import cbind  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enumerate_sweep(digits, gamma, eta, counts, u_free, n_held):
    """the held sweep written out: for every position and free haplotype in turn the four conditional probabilities from the full
    mixture, the CDF inverted at the step's uniform; returns (digits, steps whose uniform lies within 1e-9 of a CDF edge)"""
    d = np.array(digits, dtype=np.int64)
    V, G = d.shape
    Fr = G - n_held
    u = np.asarray(u_free).reshape(V, Fr)
    x = counts.astype(np.float32).astype(np.float64)
    close = 0
    for v in range(V):
        for g in range(Fr):
            rest = sum(gamma[:, h][:, None] * eta[d[v, h]][None, :] for h in range(G) if h != g)          # [S,4]
            logp = np.array([(x[v] * np.log(rest + gamma[:, g][:, None] * eta[a][None, :])).sum() for a in range(4)])
            p = np.exp(logp - logp.max())
            cdf = np.cumsum(p / p.sum())
            close += int(np.abs(cdf[:3] - u[v, g]).min() < 1e-9)
            d[v, g] = int(np.searchsorted(cdf[:3], u[v, g], side="right"))
    return d, close


@pytest.mark.parametrize("V,S,G,n_held", [(7, 3, 2, 1), (9, 2, 4, 2), (5, 4, 5, 4), (6, 1, 3, 1)])
def test_the_oracle_composition_is_the_enumerated_held_sweep(V, S, G, n_held):
    counts, _, _ = synth_counts(V, S, max(G, 2), seed=V)
    tau, gamma, eta = random_state(V, S, G, seed=G)
    u = np.random.default_rng(V + G).random(V * (G - n_held))
    new, n = H.held_sweep(tau, gamma, eta, counts, u, n_held)
    want, close = _enumerate_sweep(cbind.onehot_to_idx(tau), gamma, eta, counts, u, n_held)
    assert close == 0                                              # no step of these cases hangs on the last bits of a sum
    got = cbind.onehot_to_idx(new).astype(np.int64)
    assert np.array_equal(got, want)
    assert np.array_equal(new[:, G - n_held:], tau[:, G - n_held:]) and n == int((got != cbind.onehot_to_idx(tau)).sum())


def test_the_composition_does_not_read_the_held_columns_of_the_uniforms():
    V, S, G, n_held = 40, 5, 4, 2
    counts, _, _ = synth_counts(V, S, G, seed=3)
    tau, gamma, eta = random_state(V, S, G, seed=4)
    u = np.random.default_rng(5).random(V * (G - n_held))
    a, na = H.held_sweep(tau, gamma, eta, counts, u, n_held)
    full = np.random.default_rng(6).random((V, G))
    full[:, :G - n_held] = u.reshape(V, G - n_held)
    b = tau.copy()
    cbind.sample_tau_u(b, gamma, eta, counts, full.reshape(-1))
    assert np.array_equal(a[:, :G - n_held], b[:, :G - n_held]) and np.array_equal(a[:, G - n_held:], tau[:, G - n_held:])
    # the ends: nothing held is the full sweep, everything held changes nothing
    c = tau.copy()
    n_full = cbind.sample_tau_u(c, gamma, eta, counts, full.reshape(-1))
    d, nd = H.held_sweep(tau, gamma, eta, counts, full.reshape(-1), 0)
    assert np.array_equal(c, d) and nd == n_full
    e, ne = H.held_sweep(tau, gamma, eta, counts, np.zeros(0), G)
    assert np.array_equal(e, tau) and ne == 0


@pytest.mark.parametrize("fix_eta", [False, True])
@pytest.mark.parametrize("spec", [1, 2])
def test_the_restated_held_iteration(spec, fix_eta):
    """RefCtx against the pieces written out once more: with everything held it is _fixtau.ref_chain; with one haplotype free the gamma of
    iteration k comes from the mu/E sums at the state of iteration k - 1 and the sweep reads (new gamma, previous eta)"""
    V, S, G, n = 60, 4, 3, 3
    counts, _, _ = synth_counts(V, S, G, seed=21)
    tau, gamma, eta = random_state(V, S, G, seed=22)
    cseed = 0xC0FFEE

    def run(n_held):
        c = H.RefCtx()
        c.spec = spec
        c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(77, ctr_seed=cseed)
        c.gibbs_update_held_tau(n, n_held, fix_eta=fix_eta)
        return c
    c = run(G)
    ref = F.ref_chain(cbind.onehot_to_idx(tau), gamma, eta, counts, cseed, 0, n, spec, fix_eta)
    for key in ("gamma", "eta", "ll", "lp"):
        assert np.array_equal(c.get_trace()[key], ref[key]), key
    assert not c.get_trace()["nchange"].any() and np.array_equal(c.tau, tau)
    c = run(1)
    tr, mt = c.get_trace(), cbind.MT19937(77)
    t_prev, g_prev, e_prev = tau, gamma, eta
    for k in range(n):
        mu, E = F.stats(spec, cbind.onehot_to_idx(t_prev), g_prev, e_prev, counts, cseed, k)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, k)
        assert np.array_equal(tr["gamma"][k], g_ref) and np.array_equal(tr["eta"][k], eta if fix_eta else e_ref)
        t_ref, n_ref = H.held_sweep(t_prev, g_ref, e_prev, counts, mt.uniform(V * (G - 1)), 1)
        assert np.array_equal(tr["tau"][k], t_ref) and tr["nchange"][k] == n_ref and np.array_equal(t_ref[:, G - 1], tau[:, G - 1])
        t_prev, g_prev, e_prev = t_ref, np.ascontiguousarray(tr["gamma"][k]), np.ascontiguousarray(tr["eta"][k])
    assert c.get_star()["lp"] == max([cbind.logpost(cbind.onehot_to_idx(tau), gamma, eta, counts)] + list(tr["lp"]))


def test_the_restatement_recovers_the_free_strain():
    """the recovery case of tests/test_gpu_held_tau.py, on the restatement: 60 iterations, two true strains held, the free MAP
    haplotype equals the third strain in all 300 of 300 positions (measured; the GPU test asks for 285)"""
    res, third = H.recovery_run(H.RefCtx)
    same = int((res["tau_star"][:, 0] == third).sum())
    print("restatement: free MAP haplotype equals the third strain in %d of %d positions" % (same, len(third)))
    assert same >= 285
    assert np.array_equal(res["tau_star"][:, 1:], H.recovery_case()[1][:, 1:])


# ---- the host logic of `desman-abund --novel` ---------------------------------------------------------------------------------------
def test_novel_start_and_column_order():
    V, S, G, K = 50, 3, 2, 2
    counts, tau, _ = synth_counts(V, S, G, seed=9)
    counts[3] = 0                                                  # a position without reads: all four bases are candidates
    counts[4] = 0; counts[4, 1, 2] = 5                             # one base seen: the free digits must be it
    held = tau.astype(np.int64)
    start = held_tau.novel_start(counts, held, K, 0x1234567890)
    assert start.shape == (V, G + K) and np.array_equal(start[:, K:], held) and (start[4, :K] == 2).all()
    seen = counts.sum(axis=1) > 0
    assert all(seen[v, start[v, k]] for v in range(V) for k in range(K) if seen[v].any())
    assert np.array_equal(start, held_tau.novel_start(counts, held, K, 0x1234567890))
    assert np.array_equal(start, held_tau.novel_start(counts, held, K, 0x34567890))            # the seed modulo 2^32
    assert not np.array_equal(start, held_tau.novel_start(counts, held, K, 7))
    assert held_tau.novel_labels(G, K) == ["novel0", "novel1", "0", "1"]
    for bad in (0, 31):
        with pytest.raises(ValueError):
            held_tau.novel_start(counts, held, bad, 1)
    with pytest.raises(ValueError):
        held_tau.novel_chain(counts, held, np.eye(4), 1, n_iter=5, burn=5, context=H.RefCtx)


def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    df = pd.DataFrame(np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1), index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_the_novel_writers_on_a_numpy_served_context(tmp_path):
    V, S, G, K = 80, 3, 2, 1
    counts, tau, _ = synth_counts(V, S, G + K, seed=12)
    held = tau[:, 1:].astype(np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    novel = held_tau.novel_chain(counts, held, eta, K, n_iter=12, burn=4, seed=99, context=H.RefCtx)
    assert novel["draws"].shape == (8, S, G + K) and len(novel["ll"]) == 8 and np.array_equal(novel["tau_star"][:, K:], held)
    base = dict(ll=np.array([-10.0, -12.0]), lp_star=-9.0)
    names, contigs, positions = ["N0", "N1", "N2"], ["c%d" % (v // 30) for v in range(V)], np.arange(V) * 3 + 1
    out = str(tmp_path / "out")
    held_tau.write_novel(out, names, contigs, positions, base, novel, K)
    assert sorted(os.listdir(out)) == ["Novel_Gamma_posterior.csv", "Novel_Gamma_star.csv", "Novel_Tau_star.csv", "Novel_fit.csv", "Novel_haplotypes.csv"]
    t = pd.read_csv(os.path.join(out, "Novel_Tau_star.csv"), header=0, index_col=0)
    assert list(t.index) == contigs and list(t.columns) == ["Position"] + [str(i) for i in range(4 * (G + K))]
    onehot = t.to_numpy()[:, 1:].reshape(V, G + K, 4)
    assert np.array_equal(np.argmax(onehot, axis=2), novel["tau_star"]) and (onehot.sum(axis=2) == 1).all()
    assert np.array_equal(t["Position"].to_numpy(), positions)
    rt = dict(index_col=0, float_precision="round_trip")
    g = pd.read_csv(os.path.join(out, "Novel_Gamma_star.csv"), **rt)
    assert list(g.columns) == ["novel0", "0", "1"] and list(g.index) == names and np.array_equal(g.to_numpy(), novel["gamma_star"])
    p = pd.read_csv(os.path.join(out, "Novel_Gamma_posterior.csv"), **rt)
    assert list(p.columns) == ["%s_%s" % (lab, k) for lab in ("novel0", "0", "1") for k in ("mean", "sd", "lo", "med", "hi")]
    assert np.array_equal(p["novel0_mean"].to_numpy(), novel["mean"][:, 0])
    f = pd.read_csv(os.path.join(out, "Novel_fit.csv"), **rt)
    assert list(f.index) == [0, K] and list(f.columns) == ["deviance", "lp_star", "iters"]
    assert f.loc[0, "deviance"] == 22.0 and f.loc[0, "iters"] == 2 and f.loc[K, "deviance"] == -2.0 * novel["ll"].mean() and f.loc[K, "lp_star"] == novel["lp_star"]
    h = pd.read_csv(os.path.join(out, "Novel_haplotypes.csv"), **rt)
    d = [(novel["tau_star"][:, 0] != held[:, j]).sum() for j in range(G)]
    assert list(h.index) == ["novel0"] and h.loc["novel0", "distance"] == min(d) and str(h.loc["novel0", "nearest"]) == str(int(np.argmin(d)))
    assert h.loc["novel0", "mean_abundance"] == novel["mean"][:, 0].mean() and h.loc["novel0", "max_abundance"] == novel["mean"][:, 0].max()
    # a free haplotype that copies a held one is shown at distance 0
    over = dict(novel, tau_star=np.concatenate([held[:, 1:2], held], axis=1))
    assert held_tau.haplotype_rows(over, K).loc["novel0", "distance"] == 0 and held_tau.haplotype_rows(over, K).loc["novel0", "nearest"] == "1"


def test_novel_refusals_come_before_the_library(tmp_path):
    V, S, G = 30, 2, 2
    counts, tau, _ = synth_counts(V, S, G, seed=14)
    run = tmp_path / "run"
    run.mkdir()
    contigs, positions = ["c0"] * V, np.arange(V) + 1
    pd.DataFrame(0.96 * np.eye(4) + 0.01).to_csv(run / "Eta_star.csv")
    frame = pd.DataFrame(held_tau.onehot(tau.astype(np.int64)).reshape(V, -1), index=contigs)
    frame.insert(0, "Position", positions)
    frame.to_csv(run / "Filtered_Tau_star.csv")
    table = str(tmp_path / "new.freq")
    _write_freq(table, counts, ["N0", "N1"], contigs, positions)
    for argv, word in ((["--novel", "0"], "K >= 1"), (["--novel", "31"], "more than 32"), (["--novel", "1", "--burn", "1000"], "--burn"),
                       (["--novel", "1", "--posterior", "10", "--burn", "10"], "--burn")):
        with pytest.raises(SystemExit) as e:
            abund.main([str(run), table, "-o", str(tmp_path / "o")] + argv)
        assert word in str(e.value), (argv, e.value)
    assert not os.path.exists(str(tmp_path / "o"))
    # the held haplotypes and their alignment are those of --posterior: the model's positions, matched by (contig, Position)
    c2, p2, digits, _ = abund.load_model(str(run))
    assert np.array_equal(digits, tau) and list(p2) == list(positions) and c2 == contigs


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "desman_hip.h")).read()
    api = open(os.path.join(ROOT, "desman_amd", "csrc", "api.hip")).read()
    for name in ("dsm_ctx_sample_tau_held", "dsm_ctx_gibbs_update_held_tau"):
        assert re.search(r"\bint %s\(" % name, header) and re.search(r'extern "C" int %s\(' % name, api) and name in _lib.SIGNATURES
    assert all(callable(getattr(_lib.Context, m)) for m in ("sample_tau_held", "gibbs_update_held_tau"))
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    assert callable(HaploSNP_Sampler.update_held)
    assert "kernels_heldtau.hip" in open(os.path.join(ROOT, "desman_amd", "csrc", "Makefile")).read()
