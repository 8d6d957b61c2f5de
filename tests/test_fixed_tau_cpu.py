"""CPU side of the fixed-tau chain: the numpy pooling helper, the command line and the CSV writers of `desman-abund --posterior`, and
the conditions of the GPU law and posterior tests checked for the oracle's restatement with the same seeds."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402
import _fixtau as F  # noqa: E402

from desman_amd import _lib, abund, fixed_tau  # noqa: E402
from oracle import cbind  # noqa: E402


# ---- the pooling helper --------------------------------------------------------------------------------------------------------------
def test_pooling_adds_the_counts_of_equal_words_in_ascending_word_order():
    tau = np.array([[3, 0], [1, 2], [3, 0], [0, 0], [1, 2], [3, 0]])
    counts = np.arange(6 * 2 * 4, dtype=np.int64).reshape(6, 2, 4)
    words, row, pooled = fixed_tau.pool_by_tau_word(tau, counts)
    assert words.tolist() == [0, 3, 9] and words.dtype == np.uint64             # digit of haplotype g in bits 2g, 2g + 1
    assert row.tolist() == [1, 2, 1, 0, 2, 1]
    assert np.array_equal(pooled[0], counts[3]) and np.array_equal(pooled[1], counts[0] + counts[2] + counts[5]) \
        and np.array_equal(pooled[2], counts[1] + counts[4])
    assert np.array_equal(fixed_tau.words_to_digits(words, 2), [[0, 0], [3, 0], [1, 2]])
    onehot = cbind.idx_to_onehot(tau)
    assert np.array_equal(fixed_tau.tau_words(onehot), fixed_tau.tau_words(tau))


def test_pooling_a_table_of_distinct_words_and_a_table_of_one_word():
    rng = np.random.default_rng(3)
    V, S, G = 64, 2, 8
    tau = fixed_tau.words_to_digits(rng.permutation(4 ** G)[:V].astype(np.uint64), G)
    counts = rng.integers(0, 50, size=(V, S, 4))
    words, row, pooled = fixed_tau.pool_by_tau_word(tau, counts)
    assert len(words) == V and (np.diff(words.astype(np.int64)) > 0).all() and np.array_equal(pooled[row], counts)
    one = np.tile(tau[:1], (V, 1))
    words, row, pooled = fixed_tau.pool_by_tau_word(one, counts)
    assert len(words) == 1 and not row.any() and np.array_equal(pooled[0], counts.sum(axis=0))
    words, row, pooled = fixed_tau.pool_by_tau_word(tau[:1], counts[:1])
    assert len(words) == 1 and np.array_equal(pooled, counts[:1])


def test_the_pooled_table_has_the_likelihood_of_the_original_up_to_the_coefficients():
    counts, tau, gamma, eta = F.law_case()
    digits, pooled = F.pooled_table(tau, counts)
    K = cbind.loglik_const(counts) - cbind.loglik_const(pooled)
    a, b = cbind.loglik(tau, gamma, eta, counts), cbind.loglik(digits, gamma, eta, pooled)
    scale = max(abs(a), abs(cbind.loglik_const(counts)), abs(cbind.loglik_const(pooled)))
    assert len(digits) <= 64 and abs(a - (b + K)) <= 1e-12 * scale


# ---- the conditions of the GPU tests, for the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [2, 1])
def test_pooling_keeps_the_law_of_the_sums_for_the_oracle(spec):
    """tests/test_gpu_fixed_tau.py test 4 with the oracle's sampler in the device's place: the means of 400 draws of sum_mu and Esum ON
    THE POOLED table lie within 5 standard errors of their exact expectations ON THE ORIGINAL table"""
    counts, tau, gamma, eta = F.law_case()
    digits, pooled = F.pooled_table(tau, counts)
    draws = [F.stats(spec, digits, gamma, eta, pooled, F.LAW_SEED, it) for it in range(F.LAW_N)]
    bad = F.law_violations([d[0] for d in draws], [d[1] for d in draws], F.sum_moments(tau, gamma, eta, counts))
    assert not bad, bad


def test_posterior_conditions_hold_for_the_restated_chain():
    """tests/test_gpu_fixed_tau.py test 5 with the loop restated from the oracle's pieces (per-read mu/E pass: what the shape rule picks
    at 300 x 4 x 3 and on its pooled table), same table, start, stream key and iterations, on the original and on the pooled table"""
    counts, tau, eta = F.posterior_case()
    V, S, G = F.POST_SHAPE
    ml = R.fit_samples(counts, tau, eta, tol=1e-9, max_iter=20000)
    ml_gamma = np.asarray(ml["gamma"] if isinstance(ml, dict) else ml[0])
    posts = []
    for t, x in ((tau.astype(np.uint8), counts), F.pooled_table(tau, counts)):
        ch = F.ref_chain(t, np.full((S, G), 1.0 / G), eta, x, F.POST_SEED, 0, F.POST_N, 1, True, want_ll=False)
        post = fixed_tau.summarize(ch["gamma"][F.POST_BURN:], 0.95)
        assert not F.posterior_violations(post, ml_gamma)
        posts.append(post)
    assert not F.means_disagree(posts[0], posts[1]).any()


# ---- summaries, command line, writers ---------------------------------------------------------------------------------------------------
def test_summarize_gives_moments_and_ordered_quantiles():
    d = np.arange(11.0)[:, None, None] * np.array([[1.0, 2.0]])
    s = fixed_tau.summarize(d, 0.8)
    assert np.allclose(s["mean"], [[5.0, 10.0]]) and np.allclose(s["med"], [[5.0, 10.0]]) and np.allclose(s["lo"], [[1.0, 2.0]]) \
        and np.allclose(s["hi"], [[9.0, 18.0]]) and np.allclose(s["sd"], [[np.std(np.arange(11.0), ddof=1)] * 1 + [2 * np.std(np.arange(11.0), ddof=1)]])
    assert fixed_tau.summarize(d[:1])["sd"].tolist() == [[0.0, 0.0]]
    with pytest.raises(ValueError):
        fixed_tau.summarize(d[:0])
    with pytest.raises(ValueError):
        fixed_tau.summarize(d, 1.0)


def test_posterior_flags_parse():
    ap = abund.build_parser()
    o = ap.parse_args(["run", "t.freq"])
    assert o.posterior is None and o.burn == abund.POSTERIOR_BURN == 200 and o.posterior_seed == abund.POSTERIOR_SEED == fixed_tau.POSTERIOR_SEED
    o = ap.parse_args(["run", "t.freq", "--posterior"])
    assert o.posterior == abund.POSTERIOR_N == 1000
    o = ap.parse_args(["run", "t.freq", "--posterior", "300", "--burn", "50", "--posterior-seed", "0x10", "--fit-eta", "--interval", "0.9"])
    assert (o.posterior, o.burn, o.posterior_seed, o.fit_eta, o.interval) == (300, 50, 16, True, 0.9)
    with pytest.raises(SystemExit):
        ap.parse_args(["run", "t.freq", "--posterior", "many"])


@pytest.mark.parametrize("argv", [["--posterior", "100", "--burn", "100"], ["--posterior", "0"], ["--posterior", "10", "--burn", "-1"]])
def test_bad_posterior_lengths_end_the_call_before_anything_is_read(argv, tmp_path):
    with pytest.raises(SystemExit) as e:
        abund.main([str(tmp_path / "no_run"), str(tmp_path / "no.freq")] + argv)
    assert "--posterior" in str(e.value)


def test_posterior_writers(tmp_path):
    rng = np.random.default_rng(1)
    draws = rng.dirichlet(np.ones(3), size=(40, 2))
    post = fixed_tau.summarize(draws, 0.9)
    abund.write_posterior(str(tmp_path), ["N0", "N1"], post)
    t = pd.read_csv(tmp_path / "Projected_posterior.csv", index_col=0, float_precision="round_trip")
    assert list(t.index) == ["N0", "N1"]
    assert list(t.columns) == ["%d_%s" % (g, k) for g in range(3) for k in ("mean", "sd", "lo", "med", "hi")]
    for g in range(3):
        for k in ("mean", "sd", "lo", "med", "hi"):
            assert np.array_equal(t["%d_%s" % (g, k)].to_numpy(), post[k][:, g])
    e = fixed_tau.summarize(rng.dirichlet(np.ones(4), size=(40, 4)))
    abund.write_eta_posterior(str(tmp_path), dict(eta_mean=e["mean"], eta_sd=e["sd"]))
    t = pd.read_csv(tmp_path / "Projected_Eta_posterior.csv", index_col=0, float_precision="round_trip")
    assert t.shape == (4, 8) and np.array_equal(t[["%d_mean" % b for b in range(4)]].to_numpy(), e["mean"]) \
        and np.array_equal(t[["%d_sd" % b for b in range(4)]].to_numpy(), e["sd"])
    assert np.allclose(t[["%d_mean" % b for b in range(4)]].to_numpy().sum(axis=1), 1.0, atol=1e-12)


# ---- the interface exists ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_fixed_tau_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_gibbs_update_fixed_tau", "dsm_ctx_debug_fixtau_pool", "dsm_ctx_debug_fixtau_sample_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.Context.gibbs_update_fixed_tau) and callable(_lib.Context.debug_fixtau_pool)
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    assert callable(HaploSNP_Sampler.update_fixed_tau) and callable(HaploSNP_Sampler.posteriorGamma)
    assert "update_fixed_tau" not in open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "desman_amd", "HaploSNP_Sampler.py")).read().split("Not mirrored")[1].split('"""')[0]


def test_bad_arguments_come_back_as_error_codes_without_a_device():
    lib = _lib.load()
    assert lib.dsm_ctx_gibbs_update_fixed_tau(None, -1, 0, 0) == -2
    assert lib.dsm_ctx_gibbs_update_fixed_tau(None, 1, 0, 2) == -2
    assert lib.dsm_ctx_gibbs_update_fixed_tau(None, 1, 0, 0) == -2                # null context (dsm_ctx_need())
