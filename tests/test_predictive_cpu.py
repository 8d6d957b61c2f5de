"""Host side of the predictive model comparison (desman_amd/predictive.py) without a GPU: the numpy reference the
GPU tests compare against (tests/_predictive_ref.py) on a hand-worked case, the host arithmetic with its infinity rules, `compare`,
the C interface's declarations and the command line's refusals.  The device side is tests/test_gpu_predictive.py."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

import _predictive_ref as ref
from desman_amd import _lib, predictive
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler


def test_reference_on_a_hand_worked_case():
    # G = 1, S = 1, uniform eta: every one of the four states gives each read probability 1/4, so logz = ln 4 + N ln(1/4)
    counts = np.array([[[3, 0, 2, 1]]])
    gamma, eta = np.ones((2, 1, 1)), np.full((2, 4, 4), 0.25)
    r = ref.trace_predictive(counts, gamma, eta)
    want = math.log(4.0) + 6 * math.log(0.25)
    assert r["logz_it"].shape == (2, 1) and np.allclose(r["logz_it"], want, rtol=1e-15)
    assert r["lppd"][0] == pytest.approx(want, rel=1e-15) and r["mean"][0] == pytest.approx(want, rel=1e-15) and r["var"][0] == 0.0
    # a position without reads: every state has L = 0, logz = G ln 4
    g2 = np.random.RandomState(1).dirichlet(np.ones(3), size=(1, 2))
    r = ref.trace_predictive(np.zeros((1, 2, 4), dtype=np.int64), g2, eta[:1])
    assert r["logz_it"][0, 0] == pytest.approx(3 * math.log(4.0), rel=1e-15) and r["var"][0] == 0.0
    # G = 2 by hand: one sample of haplotype 0 alone under the identity eta sees base A -> the 4 states (A, *) have L = 0, the others -inf
    r = ref.trace_predictive(np.array([[[5, 0, 0, 0]]]), np.array([[[1.0, 0.0]]]), np.eye(4)[None])
    assert r["logz_it"][0, 0] == pytest.approx(math.log(4.0), rel=1e-15)
    assert np.array_equal(ref.states(2)[:5], [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0]])
    # the infinity rules of the statistics
    lppd, mean, var = ref.stats(np.array([[-1.0, -np.inf, -2.0], [-np.inf, -np.inf, -4.0]]))
    assert lppd[0] == pytest.approx(-1.0 + math.log(0.5)) and lppd[1] == -np.inf and lppd[2] == pytest.approx(np.log((np.exp(-2) + np.exp(-4)) / 2))
    assert list(mean[:2]) == [-np.inf, -np.inf] and list(var[:2]) == [np.inf, np.inf] and mean[2] == -3.0 and var[2] == 2.0


def test_log_multinomial_against_comb():
    rs = np.random.RandomState(5)
    counts = rs.randint(0, 9, size=(6, 3, 4))
    counts[1] = 0
    want = np.zeros(6)
    for v in range(6):
        for s in range(3):
            a, c, g, t = (int(x) for x in counts[v, s])
            want[v] += math.log(math.comb(a + c + g + t, a) * math.comb(c + g + t, c) * math.comb(g + t, g))
    got = predictive.log_multinomial(counts)
    assert got.shape == (6,) and np.allclose(got, want, rtol=1e-13, atol=1e-13) and got[1] == 0.0
    assert predictive.log_multinomial(np.zeros((0, 3, 4), dtype=np.int64)).shape == (0,)
    with pytest.raises(ValueError):
        predictive.log_multinomial(np.zeros((3, 4)))


def test_pointwise_and_summary_arithmetic():
    counts = np.array([[[2, 1, 0, 0]], [[0, 0, 0, 0]], [[1, 1, 1, 1]], [[4, 0, 0, 0]]])
    G = 3
    res = dict(lppd=np.array([-3.0, 1.0, -np.inf, -7.0]), mean=np.array([-3.5, 0.9, -np.inf, -np.inf]),
               var=np.array([0.5, 0.0, np.inf, np.inf]), n_used=9)
    pw = predictive.pointwise(res, counts, G)
    const = np.array([math.log(3.0), 0.0, math.log(24.0), 0.0]) - G * math.log(4.0)
    assert np.allclose(pw["lppd"][[0, 1, 3]], np.array([-3.0, 1.0, -7.0]) + const[[0, 1, 3]], rtol=1e-15) and pw["lppd"][2] == -np.inf
    assert np.array_equal(pw["p_waic"], res["var"]) and pw["n_iterations"] == 9
    assert pw["elpd_waic"][0] == pw["lppd"][0] - 0.5 and pw["elpd_waic"][1] == pw["lppd"][1]
    assert pw["elpd_waic"][2] == -np.inf and pw["elpd_waic"][3] == -np.inf
    assert not any(np.isnan(pw[k]).any() for k in ("lppd", "p_waic", "elpd_waic"))
    s = predictive.summary(pw)
    assert s["n_positions"] == 4 and s["n_iterations"] == 9 and s["n_high_var"] == 3
    assert s["lppd"] == -np.inf and s["elpd_waic"] == -np.inf and s["p_waic"] == np.inf
    assert s["se_lppd"] == np.inf and s["se_elpd_waic"] == np.inf and not any(isinstance(v, float) and math.isnan(v) for v in s.values())
    # all finite: plain sums and sqrt(V Var_v)
    fin = dict(lppd=np.array([-3.0, -1.0, -2.5]), p_waic=np.array([0.1, 0.5, 0.4]), n_iterations=4)
    fin["elpd_waic"] = fin["lppd"] - fin["p_waic"]
    s = predictive.summary(fin)
    assert s["lppd"] == pytest.approx(-6.5) and s["p_waic"] == pytest.approx(1.0) and s["elpd_waic"] == pytest.approx(-7.5)
    assert s["se_elpd_waic"] == pytest.approx(math.sqrt(3 * np.var(fin["elpd_waic"], ddof=1)))
    assert s["se_lppd"] == pytest.approx(math.sqrt(3 * np.var(fin["lppd"], ddof=1))) and s["n_high_var"] == 1      # 0.4 itself is not above
    assert predictive.P_WAIC_HIGH == 0.4 and predictive.N_USE == 50
    row = predictive.summary_row("fit", s)
    assert [row[c] for c in predictive.SUMMARY_COLUMNS] == ["fit", 3, 4, s["elpd_waic"], s["se_elpd_waic"], s["p_waic"], 1]
    row = predictive.summary_row("heldout", s)
    assert [row[c] for c in predictive.SUMMARY_COLUMNS] == ["heldout", 3, 4, s["lppd"], s["se_lppd"], "", ""]
    one = predictive.summary(dict(lppd=np.array([-2.0]), p_waic=np.array([0.0]), elpd_waic=np.array([-2.0]), n_iterations=1))
    assert one["se_lppd"] == np.inf and one["lppd"] == -2.0
    none = predictive.summary(dict(lppd=np.zeros(0), p_waic=np.zeros(0), elpd_waic=np.zeros(0), n_iterations=1))
    assert none["se_lppd"] == 0.0 and none["lppd"] == 0.0 and none["n_positions"] == 0


def _run_dir(path, G, fit, heldout, drop=None):
    os.makedirs(path)
    pd.DataFrame(np.full((2, G), 1.0 / G), index=["s0", "s1"]).to_csv(os.path.join(path, "Gamma_star.csv"))
    rows = []
    for kind, col in (("fit", fit), ("heldout", heldout)):
        for v, e in enumerate(col):
            rows.append(dict(Contig="c%d" % (v // 2), Position=10 + v, kind=kind, lppd=e + (0.25 if kind == "fit" else 0.0),
                             p_waic=0.25 if kind == "fit" else np.nan, elpd_waic=e))
    frame = pd.DataFrame(rows, columns=list(predictive.POSITION_COLUMNS))
    if drop is not None:
        frame = frame.drop(index=drop)
    frame.to_csv(os.path.join(path, predictive.POSITIONS_FILE), index=False)
    return path


def test_compare_orders_pairs_and_refuses(tmp_path, capsys):
    fit = {2: [-9.0, -8.0, -9.5], 3: [-7.0, -7.5, -7.25], 4: [-6.0, -6.5, -6.25]}          # the fitted rows favour G = 4 ...
    held = {2: [-10.0, -12.0, -11.0, -13.0], 3: [-8.0, -9.0, -8.5, -9.5], 4: [-8.5, -9.0, -8.0, -10.5]}     # ... the held-out ones G = 3
    d = {G: _run_dir(str(tmp_path / ("g%d" % G)), G, fit[G], held[G]) for G in (2, 3, 4)}
    rows = predictive.compare([d[2], d[4], d[3]])
    assert [r["G"] for r in rows] == [3, 4, 2] and [r["run"] for r in rows] == [d[3], d[4], d[2]]
    assert all(r["kind"] == "heldout" and r["n_positions"] == 4 for r in rows)
    assert [r["elpd"] for r in rows] == [-35.0, -36.0, -46.0] and [r["elpd_diff"] for r in rows] == [0.0, -1.0, -11.0]
    for r in rows[1:]:
        diff = np.array(held[r["G"]]) - np.array(held[3])
        assert r["se_diff"] == pytest.approx(math.sqrt(4 * np.var(diff, ddof=1)), rel=1e-14)
    assert rows[0]["se_diff"] == 0.0
    rows = predictive.compare([d[2], d[3], d[4]], kind="fit")
    assert [r["G"] for r in rows] == [4, 3, 2] and rows[1]["elpd_diff"] == pytest.approx(-3.0)      # -21.75 + 18.75
    assert rows[2]["se_diff"] == pytest.approx(math.sqrt(3 * np.var(np.array(fit[2]) - np.array(fit[4]), ddof=1)))
    # rows in another order pair by key, not by line
    shuffled = str(tmp_path / "g3s")
    _run_dir(shuffled, 3, fit[3], held[3])
    path = os.path.join(shuffled, predictive.POSITIONS_FILE)
    pd.read_csv(path).iloc[::-1].to_csv(path, index=False)
    again = predictive.compare([d[2], shuffled, d[4]])
    assert [(r["G"], r["elpd"], r["elpd_diff"]) for r in again] == [(3, -35.0, 0.0), (4, -36.0, -1.0), (2, -46.0, -11.0)]
    # a run that lacks a row, or has another one, is refused with that row named
    short = _run_dir(str(tmp_path / "short"), 4, fit[4], held[4], drop=4)
    with pytest.raises(ValueError, match=r"do not score the same positions: \(c0, 11, heldout\) is only in %s" % re.escape(d[2])):
        predictive.compare([d[2], d[3], short])
    with pytest.raises(ValueError, match=r"\(c0, 11, heldout\) is only in %s" % re.escape(d[3])):
        predictive.compare([short, d[3]])
    with pytest.raises(ValueError, match="no Predictive_positions.csv"):
        predictive.compare([d[2], str(tmp_path)])
    # the command line: the table as CSV, printed or written
    predictive.main(["compare", d[2], d[3], d[4]])
    text = capsys.readouterr().out
    assert text.splitlines()[0] == "run,G,kind,n_positions,elpd,elpd_diff,se_diff" and text.splitlines()[1].startswith(d[3] + ",3,heldout,4,-35.0,0.0,0.0")
    out = str(tmp_path / "cmp.csv")
    predictive.main(["compare", d[2], d[3], d[4], "-o", out])
    assert open(out).read() == text and not capsys.readouterr().out
    with pytest.raises(SystemExit, match="do not score the same positions"):
        predictive.main(["compare", d[2], short])


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_predictive", "dsm_pred_debug_set_chunk", "dsm_pred_debug_set_parts"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.Context.trace_predictive) and callable(_lib.pred_debug_set_chunk) and callable(_lib.pred_debug_set_parts)
    assert callable(HaploSNP_Sampler.predictive)
    assert lib.dsm_ctx_trace_predictive(None, None, 0, 0, 0, 1, None, None, None, None) == -2
    assert lib.dsm_pred_debug_set_chunk(-1) == -2 and lib.dsm_pred_debug_set_chunk(3) == 0 and lib.dsm_pred_debug_set_chunk(0) == 0
    assert lib.dsm_pred_debug_set_parts(-1) == -2 and lib.dsm_pred_debug_set_parts(2) == 0 and lib.dsm_pred_debug_set_parts(0) == 0
    assert predictive.MAX_G == _lib.ASSIGN_MAX_G


def test_predictive_is_refused_before_any_chain(tmp_path):
    from desman_amd import cli
    out = str(tmp_path / "out")
    freq = str(tmp_path / "never_read.freq")                   # the file does not exist: a run that got as far as loading would say so
    for argv, what in (([freq, "--predictive", "-g", "11", "-o", out], "-g 11 is above 10"),
                       ([freq, "-g", "3", "-o", out, "--predictive", "0"], "at least 1 stored iteration must be used; got 0"),
                       ([freq, "-g", "3", "-o", out, "--predictive", "-2"], "got -2"),
                       ([freq, "-g", "3", "-o", out, "-i", "0", "--predictive"], "at least 1 is needed")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--predictive" in str(e.value) and what in str(e.value), (argv, e.value)
    # replicate chains that share their launches do not serve the option: refused up front as well
    with pytest.raises(SystemExit, match="--predictive is not available for replicate chains"):
        cli.main_replicates([[freq, "-g", "3", "-o", out, "--predictive"]])
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse([freq, "-g", "3"]).predictive is None and parse([freq, "-g", "3", "--predictive"]).predictive == 50
    assert parse([freq, "-g", "10", "--predictive", "7"]).predictive == 7
    cli._predictive_options(parse([freq, "-g", "10", "--predictive", "7", "--check", "--relabel"]))
