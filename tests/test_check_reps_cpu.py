"""`desman --check --check-reps` without a device: the numpy restatement of dsm_ctx_trace_ppc (tests/_ppc_ref.py) is calibrated and has
power on its own, before tests/test_gpu_check_reps.py relies on it; the helpers of desman_amd/check.py; the refusals at the command line
and in the sampler before any device work; the new symbols."""
import inspect
import os
import re

import numpy as np
import pytest

import _ppc_ref as ref
from desman_amd import _lib, check


@pytest.fixture(scope="module")
def cases():
    """the restatement's results on the known-parameter table and on its spoiled copy: computed once, read by the tests below"""
    out = {}
    for spoiled in (False, True):
        counts, digits, gamma, eta = ref.known_case(spoiled=spoiled)
        out[spoiled] = ref.ppc(counts, digits, gamma, eta, [0], ref.CASE_R, ref.CASE_KEY, rng=np.random.default_rng(ref.CASE_SEED + 1))
    return out


def test_known_parameters_give_uniform_position_p_values(cases):
    """(a) V = 2000, S = 6, G = 3, 200 .. 499 reads per cell, the table drawn from the model at the parameters the check is run at, one
    iteration, R = 100.  The ten-bin chi-square of the position p-values stays below its 1 - 1e-6 quantile and the share below 0.05 lies
    in the exact binomial band (1 - 1e-6) around 5 / 101.  At ref.CASE_SEED the restatement gives a chi-square p-value of 0.60 and a
    share of 0.0495 in the band 0.0275 .. 0.0750."""
    pv, share, lo, hi = ref.calibration_figures(cases[False]["ge_position"], ref.CASE_R)
    print("ten-bin chi-square p-value %.3g; share below 0.05: %.4f, band %.4f .. %.4f" % (pv, share, lo, hi))
    assert pv > 1e-6 and lo <= share <= hi
    assert pv > 0.01                                             # the room the seed was chosen for


def test_a_spoiled_sample_is_found_and_no_other(cases):
    """(b) the same table with sample 2's A and C counts swapped at every tenth position: that sample gets p < 0.01, every other sample
    p > 0.05.  At ref.CASE_SEED the restatement gives p = 0 for it and 0.35 .. 0.96 for the others."""
    p = cases[True]["ge_sample"] / float(ref.CASE_R)
    print("sample p-values, spoiled:", p, "unspoiled:", cases[False]["ge_sample"] / float(ref.CASE_R))
    assert p[ref.SPOILED] < 0.01 and (np.delete(p, ref.SPOILED) > 0.05).all()
    assert (np.delete(p, ref.SPOILED) > 0.15).all()              # the room the seed was chosen for


def test_observed_side_is_check_cell_terms(cases):
    counts, digits, gamma, eta = ref.known_case()
    terms = check.cell_terms(counts, digits[0], gamma[0], eta[0])
    assert np.array_equal(ref.pearson(counts, ref.cell_p(digits[0], gamma[0], eta[0])), terms["X"])
    assert np.allclose(cases[False]["obs_sample"], terms["X"].sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(cases[False]["obs_position"], terms["X"].sum(axis=1), rtol=1e-12, atol=0)
    # the replicates reproduce the exact mean of X: |z| < 5 with the standard error from the exact W.  Per sample only: T_s adds 2000
    # cells and its mean over 100 replicates is normal; T_v adds 6 cells whose rare bases (p = 0.01, three expected reads) are strongly
    # skewed, and a normal bound on 2000 such means of 100 is not exact enough (this seed's largest is 5.67)
    for kind, axis in (("sample", 0),):
        E, W = terms["E"].sum(axis=axis), terms["W"].sum(axis=axis)
        z = (cases[False]["rep_" + kind][:, 0] / ref.CASE_R - E) / np.sqrt(W / ref.CASE_R)
        assert (np.abs(z) < 5).all(), (kind, float(np.abs(z).max()))


def test_read_by_read_draws_follow_the_rule():
    """thresholds by the read loop's rule; a base with p = 0 is never drawn, the last base with p > 0 takes the remainder; the draw of a
    cell depends on (key, v, s, t, r) alone"""
    p = np.array([[[0.25, 0.25, 0.5, 0.0], [0.0, 1.0, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4], [0.0, 0.0, 0.0, 0.0]]])
    th, c3 = ref.thresholds(p)
    assert th[0, 0].tolist() == [1 << 30, 1 << 31, 4294967295] and th[0, 1].tolist() == [0, 4294967295, 4294967295] and c3[0, 3] == 0
    N = np.array([[100, 128, 77, 5]])
    x = ref.draw_replicate(N, p, 99, 3, 1)
    assert x[0, 0, 3] == 0 and x[0, 0].sum() == 100 and x[0, 1].tolist() == [0, 128, 0, 0] and x[0, 2].sum() == 77 and (x[0, 3] == 0).all()
    wide = ref.draw_replicate(np.array([[100, 128, 77, 5], [1, 2, 3, 4]]), np.concatenate([p, p]), 99, 3, 1)
    assert np.array_equal(wide[0], x[0]) and not np.array_equal(ref.draw_replicate(N, p, 99, 3, 2)[0, 2], x[0, 2])
    assert not np.array_equal(ref.draw_replicate(N, p, 98, 3, 1)[0, 2], x[0, 2])
    with pytest.raises(AssertionError):
        ref.draw_replicate(np.array([[129]]), p[:, :1], 99, 0, 0)


def test_sums_run_in_the_stated_order():
    rs = np.random.RandomState(5)
    for V, S in ((70, 5), (9, 130), (300, 64)):
        X = rs.random_sample((V, S)) * 10.0 ** rs.randint(-8, 8, size=(V, S))
        assert np.allclose(ref.sum_over_samples(X), X.sum(axis=1), rtol=1e-12) and np.allclose(ref.sum_over_positions(X), X.sum(axis=0), rtol=1e-12)
    assert [ref.tiling(S) for S in (1, 2, 5, 20, 40, 64, 65, 130, 300, 512)] == \
        [(1, 1), (2, 1), (8, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 4), (64, 8), (64, 8)]


def test_q_values_batches_and_tables():
    p = np.array([0.01, 0.04, 0.03, 0.5, np.nan, 0.02])
    q = check.bh_qvalues(p)
    assert np.isnan(q[4]) and np.allclose(q[[0, 5, 2, 1, 3]], [0.05, 0.05, 0.05, 0.05, 0.5])
    assert (check.bh_qvalues(np.zeros(3)) == 0).all() and check.bh_qvalues(np.array([])).size == 0
    for n_stored, stride in ((40, 1), (500, 10), (7, 2), (1, 1), (3, 5)):
        calls, B = check.ppp_batches(n_stored, stride)
        used = [t for it0, n_it, _ in calls for t in range(it0, it0 + n_it, stride)]
        assert used == list(range(0, n_stored, stride)) and sum(c for _, _, c in calls) == B
        assert all(it0 % stride == 0 and n_it >= 1 for it0, n_it, _ in calls)
    assert check.default_stride(500) == 10 and check.default_stride(40) == 1 and check.default_stride(0) == 1
    mk = lambda ge, n_used: (dict(ge_sample=np.array(ge), rep_sample=np.array([[4.0 * n_used, 10.0 * n_used]] * len(ge)),
                                  obs_sample=np.array([3.0 * n_used] * len(ge)), n_used=n_used, R=2), True)
    tab = check.ppp_table([mk([1, 4], 2), mk([3, 4], 2)], "sample")
    assert np.allclose(tab["p"], [0.5, 1.0]) and np.allclose(tab["T_obs"], 3.0) and np.allclose(tab["T_rep"], 2.0)
    assert np.allclose(tab["T_rep_sd"], 1.0) and np.allclose(tab["p_mcse"], [0.25, 0.0])
    assert np.isnan(check.ppp_table([mk([1], 2)], "sample")["p_mcse"]).all()


def test_symbols_are_declared_exported_and_bound():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_ppc", "dsm_ppc_debug_set_parts", "dsm_ppc_debug_set_chunk", "dsm_ppc_debug_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for fn in (_lib.Context.trace_ppc, _lib.Context.ppc_debug_path, _lib.ppc_debug_set_parts, _lib.ppc_debug_set_chunk,
               HaploSNP_Sampler.fitReplicates):
        assert callable(fn)
    assert inspect.signature(HaploSNP_Sampler.fitReplicates).parameters["reps"].default == check.REPS == 20
    assert lib.dsm_ctx_trace_ppc(None, 0, 0, 1, 1, 0, None, None, None, None, None, None) != 0             # (a null context)
    assert lib.dsm_ppc_debug_set_parts(-1) == -2
    assert re.search(r"#define\s+DSM_PPC_MAX_R\s+%d\b" % ref.MAX_R, hdr) and re.search(r"#define\s+DSM_PPC_READS\s+%d\b" % ref.READS, hdr)
    src = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "desman_amd", "csrc", "dsm_device.h")).read()
    assert re.search(r"#define\s+DSM_STREAM_PPCR\s+0x%08Xu" % ref.STREAM_PPCR, src) and ref.STREAM_PPCR == int.from_bytes(b"PPCR", "big")
    tags = [int(x, 16) for x in re.findall(r"#define\s+DSM_STREAM_\w+\s+0x([0-9A-Fa-f]{8})u", src)]
    assert len(tags) == len(set(tags))


def test_the_command_line_refuses_what_it_cannot_serve_before_any_chain(tmp_path, monkeypatch):
    from desman_amd import cli

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    out = str(tmp_path / "out")
    freq = str(tmp_path / "never_read.freq")                   # the file does not exist: a run that got as far as loading would say so
    base = [freq, "-g", "3", "-o", out]
    for args, msg in ((["--check-reps"], "--check-reps needs --check"), (["--check-reps", "5"], "--check-reps needs --check"),
                      (["--check", "--check-reps", "0"], "1 to 1024 replicates per iteration; got 0"),
                      (["--check", "--check-reps", "-2"], "got -2"), (["--check", "--check-reps", "1025"], "got 1025"),
                      (["--check", "--check-reps", "-i", "0"], "at least 1 is needed"),
                      (["--check", "--check-stride", "2"], "--check-stride needs --check-reps"),
                      (["--check", "--check-reps", "--check-stride", "0"], "--check-stride: at least 1; got 0")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + args)
        assert msg in str(e.value), (args, str(e.value))
    with pytest.raises(SystemExit, match="--check-reps is not available for replicate chains"):
        cli.main_replicates([base + ["--check", "--check-reps"]])
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse(base).check_reps is None and parse(base + ["--check", "--check-reps"]).check_reps == check.REPS
    assert parse(base + ["--check", "--check-reps", "7", "--check-stride", "3"]).check_stride == 3
    assert "conservative" in cli.build_parser().format_help() and "probability scale" in cli.build_parser().format_help()


def test_the_sampler_refuses_what_it_cannot_serve_before_any_device_work(monkeypatch):
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler

    def boom(*a, **k):
        raise AssertionError("the library was called")
    chain = HaploSNP_Sampler.__new__(HaploSNP_Sampler)
    chain.max_iter, chain._have_trace = 10, True
    chain._ctx = type("C", (), {"trace_ppc": boom})()
    with pytest.raises(ValueError, match="at least 1 replicate"):
        chain.fitReplicates(reps=0)
    with pytest.raises(ValueError, match="stride must be at least 1"):
        chain.fitReplicates(reps=3, stride=0)
    chain._have_trace = False
    with pytest.raises(_lib.DesmanHipError, match="no update"):
        chain.fitReplicates(reps=3)
