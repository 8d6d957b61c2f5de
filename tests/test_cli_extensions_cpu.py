"""The extension options of `desman` (--diagnose, --marginals, --check*, --predictive, --pair-moves) are validated by one function for
main() and for main_replicates(): every bad option set the per-option tests feed to main() (tests/test_diagnose_cpu.py,
test_tau_rb_cpu.py, test_check_cpu.py, test_check_reps_cpu.py, test_predictive_cpu.py, test_tau_pairs_cpu.py) goes to both here, and the
full text of the SystemExit is pinned.  The texts were recorded from the command line as it was before the two entry points shared that
function.  Every run stops before a table is read or the library is loaded, so no file and no GPU is needed."""
import os

import pytest

from desman_amd import _lib, cli

NO_REPS = "desman: %s is not available for replicate chains that share their launches: run the chains one by one"
FEW = "desman: %s: %d stored iterations (-i) are fewer than two batches of %d"

# (options, the text of main(), the text of main_replicates() -- None: the same)
CASES = [
    (["-i", "40", "--diagnose", "0"], "desman: --diagnose: the batch length must be at least 1; got 0", None),
    (["-i", "40", "--diagnose", "-2"], "desman: --diagnose: the batch length must be at least 1; got -2", None),
    (["-i", "40", "--diagnose", "21"], FEW % ("--diagnose", 40, 21), None),
    (["-i", "1", "--diagnose"], FEW % ("--diagnose", 1, 1), None),
    (["--diagnose", "126"], FEW % ("--diagnose", 250, 126), None),
    (["-i", "1", "--marginals"], FEW % ("--marginals", 1, 1), None),
    (["-i", "0", "--marginals"], FEW % ("--marginals", 0, 1), None),
    (["-i", "40", "--marginals", "--diagnose", "21"], FEW % ("--diagnose", 40, 21), None),       # --diagnose is looked at first
    (["-i", "40", "--marginals", "--diagnose", "0"], "desman: --diagnose: the batch length must be at least 1; got 0", None),
    (["--check-cells"], "desman: --check-cells needs --check", None),
    (["-i", "0", "--check"], "desman: --check: 0 stored iterations (-i): at least 1 is needed", None),
    (["-i", "0", "--check", "--check-cells", "--relabel"], "desman: --check: 0 stored iterations (-i): at least 1 is needed", None),
    (["--check-reps"], "desman: --check-reps needs --check", None),
    (["--check-reps", "5"], "desman: --check-reps needs --check", None),
    (["--check", "--check-stride", "2"], "desman: --check-stride needs --check-reps", None),
    (["--check", "--check-reps", "-i", "0"], "desman: --check: 0 stored iterations (-i): at least 1 is needed", None),
    (["--check", "--check-reps", "0"], "desman: --check-reps: 1 to 1024 replicates per iteration; got 0", NO_REPS % "--check-reps"),
    (["--check", "--check-reps", "-2"], "desman: --check-reps: 1 to 1024 replicates per iteration; got -2", NO_REPS % "--check-reps"),
    (["--check", "--check-reps", "1025"], "desman: --check-reps: 1 to 1024 replicates per iteration; got 1025", NO_REPS % "--check-reps"),
    (["--check", "--check-reps", "--check-stride", "0"], "desman: --check-stride: at least 1; got 0", NO_REPS % "--check-reps"),
    (["-g", "11", "--predictive"], "desman: --predictive sums over all 4^G haplotype states of a position: -g 11 is above 10",
     NO_REPS % "--predictive"),
    (["--predictive", "0"], "desman: --predictive: at least 1 stored iteration must be used; got 0", NO_REPS % "--predictive"),
    (["--predictive", "-2"], "desman: --predictive: at least 1 stored iteration must be used; got -2", NO_REPS % "--predictive"),
    (["-i", "0", "--predictive"], "desman: --predictive: 0 stored iterations (-i): at least 1 is needed", NO_REPS % "--predictive"),
    (["--pair-moves", "0"], "desman: --pair-moves: a pair pass every E-th iteration needs E >= 1; got 0", NO_REPS % "--pair-moves"),
    (["--pair-moves", "-3"], "desman: --pair-moves: a pair pass every E-th iteration needs E >= 1; got -3", NO_REPS % "--pair-moves"),
    # two faults at once: the options are looked at in the order pair moves, diagnose, marginals, check, predictive
    (["--pair-moves", "0", "--diagnose", "0"], "desman: --pair-moves: a pair pass every E-th iteration needs E >= 1; got 0",
     NO_REPS % "--pair-moves"),
    (["--diagnose", "0", "--check-cells"], "desman: --diagnose: the batch length must be at least 1; got 0", None),
    (["--check-cells", "--predictive", "0"], "desman: --check-cells needs --check", None),
    # what replicate chains do not serve is refused for them although the option set is sound
    (["--pair-moves"], None, NO_REPS % "--pair-moves"),
    (["--check", "--check-reps"], None, NO_REPS % "--check-reps"),
    (["--predictive"], None, NO_REPS % "--predictive"),
]


@pytest.fixture()
def base(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    out = str(tmp_path / "out")
    yield [str(tmp_path / "never_read.freq"), "-g", "3", "-o", out]      # a run that got as far as loading would say so
    assert not os.path.exists(out)


@pytest.mark.parametrize("extra,single,replicate", CASES, ids=[" ".join(c[0]) for c in CASES])
def test_refused_before_any_chain(base, extra, single, replicate):
    if single is not None:
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert str(e.value) == single
    with pytest.raises(SystemExit) as e:
        cli.main_replicates([base + extra])
    assert str(e.value) == (single if replicate is None else replicate)


def test_one_batch_rule_for_both_flags():
    parse = cli.build_parser().parse_args
    for argv in (["x", "-g", "3", "--diagnose", "--marginals"], ["x", "-g", "3", "-i", "40", "--diagnose", "4", "--marginals"],
                 ["x", "-g", "3", "-i", "500", "--diagnose", "--marginals"]):
        opts = parse(argv)
        assert cli._diagnose_batch_len(opts) == cli._marginals_batch_len(opts) == cli._extension_options(opts)["diag_len"]
    ext = cli._extension_options(parse(["x", "-g", "3", "-i", "40", "--marginals", "--pair-moves"]))
    assert ext == dict(pair_every=cli.PAIR_MOVES, diag_len=None, marg_len=6)
    assert cli._extension_options(parse(["x", "-g", "3"])) == dict(pair_every=0, diag_len=None, marg_len=None)
