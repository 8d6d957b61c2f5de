"""`desman-assign`: haplotype calls for positions that were not in a fit, from the fit's result files.

    python -m desman_amd.assign <run_dir> <positions.freq> [-o DIR] [--mean] [--draw] [--seed N] [--device N]
                                [--sampled [T]] [--burn B] [--pairs [E]]

The reference reserves `desman -a` for this (bin/desman:209-240, HaploSNP_Sampler.assignTau) but the branch is dead upstream and
its 4^G Python loops are unusable above G ~ 5; `desman -a` stays rejected here (desman_amd/cli.py).  This entry point needs no
chain: it reads ``Gamma_star.csv`` + ``Eta_star.csv`` (``--mean``: ``Gamma_mean.csv`` + ``Eta_mean.csv``) of a finished `desman`
output directory, maps the sample columns of the new base-count table onto the run's samples by name, evaluates all 4^G joint
states of every position on the GPU (include/desman_hip.h: dsm_assign_tau, G <= 10) and writes

    Assigned_Tau_star.csv   index = contig, Position, then G x 4 one-hot columns (haplotype-major): the MAP state,
                            or one posterior draw with --draw (the reference's assignTau)
    Assigned_Tau_conf.csv   index = contig, Position, column 0 = posterior probability of the MAP state (the reference's conf)
    Assigned_Tau_mean.csv   the exact marginals P(tau_vg = a), layout of Tau_Mean.csv
    assign_fit.txt          Assign,<G>,<N>,<sum of the positions' log normalisers>

With ``--sampled [T]`` every G <= 32 is accepted: each position runs four private Gibbs chains of B burn-in and T kept sweeps on the
GPU (dsm_assign_tau_sampled), keyed by ``--seed``.  The three tables keep their layout -- the MAP state is the
best state any chain saw, polished by coordinate ascent (``--draw``: chain 0's last state), conf the share of the kept end-of-sweep
states equal to it, the marginals Rao-Blackwellised means -- and there are

    Assigned_Tau_spread.csv index = contig, Position, column 0 = the largest disagreement between the four chains' own marginals:
                            large where the chains sit in different modes (two haplotypes of near-equal abundance with swapped bases)
    assign_fit.txt          AssignSampled,<G>,<N>,<B>,<T>,<sum of the MAP states' log-likelihoods>

``--pairs [E]`` adds joint moves of two haplotypes to ``--sampled``: every E-th sweep is followed by a pass that redraws the bases of
every pair of haplotypes from their 16-state conditional, and the polish climbs over pairs as well, so swapped bases of two
haplotypes are one step apart (dsm_assign_tau_sampled_pairs).  The files keep their names and formats.
"""
import argparse
import os
import sys

import numpy as np
import pandas as pd

from .Output_Results import _table_bytes, rchop

DRAW_SEED = 23724839        # default --seed: the default sampler seed of `desman` (bin/desman:51)
SAMPLED_KEPT, SAMPLED_BURN = 100, 20    # --sampled / --burn: conventions, not tuned (desman_amd/_lib.py has the same pair)
SAMPLED_PAIRS = 5           # a bare --pairs: a pair pass after every fifth sweep -- a convention, not tuned (_lib.SAMPLED_PAIRS)
SAMPLED_MAX_G = 32          # DSM_MAX_G
SPREAD_HIGH = 0.1           # the log line counts the positions above it: a convention for that line only, like check.Z_HIGH


# where the sampled form becomes the cheaper one: measured on the MI355X at S = 64, N = 10 000 ("Measurement")
SAMPLED_CHEAPER = ("At the default sweeps it is the cheaper form from G = 8 (measured at S = 64: 2.9 times faster than the exact call at "
                   "G = 8, 38 times at G = 10, 3 times slower at G = 6).")


def build_parser():
    ap = argparse.ArgumentParser(prog="desman-assign",
                                 description="exact haplotype assignment of new positions from a finished desman run (MI355X)")
    ap.add_argument("run_dir", help="output directory of a finished `desman` run")
    ap.add_argument("freq_file", help="base-count table of the positions to assign: Contig,Position,<sample>-A,-C,-G,-T,...")
    ap.add_argument("-o", "--output_dir", type=str, default=None, help="directory for the result files (default: run_dir)")
    ap.add_argument("--mean", action="store_true", help="use Gamma_mean.csv / Eta_mean.csv instead of the MAP sample's files")
    ap.add_argument("--draw", action="store_true", help="write one posterior draw per position instead of the MAP state")
    ap.add_argument("--seed", type=int, default=DRAW_SEED, help="seed of --draw; with --sampled the key of the chains")
    ap.add_argument("--sampled", type=int, nargs="?", const=SAMPLED_KEPT, default=None, metavar="T",
                    help="four private Gibbs chains per position with T kept sweeps (default %d: a convention, not tuned) instead of "
                         "all 4^G states: any G <= %d.  %s" % (SAMPLED_KEPT, SAMPLED_MAX_G, SAMPLED_CHEAPER))
    ap.add_argument("--burn", type=int, default=None, metavar="B",
                    help="burn-in sweeps of --sampled (default %d: a convention, not tuned)" % SAMPLED_BURN)
    ap.add_argument("--pairs", type=int, nargs="?", const=SAMPLED_PAIRS, default=None, metavar="E",
                    help="with --sampled: a pass of joint moves of two haplotypes after every E-th sweep (default %d: a convention, not "
                         "tuned) and in the polish; crosses swapped bases of two haplotypes, costs about 2 (G - 1) / E more time"
                         % SAMPLED_PAIRS)
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    return ap


def load_model(run_dir, mean=False):
    """(sample names, gamma [S,G], eta [4,4]) of a run directory; exits with a message naming the file that is missing"""
    tag = "mean" if mean else "star"
    paths = [os.path.join(run_dir, "%s_%s.csv" % (k, tag)) for k in ("Gamma", "Eta")]
    for path in paths:
        if not os.path.isfile(path):
            sys.exit("desman-assign: can't open '%s'" % path)
    gamma_df = pd.read_csv(paths[0], header=0, index_col=0, float_precision="round_trip")
    eta = pd.read_csv(paths[1], header=0, index_col=0, float_precision="round_trip").to_numpy(dtype=np.float64)
    if eta.shape != (4, 4):
        sys.exit("desman-assign: '%s' is not a 4 x 4 table" % paths[1])
    names = [str(n) for n in gamma_df.index.tolist()]
    return names, np.ascontiguousarray(gamma_df.to_numpy(dtype=np.float64)), np.ascontiguousarray(eta)


def map_samples(table, names):
    """counts [N,S,4] of the run's samples `names`, taken from the table's <sample>-A/-C/-G/-T columns by name"""
    cols = [str(c) for c in table.columns.values.tolist()]
    if not cols or cols[0] != "Position" or (len(cols) - 1) % 4:
        sys.exit("desman-assign: the count table needs a Position column followed by four columns per sample")
    first = {rchop(cols[1 + 4 * k], "-A"): 1 + 4 * k for k in range((len(cols) - 1) // 4)}
    missing = [n for n in names if n not in first]
    if missing:
        sys.exit("desman-assign: sample '%s' of the run is not in the count table" % missing[0])
    data = table.to_numpy()
    take = np.array([[first[n] + b for b in range(4)] for n in names], dtype=np.int64)       # [S,4] column numbers
    return np.ascontiguousarray(data[:, take].astype(np.int64))


def write_table(path, values, names, positions):
    """a haplotype table as Output_Results writes them: index = names, Position first, then the flattened columns"""
    flat = np.reshape(values, (values.shape[0], -1))
    text = _table_bytes(flat, names, positions)
    if text is not None:
        with open(path, "wb") as fh:
            fh.write(text)
        return
    frame = pd.DataFrame(flat, index=names)
    frame['Position'] = np.asarray(positions)
    order = frame.columns.tolist()
    frame[order[-1:] + order[:-1]].to_csv(path)


def onehot(state):
    """[N,G] digits -> [N,G,4] int64 one-hot"""
    out = np.zeros(state.shape + (4,), dtype=np.int64)
    np.put_along_axis(out, state.astype(np.int64)[..., None], 1, axis=2)
    return out


def write_results(out_dir, names, positions, res, draw=False):
    os.makedirs(out_dir, exist_ok=True)
    state = res["draw_state"] if draw else res["map_state"]
    N, G = state.shape
    write_table(os.path.join(out_dir, "Assigned_Tau_star.csv"), onehot(state), names, positions)
    conf = pd.DataFrame(res["conf"], index=names)                           # bin/desman:225-240
    conf['Position'] = np.asarray(positions)
    order = conf.columns.tolist()
    conf[order[-1:] + order[:-1]].to_csv(os.path.join(out_dir, "Assigned_Tau_conf.csv"))
    write_table(os.path.join(out_dir, "Assigned_Tau_mean.csv"), res["marg"], names, positions)
    with open(os.path.join(out_dir, "assign_fit.txt"), "w") as fh:
        fh.write("Assign,%d,%d,%f\n" % (G, N, float(np.sum(res["logz"]))))


def write_sampled_results(out_dir, names, positions, res, burn, kept, draw=False):
    os.makedirs(out_dir, exist_ok=True)
    state = res["draw_state"] if draw else res["map_state"]
    N, G = state.shape
    write_table(os.path.join(out_dir, "Assigned_Tau_star.csv"), onehot(state), names, positions)
    for key, fname in (("conf", "Assigned_Tau_conf.csv"), ("spread", "Assigned_Tau_spread.csv")):
        frame = pd.DataFrame(res[key], index=names)
        frame['Position'] = np.asarray(positions)
        order = frame.columns.tolist()
        frame[order[-1:] + order[:-1]].to_csv(os.path.join(out_dir, fname))
    write_table(os.path.join(out_dir, "Assigned_Tau_mean.csv"), res["marg"], names, positions)
    with open(os.path.join(out_dir, "assign_fit.txt"), "w") as fh:
        fh.write("AssignSampled,%d,%d,%d,%d,%f\n" % (G, N, burn, kept, float(np.sum(res["map_ll"]))))


def main(argv=None):
    opts = build_parser().parse_args(argv)
    if opts.burn is not None and opts.sampled is None:
        sys.exit("desman-assign: --burn needs --sampled")
    if opts.pairs is not None and opts.sampled is None:
        sys.exit("desman-assign: --pairs needs --sampled")
    if opts.pairs is not None and not 0 <= opts.pairs <= 65536:
        sys.exit("desman-assign: --pairs E needs 0 <= E <= 65536")
    if opts.sampled is not None:
        burn = SAMPLED_BURN if opts.burn is None else opts.burn
        if opts.sampled < 1 or burn < 0 or opts.sampled + burn > 65536:
            sys.exit("desman-assign: --sampled T --burn B need T >= 1, B >= 0 and B + T <= 65536")
    names, gamma, eta = load_model(opts.run_dir, opts.mean)
    if not os.path.isfile(opts.freq_file):
        sys.exit("desman-assign: can't open '%s'" % opts.freq_file)
    table = pd.read_csv(opts.freq_file, header=0, index_col=0)
    counts = map_samples(table, names)
    out_dir, row_names, positions = opts.output_dir or opts.run_dir, [str(n) for n in table.index.tolist()], table['Position'].to_numpy()
    if opts.sampled is not None and gamma.shape[1] > SAMPLED_MAX_G:
        sys.exit("desman-assign: %d haplotypes; the limit of --sampled is G = %d" % (gamma.shape[1], SAMPLED_MAX_G))
    from . import _lib                                                      # nothing above needs the library or a GPU
    if opts.sampled is not None:
        res = _lib.assign_tau_sampled(counts, gamma, eta, seed=opts.seed, burn=burn, kept=opts.sampled, device=opts.device,
                                      pair_every=opts.pairs or 0)
        write_sampled_results(out_dir, row_names, positions, res, burn, opts.sampled, opts.draw)
        print("desman-assign --sampled: %d of %d positions with spread > %.1f (chains in different modes)"
              % (int(np.sum(res["spread"] > SPREAD_HIGH)), len(res["spread"]), SPREAD_HIGH), file=sys.stderr)
        return res
    if gamma.shape[1] > _lib.ASSIGN_MAX_G:
        sys.exit("desman-assign: %d haplotypes; all 4^G joint states are evaluated, the limit is G = %d (--sampled runs to G = %d)"
                 % (gamma.shape[1], _lib.ASSIGN_MAX_G, SAMPLED_MAX_G))
    res = _lib.assign_tau(counts, gamma, eta, seed=opts.seed if opts.draw else None, device=opts.device)
    write_results(out_dir, row_names, positions, res, opts.draw)
    return res


if __name__ == "__main__":
    main()
