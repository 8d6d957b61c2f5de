"""`desman-abund`: abundances of a finished run's haplotypes in samples that were not in the fit.

    python -m desman_amd.abund <run_dir> <table.freq> [-o DIR] [--tau FILE] [--only-new] [--presence] [--interval [LEVEL]] [--ctol X]
                                                      [--fit-eta] [--posterior [N]] [--burn B] [--posterior-seed X] [--novel K]
                                                      [--max-iter N] [--tol X] [--device N]

`desman` drops every sample whose mean depth is not above -m, and a sample sequenced after the fit has no row in ``Gamma_star.csv``
either; a refit would give new haplotypes with new labels.  This entry point holds the run's haplotypes and error matrix fixed and
fits each sample's abundance row by maximum likelihood on the GPU (include/desman_hip.h: dsm_fit_gamma; the reference has no
counterpart).  It reads ``Eta_star.csv`` and the haplotypes -- ``--tau FILE``, else ``Collated_Tau_star.csv`` (the -r path: every
position), else ``Filtered_Tau_star.csv`` -- matches the model's positions to the rows of the base-count table by (contig,
Position) and writes

    Projected_Gamma.csv      layout and sample naming of Gamma_star.csv
    Projected_fit.csv        per sample: reads, mean depth over the model's positions, loglik, deviance, deviance per read,
                             iters, converged (0: --max-iter ended the iteration, the row is not the maximum)
    Projected_presence.csv   with --presence: S x G likelihood-ratio statistics 2 (L - max L with haplotype g absent)
    Projected_interval.csv   with --interval [LEVEL] (default 0.95): per sample and haplotype <g>_lo, <g>_hi, <g>_flag -- the
                             profile-likelihood interval of the abundance in Projected_Gamma.csv (dsm_fit_gamma_interval; each end
                             found to --ctol) and its flag bits: 1 lo is the boundary 0, 2 hi is the boundary 1, 4 an inner fit
                             ended at --max-iter (the interval is too narrow)

    Projected_posterior.csv  with --posterior [N] (default 1000 iterations, the first --burn B = 200 dropped): per sample and haplotype
                             <g>_mean, <g>_sd, <g>_lo, <g>_med, <g>_hi of the abundance's posterior under the run's Dirichlet prior
                             (alpha = 0.1) with the haplotypes held (dsm_ctx_gibbs_update_fixed_tau); lo / hi at the level of
                             --interval when given, else 0.95.  --posterior-seed X keys the chain's streams: the same call writes
                             the same file.  Where the profile interval of an absent haplotype says lo = 0 and no more, this says
                             how much abundance the data still allow.

With --fit-eta the error matrix is not the run's: the samples may come from another library preparation, sequencer or mapper than the
fit's.  One error matrix shared by the samples of the call is estimated together with their abundances, from ``Eta_star.csv`` as the
start (dsm_fit_gamma_eta); Projected_Gamma.csv and Projected_fit.csv then hold the joint fit's rows (iters and converged are the
call's), Projected_fit.csv has one more column, loglik_eta0 (the fit with the run's error matrix), --presence and --interval use the
fitted matrix, and two more files are written:

    Projected_Eta.csv        the fitted error matrix, in the format of Eta_star.csv
    Projected_eta_fit.csv    one row: loglik, loglik_eta0 (both summed over the samples), lr_eta = 2 (loglik - loglik_eta0), iters,
                             converged, dead_rows (bit a: no haplotype with abundance carries base a, row a is the run's)
    Projected_Eta_posterior.csv   with --posterior: the chain samples the error matrix too, from the fitted one as its start; per
                             true base (row) <b>_mean and <b>_sd of the posterior of eta[row, b]

With --novel K the new samples may also contain strains the run did not find: the run's G haplotypes are held, K free haplotypes are
placed in front of them and sampled together with the abundances by the partly held chain (dsm_ctx_gibbs_update_held_tau; DESIGN.md
sec. 8e) -- --posterior N iterations, the first --burn dropped (that option's defaults when it is not given), streams keyed by
--posterior-seed, eta = the run's (held) or, with --fit-eta, the fitted one as the start (sampled).  The start is not tuned: uniform
abundance rows over the G + K haplotypes, every free digit drawn uniformly from the bases with a non-zero pooled count at its position
by numpy's RandomState(--posterior-seed mod 2^32).  The K = 0 chain of --posterior is run on the same table as the baseline.  Written
next to the usual files, which do not change (--interval and --presence speak of the held-only model):

    Novel_Tau_star.csv         all K + G haplotypes of the MAP state in the format of Filtered_Tau_star.csv, the K free ones first; the
                               held ones are the input
    Novel_Gamma_star.csv       the MAP state's abundances; columns novel0 .. novel<K-1>, then the run's haplotypes under their numbers
    Novel_Gamma_posterior.csv  <label>_mean, _sd, _lo, _med, _hi per sample and haplotype after burn-in (lo / hi as --posterior)
    Novel_fit.csv              one row for K = 0 and one for K: deviance = -2 mean(ll) after burn-in, lp_star = lp of the MAP record,
                               iters = iterations kept
    Novel_haplotypes.csv       per free haplotype: distance = positions in which it differs from the nearest held haplotype, nearest =
                               that haplotype, mean_abundance / max_abundance over the samples (posterior means).  A free haplotype at
                               distance 0 from a held one is an over-fit; the file shows that, it does not decide it.
"""
import argparse
import os
import sys

import numpy as np
import pandas as pd

from .Output_Results import rchop

POSTERIOR_N, POSTERIOR_BURN, POSTERIOR_SEED = 1000, 200, 0x8C1F3A5D7E9B2468      # fixed_tau.POSTERIOR_SEED
MAX_ITER, TOL, CTOL = 20000, 1.0e-9, 1.0e-6          # _lib.FIT_MAX_ITER / FIT_TOL / FIT_CTOL (the parser must not need the library)
NOVEL_MAX_G = 32                                     # held_tau.MAX_G = DSM_MAX_G
TAU_FILES = ("Collated_Tau_star.csv", "Filtered_Tau_star.csv")


def build_parser():
    ap = argparse.ArgumentParser(prog="desman-abund",
                                 description="abundances of a finished desman run's haplotypes in further samples (MI355X)")
    ap.add_argument("run_dir", help="output directory of a finished `desman` run")
    ap.add_argument("freq_file", help="base-count table with the samples to fit: Contig,Position,<sample>-A,-C,-G,-T,...")
    ap.add_argument("-o", "--output_dir", type=str, default=None, help="directory for the result files (default: run_dir)")
    ap.add_argument("--tau", type=str, default=None, help="haplotype table to use instead of the run's Collated / Filtered_Tau_star.csv")
    ap.add_argument("--only-new", action="store_true", help="fit only the samples without a row in the run's Gamma_star.csv")
    ap.add_argument("--presence", action="store_true", help="also write the likelihood-ratio statistics of each haplotype's absence")
    ap.add_argument("--interval", type=float, nargs="?", const=0.95, default=None, metavar="LEVEL",
                    help="also write the profile-likelihood intervals of the abundances at this confidence level (default 0.95)")
    ap.add_argument("--fit-eta", action="store_true",
                    help="estimate one error matrix for the samples of the table together with their abundances (start: Eta_star.csv)")
    ap.add_argument("--posterior", type=int, nargs="?", const=POSTERIOR_N, default=None, metavar="N",
                    help="also write the posterior of the abundances under the run's Dirichlet prior, from N iterations of the "
                         "fixed-haplotype chain (default %d); with --fit-eta the chain samples the error matrix too" % POSTERIOR_N)
    ap.add_argument("--burn", type=int, default=POSTERIOR_BURN, metavar="B",
                    help="iterations of --posterior dropped at the start (default %d)" % POSTERIOR_BURN)
    ap.add_argument("--posterior-seed", type=lambda v: int(v, 0), default=POSTERIOR_SEED, metavar="X",
                    help="stream key of the --posterior chain (default 0x%X)" % POSTERIOR_SEED)
    ap.add_argument("--novel", type=int, default=None, metavar="K",
                    help="also fit K further haplotypes to the samples with the run's haplotypes held (the partly held chain; length, "
                         "burn-in and key as --posterior) and write the Novel_* files")
    ap.add_argument("--ctol", type=float, default=CTOL, help="width to which an interval end is found (default %g)" % CTOL)
    ap.add_argument("--max-iter", type=int, default=MAX_ITER, help="EM steps at most (default %d)" % MAX_ITER)
    ap.add_argument("--tol", type=float, default=TOL, help="stop when no abundance moves by this much in a step (default %g)" % TOL)
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    return ap


def tau_path(run_dir, tau=None):
    """the haplotype table of a run: the one named, else the collated table of a -r run, else the filtered one"""
    if tau is not None:
        if not os.path.isfile(tau):
            sys.exit("desman-abund: can't open '%s'" % tau)
        return tau
    for name in TAU_FILES:
        path = os.path.join(run_dir, name)
        if os.path.isfile(path):
            return path
    sys.exit("desman-abund: can't open '%s'" % os.path.join(run_dir, TAU_FILES[-1]))


def load_model(run_dir, tau=None):
    """(contigs, positions, tau digits [V,G], eta [4,4]) of a run directory; exits with a message naming what is missing"""
    eta_path = os.path.join(run_dir, "Eta_star.csv")
    if not os.path.isfile(eta_path):
        sys.exit("desman-abund: can't open '%s'" % eta_path)
    eta = pd.read_csv(eta_path, header=0, index_col=0, float_precision="round_trip").to_numpy(dtype=np.float64)
    if eta.shape != (4, 4):
        sys.exit("desman-abund: '%s' is not a 4 x 4 table" % eta_path)
    path = tau_path(run_dir, tau)
    table = pd.read_csv(path, header=0, index_col=0)
    cols = [str(c) for c in table.columns.values.tolist()]
    if not cols or cols[0] != "Position" or (len(cols) - 1) % 4 or len(cols) < 5:
        sys.exit("desman-abund: '%s' needs a Position column followed by four columns per haplotype" % path)
    onehot = table.to_numpy()[:, 1:].reshape(len(table), (len(cols) - 1) // 4, 4)
    if not ((onehot == 0) | (onehot == 1)).all() or not (onehot.sum(axis=2) == 1).all():
        sys.exit("desman-abund: '%s' is not a one-hot haplotype table" % path)
    digits = np.ascontiguousarray(np.argmax(onehot, axis=2), dtype=np.int64)
    return [str(n) for n in table.index.tolist()], table["Position"].to_numpy(), digits, np.ascontiguousarray(eta)


def sample_names(table):
    cols = [str(c) for c in table.columns.values.tolist()]
    if not cols or cols[0] != "Position" or (len(cols) - 1) % 4 or len(cols) < 5:
        sys.exit("desman-abund: the count table needs a Position column followed by four columns per sample")
    return [rchop(cols[1 + 4 * k], "-A") for k in range((len(cols) - 1) // 4)]


def match_positions(table, contigs, positions):
    """row of the count table for every model position, by (contig, Position); a model position the table lacks is an error that
    names it, rows of the table that are not in the model are ignored (a key that occurs twice: its first row)"""
    where = {}
    for r, key in enumerate(zip((str(n) for n in table.index.tolist()), table["Position"].tolist())):
        where.setdefault(key, r)
    rows = np.empty(len(contigs), dtype=np.int64)
    for i, key in enumerate(zip(contigs, (int(p) for p in positions))):
        if key not in where:
            sys.exit("desman-abund: position %s,%d of the model is not in the count table" % key)
        rows[i] = where[key]
    return rows


def fitted_names(run_dir):
    """sample names with a row in the run's Gamma_star.csv (none if the run has no such file)"""
    path = os.path.join(run_dir, "Gamma_star.csv")
    if not os.path.isfile(path):
        return []
    return [str(n) for n in pd.read_csv(path, header=0, index_col=0).index.tolist()]


def select_counts(table, rows, keep):
    """counts [V,S',4] int64 of the samples number `keep` at the table rows `rows`"""
    data = table.to_numpy()[rows, 1:]
    cube = data.reshape(len(rows), (data.shape[1]) // 4, 4)
    return np.ascontiguousarray(cube[:, keep, :].astype(np.int64))


def write_results(out_dir, names, counts, res):
    os.makedirs(out_dir, exist_ok=True)
    pd.DataFrame(res["gamma"], index=names).to_csv(os.path.join(out_dir, "Projected_Gamma.csv"))      # Output_Results._abundance_table
    reads = counts.sum(axis=(0, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        per_read = np.where(reads > 0, res["deviance"] / np.maximum(reads, 1), 0.0)
    fit = pd.DataFrame({"reads": reads.astype(np.int64), "mean_depth": reads / float(counts.shape[0]), "loglik": res["loglik"],
                        "deviance": res["deviance"], "deviance_per_read": per_read, "iters": np.asarray(res["iters"], dtype=np.int64),
                        "converged": np.asarray(res["converged"], dtype=np.int64)}, index=names)
    if "loglik0" in res:
        fit["loglik_eta0"] = res["loglik0"]
    fit.to_csv(os.path.join(out_dir, "Projected_fit.csv"))
    if "lr_absent" in res:
        pd.DataFrame(res["lr_absent"], index=names).to_csv(os.path.join(out_dir, "Projected_presence.csv"))


def write_eta(out_dir, res):
    """Projected_Eta.csv in the format of Eta_star.csv (Output_Results), and the one-row Projected_eta_fit.csv"""
    pd.DataFrame(res["eta"]).to_csv(os.path.join(out_dir, "Projected_Eta.csv"))
    row = {"loglik": [float(np.sum(res["loglik"]))], "loglik_eta0": [float(np.sum(res["loglik0"]))], "lr_eta": [res["lr_eta"]],
           "iters": [int(res["iters"])], "converged": [int(res["converged"])], "dead_rows": [int(res["dead_rows"])]}
    pd.DataFrame(row).to_csv(os.path.join(out_dir, "Projected_eta_fit.csv"), index=False)


def fit_eta(counts, digits, eta, opts):
    """the joint fit in the layout of fit_gamma's result: iters and converged per sample (the call's), the call's scalars under eta_fit"""
    from . import _lib
    S = counts.shape[1]
    joint = _lib.fit_gamma_eta(counts, digits, eta, max_iter=opts.max_iter, tol=opts.tol, device=opts.device)
    res = dict(joint)
    res["iters"] = np.full(S, joint["iters"], dtype=np.int64)
    res["converged"] = np.full(S, joint["converged"], dtype=np.int64)
    res["eta_fit"] = joint
    return res


def write_interval(out_dir, names, iv):
    """Projected_interval.csv: rows and haplotype names of Projected_Gamma.csv, three columns per haplotype"""
    cols = {}
    for g in range(iv["lo"].shape[1]):
        cols["%d_lo" % g] = iv["lo"][:, g]
        cols["%d_hi" % g] = iv["hi"][:, g]
        cols["%d_flag" % g] = np.asarray(iv["flags"][:, g], dtype=np.int64)
    pd.DataFrame(cols, index=names).to_csv(os.path.join(out_dir, "Projected_interval.csv"))


def write_posterior(out_dir, names, post):
    """Projected_posterior.csv: rows and haplotype names of Projected_Gamma.csv, five columns per haplotype"""
    cols = {}
    for g in range(post["mean"].shape[1]):
        for key in ("mean", "sd", "lo", "med", "hi"):
            cols["%d_%s" % (g, key)] = post[key][:, g]
    pd.DataFrame(cols, index=names).to_csv(os.path.join(out_dir, "Projected_posterior.csv"))


def write_eta_posterior(out_dir, post):
    """Projected_Eta_posterior.csv: rows of Eta_star.csv (true base), <b>_mean and <b>_sd per observed base"""
    cols = {}
    for b in range(4):
        cols["%d_mean" % b] = post["eta_mean"][:, b]
        cols["%d_sd" % b] = post["eta_sd"][:, b]
    pd.DataFrame(cols).to_csv(os.path.join(out_dir, "Projected_Eta_posterior.csv"))


def main(argv=None):
    opts = build_parser().parse_args(argv)
    if opts.interval is not None and not 0.0 < opts.interval < 1.0:
        sys.exit("desman-abund: --interval needs a level between 0 and 1")
    if opts.posterior is not None and not (opts.posterior >= 1 and 0 <= opts.burn < opts.posterior):
        sys.exit("desman-abund: --posterior needs N >= 1 iterations and 0 <= --burn < N")
    n_chain = POSTERIOR_N if opts.posterior is None else opts.posterior
    if opts.novel is not None and opts.novel < 1:
        sys.exit("desman-abund: --novel needs K >= 1 free haplotypes")
    if opts.novel is not None and not 0 <= opts.burn < n_chain:
        sys.exit("desman-abund: --novel runs %d iterations (--posterior N), --burn must lie in 0 .. N - 1" % n_chain)
    contigs, positions, digits, eta = load_model(opts.run_dir, opts.tau)
    if opts.novel is not None and digits.shape[1] + opts.novel > NOVEL_MAX_G:
        sys.exit("desman-abund: --novel %d with the run's %d haplotypes makes more than %d" % (opts.novel, digits.shape[1], NOVEL_MAX_G))
    if not os.path.isfile(opts.freq_file):
        sys.exit("desman-abund: can't open '%s'" % opts.freq_file)
    table = pd.read_csv(opts.freq_file, header=0, index_col=0)
    names = sample_names(table)
    rows = match_positions(table, contigs, positions)
    keep = list(range(len(names)))
    if opts.only_new:
        old = set(fitted_names(opts.run_dir))
        keep = [k for k in keep if names[k] not in old]
    if not keep:
        sys.exit("desman-abund: no sample to fit (--only-new: every sample of the table has a row in Gamma_star.csv)")
    counts = select_counts(table, rows, keep)
    from . import _lib                                                      # nothing above needs the library or a GPU
    if opts.fit_eta:
        res = fit_eta(counts, digits, eta, opts)
        joint = res["eta_fit"]
        if not np.isfinite(joint["eta"]).all() or not joint["gamma"].any():
            print("desman-abund: --fit-eta: Eta_star.csv gives some read probability 0, nothing was fitted "
                  "(Projected_fit.csv: loglik = -inf)", file=sys.stderr)
        elif not joint["converged"]:
            print("desman-abund: --fit-eta did not converge in %d steps (Projected_eta_fit.csv: converged = 0)" % opts.max_iter,
                  file=sys.stderr)
        if joint["dead_rows"]:
            print("desman-abund: --fit-eta: no haplotype with abundance carries base %s, the rows of Projected_Eta.csv for them are "
                  "the run's (Projected_eta_fit.csv: dead_rows = %d)"
                  % (", ".join("ACGT"[a] for a in range(4) if joint["dead_rows"] >> a & 1), joint["dead_rows"]), file=sys.stderr)
        eta = np.ascontiguousarray(joint["eta"])                            # --presence and --interval below: the fitted matrix
        if opts.presence:
            res["lr_absent"] = _lib.fit_gamma(counts, digits, eta, max_iter=opts.max_iter, tol=opts.tol, presence=True,
                                              device=opts.device)["lr_absent"]
        write_results(opts.output_dir or opts.run_dir, [names[k] for k in keep], counts, res)
        write_eta(opts.output_dir or opts.run_dir, joint)
        n_open = 0
    else:
        res = _lib.fit_gamma(counts, digits, eta, max_iter=opts.max_iter, tol=opts.tol, presence=opts.presence, device=opts.device)
        write_results(opts.output_dir or opts.run_dir, [names[k] for k in keep], counts, res)
        n_open = int((np.asarray(res["converged"]) == 0).sum())
    if n_open:
        print("desman-abund: %d of %d samples did not converge in %d steps (Projected_fit.csv: converged = 0)"
              % (n_open, len(keep), opts.max_iter), file=sys.stderr)
    if opts.interval is not None:
        iv = _lib.fit_gamma_interval(counts, digits, eta, res["gamma"], level=opts.interval, max_iter=opts.max_iter, tol=opts.tol,
                                     ctol=opts.ctol, device=opts.device)
        write_interval(opts.output_dir or opts.run_dir, [names[k] for k in keep], iv)
        short = [names[k] for i, k in enumerate(keep) if (np.asarray(iv["flags"][i]) & 4).any()]
        if short:
            print("desman-abund: an inner fit of %d of %d samples ended at --max-iter %d, their intervals are too narrow "
                  "(Projected_interval.csv: flag bit 4): %s" % (len(short), len(keep), opts.max_iter, ", ".join(short)), file=sys.stderr)
        res.update(iv)
    if opts.posterior is not None:
        from . import fixed_tau
        post = fixed_tau.posterior_gamma(counts, digits, eta, n_iter=opts.posterior, burn=opts.burn, fix_eta=not opts.fit_eta,
                                         level=0.95 if opts.interval is None else opts.interval, seed=opts.posterior_seed,
                                         device=opts.device)
        write_posterior(opts.output_dir or opts.run_dir, [names[k] for k in keep], post)
        if opts.fit_eta:
            write_eta_posterior(opts.output_dir or opts.run_dir, post)
        res["posterior"] = post
    if opts.novel is not None:
        from . import fixed_tau, held_tau
        chain = dict(n_iter=n_chain, burn=opts.burn, fix_eta=not opts.fit_eta, level=0.95 if opts.interval is None else opts.interval,
                     seed=opts.posterior_seed, device=opts.device)
        base = res["posterior"] if "posterior" in res else fixed_tau.posterior_gamma(counts, digits, eta, **chain)     # K = 0
        novel = held_tau.novel_chain(counts, digits, eta, opts.novel, **chain)
        held_tau.write_novel(opts.output_dir or opts.run_dir, [names[k] for k in keep], contigs, positions, base, novel, opts.novel)
        res["novel"], res["novel_base"] = novel, base
    return res


if __name__ == "__main__":
    main()
