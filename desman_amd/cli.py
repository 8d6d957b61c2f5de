"""`desman` command line on the device-resident classes.

Drop-in contract (reference: bin/desman:21-242): the same flags with the same defaults and quirks, and the
same output files.  The driver itself is organised differently: a flag table, then four
stages -- load, fit, report, assign-the-rest.
"""
import argparse
import logging
import os
import sys
import threading

import numpy as np
import pandas as pd
from numpy.random import RandomState

from . import sampletau
from .HaploSNP_Sampler import HaploSNP_Sampler
from .Init_NMFT import Init_NMFT
from .Output_Results import Output_Results
from .Variant_Filter import Variant_Filter

POSITION_SELECT_SEED = 238329          # fixed seed of the -r position draw (bin/desman:85-86)
DEFAULT_ITER = 250                     # the iterations a chain stores without -i, or with a bare -i: the sampler's own default

# (short, long, kwargs) -- defaults and nargs/const quirks as in bin/desman:25-59
_FLAGS = [
    ('-g', '--genomes', dict(type=int, required=True, help="number of haplotypes to infer")),
    ('-f', '--filter_variants', dict(nargs='?', const=3.84, type=float,
                                     help="likelihood-ratio variant filter; optional chi2 threshold (3.84)")),
    ('-r', '--random_select', dict(nargs='?', const=1e3, type=int,
                                   help="fit on this many random positions (1000), then assign the others")),
    ('-e', '--eta_file', dict(type=str, help="CSV with the initial 4x4 error matrix")),
    ('-a', '--assign_file', dict(type=str, help="(dead upstream) extra positions to assign")),
    ('-o', '--output_dir', dict(type=str, default="output", help="directory for all result files")),
    ('-p', '--optimiseP', dict(default=True, type=bool, help="optimise the mixture proportion in the filter")),
    ('-i', '--no_iter', dict(nargs='?', const=DEFAULT_ITER, type=int, help="Gibbs iterations per phase")),
    ('-m', '--min_coverage', dict(type=float, default=5.0, help="drop samples whose mean depth is not above this")),
    ('-q', '--max_qvalue', dict(default=1.0e-3, type=float, help="q-value cut of the variant filter")),
    ('-s', '--random_seed', dict(default=23724839, type=int, help="seed of both sampler RNG streams")),
    ('-v', '--min_variant_freq', dict(nargs='?', const=0.01, type=float, help="minimum variant frequency (0.01)")),
]


from .check import REPS as CHECK_REPS, N_USE as CHECK_N_USE        # a bare --check-reps; the used iterations --check-stride defaults to
CHECK_MAX_REPS = 1024       # DSM_PPC_MAX_R (include/desman_hip.h)
PAIR_MOVES = 5            # a bare --pair-moves: a pair pass after every fifth iteration -- the convention of `desman-assign --pairs`


def build_parser():
    ap = argparse.ArgumentParser(prog="desman", description="strain haplotypes and abundances from base counts (MI355X)")
    ap.add_argument("variant_file", help="base-count table: Contig,Position,<sample>-A,-C,-G,-T,...")
    for short, long_, kw in _FLAGS:
        ap.add_argument(short, long_, **kw)
    ap.add_argument('--device', type=int, default=0, help="GPU ordinal (extension)")
    ap.add_argument('--relabel', action='store_true',
                    help="also write the posterior summaries with every stored iteration's haplotype labels matched to the MAP "
                         "haplotypes first (Relabel.csv, Tau_Mean_relabelled.csv, Gamma_Mean_relabelled.csv, SND_posterior.csv, "
                         "Haplotype_stability.csv) (extension)")
    ap.add_argument('--relabel-ref', dest='relabel_ref', type=str, metavar='TAU_CSV',
                    help="with --relabel (implied): match the labels to the haplotypes of this Filtered_Tau_star.csv -- another run on "
                         "the same positions with the same -g -- instead of this run's own MAP haplotypes; a file that does not fit is refused "
                         "before the chain starts, but a chain that merges identical haplotypes after burn-in ends up with fewer than "
                         "-g, can no longer follow the file and stops with that message after the run: give the -g the other run kept "
                         "(extension)")
    ap.add_argument('--diagnose', nargs='?', const=True, default=None, type=int, metavar='L',
                    help="also write convergence diagnostics of the stored iterations: Tau_MCSE.csv (Monte Carlo standard error of "
                         "Tau_Mean.csv by batch means), Tau_diag.csv (per position and haplotype: smallest effective sample size, "
                         "largest split R-hat, number of base changes) and Diag_scalars.csv (lp, ll, every gamma entry); L = batch "
                         "length (default floor(sqrt(iterations))), at least 2 L iterations are needed; with --relabel / --relabel-ref "
                         "the diagnostics are those of the relabelled trace (extension)")
    ap.add_argument('--check', action='store_true',
                    help="also write the posterior predictive fit of the stored iterations: Fit_samples.csv and Fit_positions.csv "
                         "(per sample / per position: non-empty cells, posterior mean of Pearson's X2, its expectation under the "
                         "model, the standardised discrepancy z and the deviance); a large z marks a sample or a position the "
                         "haplotypes do not explain; z is a conservative score, not a p-value: --check-reps gives one (extension)")
    ap.add_argument('--check-reps', dest='check_reps', nargs='?', const=CHECK_REPS, default=None, type=int, metavar='R',
                    help="with --check: also write posterior predictive p-values, Fit_samples_ppp.csv and Fit_positions_ppp.csv (per "
                         "sample / per position: T_obs, the posterior mean of Pearson's X2 summed over the other index; T_rep and "
                         "T_rep_sd, the same on R replicate tables drawn from the model at every used iteration (default %d: a "
                         "convention, not tuned); p, the share of replicates at least as extreme as the data; p_mcse, its Monte Carlo "
                         "standard error by batch means over iterations; for positions also q, the Benjamini-Hochberg q-value).  "
                         "Unlike z, p is on a probability scale, and uniform when the parameters are known; at fitted parameters "
                         "posterior predictive p-values are themselves conservative, because the data are used twice (extension)"
                         % CHECK_REPS)
    ap.add_argument('--check-stride', dest='check_stride', default=None, type=int, metavar='K',
                    help="with --check-reps: use every K-th stored iteration (default: about %d evenly spaced ones, as --predictive "
                         "does) (extension)" % CHECK_N_USE)
    ap.add_argument('--check-cells', dest='check_cells', action='store_true',
                    help="with --check: also write Fit_cells.csv, positions x samples, the posterior mean X2 of every cell (extension)")
    ap.add_argument('--predictive', nargs='?', const=50, default=None, type=int, metavar='N',
                    help="also write the position-marginal predictive density of the chain, for choosing -g: Predictive_positions.csv "
                         "(per position: lppd, p_waic, elpd_waic with the haplotype bases summed out; kind `fit` = WAIC of the fitted "
                         "positions, with -r also kind `heldout` = the log predictive density of the positions left out of the fit) and "
                         "Predictive_summary.csv; from N evenly spaced stored iterations (default 50, a convention); -g up to 10; "
                         "compare runs with `python -m desman_amd.predictive compare` (extension)")
    ap.add_argument('--marginals', action='store_true',
                    help="also write the Rao-Blackwellised posterior of the haplotype bases from the stored iterations: Tau_Mean_rb.csv "
                         "(the layout of Tau_Mean.csv; the average of each base's exact conditional probability instead of the average "
                         "of the sampled bases: finer than 1/iterations, and not 0 or 1 merely because a base never flipped), "
                         "Tau_rb_MCSE.csv (its Monte Carlo standard error by batch means; batch length as --diagnose [L]) and "
                         "Tau_calls.csv (per position and haplotype: the most probable base, its probability, the base of Tau_star, "
                         "whether they agree, the entropy); with --relabel / --relabel-ref under that relabelling (extension)")
    ap.add_argument('--marginal-pairs', dest='marginal_pairs', nargs='?', const=True, default=None, type=int, metavar='K',
                    help="with --marginals (implied): also write the Rao-Blackwellised JOINT posterior of the bases of every two "
                         "haplotypes, from every K-th stored iteration: SND_rb.csv (per pair: the expected number of positions at which "
                         "they differ, its Monte Carlo standard error, the share of positions that probably differ, the distance in "
                         "Tau_star) and Tau_pairs.csv (per position and pair with a doubtful call in Tau_calls.csv: the most probable "
                         "two bases, P(same base), the mass that only asks which of the two carries which base, the mutual information, "
                         "and kind = phase where the data know the two bases but not their owners, else base); without K the largest "
                         "stride that still uses max(50, two batches) iterations: K = max(1, iterations // max(50, 2 L)), L the batch "
                         "length of --diagnose [L]; -g at least 2 (extension)")
    ap.add_argument('--pair-moves', dest='pair_moves', nargs='?', const=PAIR_MOVES, default=None, type=int, metavar='E',
                    help="add joint moves of two haplotypes to the Gibbs chain, burn-in and sampling alike: the sweep of every E-th "
                         "iteration (default %d: a convention, not tuned) is followed by a pass that redraws the bases of every pair of "
                         "haplotypes of a position from their 16-state conditional, so two haplotypes that carry each other's bases can "
                         "swap them; the chain's law is unchanged; not for replicate chains that share their launches (extension)"
                         % PAIR_MOVES)
    return ap


def _pair_moves_options(opts, replicates=False):
    """--pair-moves: refused here, before any chain, where it cannot be served; returns the pair_every of the sampler (0 = off)"""
    if opts.pair_moves is None:
        return 0
    if replicates:
        sys.exit("desman: --pair-moves is not available for replicate chains that share their launches: run the chains one by one")
    if opts.pair_moves < 1:
        sys.exit("desman: --pair-moves: a pair pass every E-th iteration needs E >= 1; got %d" % opts.pair_moves)
    return opts.pair_moves


_TABLES_LOCK = threading.Lock()
_TABLES_CACHE = {}                      # (path, mtime, size) -> parsed frame, the most recent few


def _read_table(path):
    """the base-count table of `path`, parsed once per process while the file is unchanged: a G-sweep runs every chain through
    main() / main_replicates() in one process (desman_amd.chains), and parsing a 50 000 x 96 table (58 MB of text) costs more than
    the chain's GPU time.  The frame is only ever read (Variant_Filter copies it into arrays, Output_Results slices it)."""
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_mtime_ns, st.st_size)
    with _TABLES_LOCK:
        table = _TABLES_CACHE.get(key)
        if table is None:
            table = pd.read_csv(path, header=0, index_col=0)
            while len(_TABLES_CACHE) >= 2:
                _TABLES_CACHE.pop(next(iter(_TABLES_CACHE)))
            _TABLES_CACHE[key] = table
    return table


def _load(opts, report):
    """CSV -> count tensor, sample filter, optional variant filter / eta file / position subsample."""
    logging.info('position-selection RNG seeded with %d' % POSITION_SELECT_SEED)
    table = _read_table(opts.variant_file)
    flt = Variant_Filter(table, randomState=RandomState(POSITION_SELECT_SEED), optimise=opts.optimiseP,
                         threshold=opts.filter_variants, min_coverage=opts.min_coverage, qvalue_cutoff=opts.max_qvalue)
    flt.device = opts.device
    if flt.S < 1 or flt.V < 1:
        logging.error('nothing to do: %d samples above the coverage cut, %d positions' % (flt.S, flt.V))
        sys.exit()
    logging.info('%d samples, %d positions, %d haplotypes requested' % (flt.S, flt.V, opts.genomes))
    if opts.filter_variants is not None:
        logging.info('variant filter: optimise=%s threshold=%s min_coverage=%s q<=%s min_freq=%s'
                     % (opts.optimiseP, opts.filter_variants, opts.min_coverage, opts.max_qvalue, opts.min_variant_freq))
        flt.get_filtered_VariantsLogRatio()                       # lrt_kernel on the GPU
        logging.info('variant filter kept %d positions' % flt.NS)
    if opts.eta_file is not None:
        logging.info('initial error matrix read from %s' % opts.eta_file)
        flt.eta = pd.read_csv(opts.eta_file, header=0, index_col=0).to_numpy()
    subsample = opts.random_select
    if subsample is not None:
        if subsample < flt.V:
            logging.info('fitting on %d random positions' % subsample)
            flt.select_Random(subsample)
        else:
            logging.info('only %d positions: the -r subsample of %d is ignored' % (flt.V, subsample))
            subsample = None
    return table, flt, subsample


def _fit(opts, flt, pair_every=0):
    """NMF-tensor initialisation, burn-in, degenerate-haplotype merge, sampling (bin/desman:129-153)."""
    logging.info('sampler seed %d', opts.random_seed)
    rng = RandomState(opts.random_seed)
    sampletau.initRNG()
    sampletau.setRNG(opts.random_seed)
    nmft = Init_NMFT(flt.snps_filter, opts.genomes, rng, device=opts.device)
    logging.info('NMF-tensor initialisation')
    nmft.factorize()
    chain = HaploSNP_Sampler(flt.snps_filter, opts.genomes, rng, max_iter=opts.no_iter, device=opts.device,
                             ctx=nmft._ctx,                        # same resident count tensor
                             pair_every=pair_every)
    chain.tau = np.copy(nmft.get_tau(), order='C')
    chain.updateTauIndices()
    chain.gamma = np.copy(nmft.get_gamma(), order='C')
    chain.eta = np.copy(flt.eta, order='C')
    logging.info('Gibbs burn-in')
    chain.update()
    chain.removeDegenerate()
    logging.info('Gibbs sampling')
    chain.update()
    return chain


# result tables of a fitted chain: (writer method of Output_Results, attribute or method of the sampler)
_TABLES = (("output_Filtered_Tau", "tau_star"), ("output_Tau_Mean", "tauMean"), ("output_Gamma", "gamma_star"),
           ("output_Gamma_Mean", "gammaMean"), ("output_Eta", "eta_star"), ("output_Eta_Mean", "etaMean"))


def _report(report, table, flt, chain, requested):
    report.set_Variants(table)
    report.set_Variant_Filter(flt)
    report.set_haplo_SNP(chain, requested)
    for writer, source in _TABLES:
        value = getattr(chain, source)
        getattr(report, writer)(value() if callable(value) else value)
    report.output_Selected_Variants()


def _relabel_reference(opts, table, flt):
    """--relabel-ref: the other run's haplotypes as [V, G] digits, checked against the positions this run is about to fit and against
    -g; the run stops here, before any chain, if the file does not fit.  None without the option."""
    if opts.relabel_ref is None:
        return None
    from . import relabel
    if not os.path.isfile(opts.relabel_ref):
        sys.exit("desman: can't open --relabel-ref file '%s'" % opts.relabel_ref)
    rows = np.asarray(flt.selected_indices, dtype=np.int64)
    names = table.index.to_numpy()[rows]
    positions = table['Position'].to_numpy()[rows]
    try:
        return relabel.read_reference(opts.relabel_ref, positions, names, opts.genomes)
    except ValueError as e:
        sys.exit("desman: --relabel-ref: %s" % e)


def _report_relabel(report, chain, ref):
    """--relabel: the relabelled summaries of the fitted chain, next to the usual files (which do not change)"""
    if ref is not None and ref.shape[1] != chain.G:
        sys.exit("desman: --relabel-ref: the chain kept %d of the %d haplotypes after merging identical ones; the reference has %d"
                 % (chain.G, ref.shape[1], ref.shape[1]))
    chain.relabel_ref = ref
    report.output_Relabel(chain.relabelling())
    report.output_Tau_Mean_relabelled(chain.tauMeanRelabelled())
    report.output_Gamma_Mean_relabelled(chain.gammaMeanRelabelled())
    report.output_SND_posterior(chain.sndPosterior())
    report.output_Haplotype_stability(chain.haplotypeStability())


def _stored_iterations(opts):
    """the iterations the chain of this run will store"""
    return DEFAULT_ITER if opts.no_iter is None else opts.no_iter


def _batch_len(opts, flag):
    """the batch length of `flag` (--diagnose, --marginals) -- the L of --diagnose [L] where one is given, else floor(sqrt(iterations))
    -- checked against the iterations a chain will store; the run stops here, before any chain, if there are fewer than 2 L of them"""
    from . import diagnose
    n = _stored_iterations(opts)
    given = opts.diagnose is not None and opts.diagnose is not True          # a bare --diagnose parses as True, --diagnose L as the int
    L = opts.diagnose if given else diagnose.default_batch_len(n)
    if L < 1:
        sys.exit("desman: %s: the batch length must be at least 1; got %d" % (flag, L))
    if n < 2 * L:
        sys.exit("desman: %s: %d stored iterations (-i) are fewer than two batches of %d" % (flag, n, L))
    return L


def _diagnose_batch_len(opts):
    """--diagnose: the batch length L of its files.  None without the option."""
    return None if opts.diagnose is None else _batch_len(opts, "--diagnose")


def _marginals_batch_len(opts):
    """--marginals (--marginal-pairs implies it): the batch length of Tau_rb_MCSE.csv.  None without the option."""
    return _batch_len(opts, "--marginals") if opts.marginals or opts.marginal_pairs is not None else None


def _marginal_pairs_stride(opts):
    """--marginal-pairs [K]: the stride K of a run whose options _marginal_pairs_options has accepted -- the K given or, for a bare
    flag, marginals.pairs_stride of the stored iterations and the batch length.  None without the option."""
    if opts.marginal_pairs is None:
        return None
    if opts.marginal_pairs is not True:                          # a bare flag parses as True, --marginal-pairs K as the int
        return opts.marginal_pairs
    from . import marginals
    return marginals.pairs_stride(_stored_iterations(opts), _batch_len(opts, "--marginals"))


def _marginal_pairs_options(opts):
    """--marginal-pairs [K]: refused here, before any chain, where --marginals is, for fewer than two haplotypes and for a K that leaves
    fewer than two batches.  (The stride is not handed on with the batch lengths: what _extension_options returns is three keys, and
    _marginal_pairs_stride costs nothing.)"""
    if opts.marginal_pairs is None:
        return
    L = _batch_len(opts, "--marginals")
    n = _stored_iterations(opts)
    if opts.genomes < 2:
        sys.exit("desman: --marginal-pairs: a pair needs two haplotypes; got -g %d" % opts.genomes)
    K = _marginal_pairs_stride(opts)
    if K < 1:
        sys.exit("desman: --marginal-pairs: every K-th stored iteration needs K >= 1; got %d" % K)
    if -(-n // K) < 2 * L:
        sys.exit("desman: --marginal-pairs: every %d-th of %d stored iterations (-i) are fewer than two batches of %d" % (K, n, L))


def _report_diagnose(report, chain, L):
    """--diagnose: the convergence diagnostics of the fitted chain, next to the usual files (which do not change); under the
    relabelling of --relabel / --relabel-ref where one was made"""
    report.output_Tau_MCSE(chain.tauMCSE(L))
    report.output_Tau_diag(chain.tauDiagnostics(L))
    report.output_Diag_scalars(chain.scalarDiagnostics(L))


def _report_marginals(report, chain, L):
    """--marginals: the Rao-Blackwellised tau marginals of the fitted chain, next to the usual files (which do not change); under the
    relabelling of --relabel / --relabel-ref where one was made"""
    report.output_Tau_marginals(chain.tauMarginals(L), relabelled=chain._diag_perm() is not None)


def _report_marginal_pairs(report, chain, L, K):
    """--marginal-pairs: the joint posterior of every two haplotypes' bases, next to the files of --marginals (which do not change);
    under the same relabelling.  A chain that merged its haplotypes down to one has no pair."""
    if chain.G < 2:
        logging.info("--marginal-pairs: the chain kept one haplotype after merging identical ones: no pair, no file")
        return
    report.output_Tau_pairs(chain.tauPairs(L, K))


def _check_options(opts, replicates=False):
    """--check / --check-cells / --check-reps / --check-stride: refused here, before any chain, where they cannot be served"""
    if opts.check_cells and not opts.check:
        sys.exit("desman: --check-cells needs --check")
    if opts.check_reps is not None and not opts.check:
        sys.exit("desman: --check-reps needs --check")
    if opts.check_stride is not None and opts.check_reps is None:
        sys.exit("desman: --check-stride needs --check-reps")
    if opts.check and opts.no_iter is not None and opts.no_iter < 1:
        sys.exit("desman: --check: %d stored iterations (-i): at least 1 is needed" % opts.no_iter)
    if opts.check_reps is not None:
        if replicates:
            sys.exit("desman: --check-reps is not available for replicate chains that share their launches: run the chains one by one")
        if opts.check_reps < 1 or opts.check_reps > CHECK_MAX_REPS:
            sys.exit("desman: --check-reps: 1 to %d replicates per iteration; got %d" % (CHECK_MAX_REPS, opts.check_reps))
        if opts.check_stride is not None and opts.check_stride < 1:
            sys.exit("desman: --check-stride: at least 1; got %d" % opts.check_stride)


def _report_check(report, chain, cells):
    """--check: the fit of the chain per sample and per position (--check-cells: per cell too), next to the usual files (which do not
    change); the statistic does not depend on the haplotype labels, so --relabel changes nothing here"""
    fit = chain.fitCheck(cells=cells)
    report.output_Fit(fit[0], fit[1])
    if cells:
        report.output_Fit_cells(fit[2])


def _report_check_reps(report, chain, reps, stride):
    """--check --check-reps: posterior predictive p-values per sample and per position from replicate tables, next to the files of
    --check (which do not change); p_b does not depend on the haplotype labels, so --relabel changes nothing here either"""
    samples, positions = chain.fitReplicates(reps=reps, stride=stride)
    report.output_Fit_ppp(samples, positions)


def _predictive_options(opts, replicates=False):
    """--predictive: refused here, before any chain, where it cannot be served"""
    if opts.predictive is None:
        return
    from . import predictive
    if replicates:
        sys.exit("desman: --predictive is not available for replicate chains that share their launches: run the chains one by one")
    if opts.predictive < 1:
        sys.exit("desman: --predictive: at least 1 stored iteration must be used; got %d" % opts.predictive)
    if opts.genomes > predictive.MAX_G:
        sys.exit("desman: --predictive sums over all 4^G haplotype states of a position: -g %d is above %d" % (opts.genomes, predictive.MAX_G))
    if opts.no_iter is not None and opts.no_iter < 1:
        sys.exit("desman: --predictive: %d stored iterations (-i): at least 1 is needed" % opts.no_iter)


def _report_predictive(report, flt, chain, n_use, subsample):
    """--predictive: the fitted positions scored on the chain's resident table (WAIC) and, with -r, the positions left out of the fit --
    the rows _assign_rest takes -- scored under the same traces (held-out log predictive density); next to the usual files, which do
    not change"""
    from . import predictive
    fit = chain.predictive(n_use)
    rest = None
    if subsample is not None:
        rest = chain.predictive(n_use, counts=flt.snps_filter_original[~np.asarray(flt.selected, dtype=bool), :])
    summary = {"fit": predictive.summary(fit)}
    if rest is not None:
        summary["heldout"] = predictive.summary(rest)
    report.output_Predictive(fit, rest, summary)


def _extension_options(opts, replicates=False):
    """every extension option of a run, refused here, before any chain, where it cannot be served (replicates: for replicate chains
    that share their launches); returns what the fit and the reports need of them"""
    pair_every = _pair_moves_options(opts, replicates)
    diag_len = _diagnose_batch_len(opts)
    marg_len = _marginals_batch_len(opts)
    _marginal_pairs_options(opts)
    _check_options(opts, replicates)
    _predictive_options(opts, replicates)
    return dict(pair_every=pair_every, diag_len=diag_len, marg_len=marg_len)


def _report_extensions(opts, ext, report, flt, chain, ref, subsample):
    """the reports of every extension option of the run, for a fitted chain (ext: of _extension_options; ref: of _relabel_reference)"""
    if opts.relabel or ref is not None:
        _report_relabel(report, chain, ref)
    if ext["diag_len"] is not None:
        _report_diagnose(report, chain, ext["diag_len"])
    if ext["marg_len"] is not None:
        _report_marginals(report, chain, ext["marg_len"])
    if opts.marginal_pairs is not None:
        _report_marginal_pairs(report, chain, ext["marg_len"], _marginal_pairs_stride(opts))
    if opts.check:
        _report_check(report, chain, opts.check_cells)
    if opts.check_reps is not None:
        _report_check_reps(report, chain, opts.check_reps, opts.check_stride)
    if opts.predictive is not None:
        _report_predictive(report, flt, chain, opts.predictive, subsample)


def _rest_nmft(opts, flt, chain):
    """-r: the positions left out of the fit and their NMFT with the fitted chain's gamma held (not yet factorized)"""
    rest = flt.snps_filter_original[~np.asarray(flt.selected, dtype=bool), :]
    nmft = Init_NMFT(rest, chain.G, chain.randomState, device=opts.device)
    nmft.gamma = np.transpose(chain.gamma)
    logging.info('NMF-tensor initialisation of the %d remaining positions (gamma fixed)' % rest.shape[0])
    return rest, nmft


def _rest_sampler(opts, chain, rest, nmft):
    """-r: the tau-only sampler of `rest` on the context of its factorized NMFT, with the fitted chain's means and stores"""
    other = HaploSNP_Sampler(rest, chain.G, chain.randomState, max_iter=opts.no_iter, device=opts.device, ctx=nmft._ctx)
    other.tau = nmft.get_tau()
    other.updateTauIndices()
    other.gamma_star = np.copy(chain.gammaMean(), order='C')
    other.eta_star = np.copy(chain.etaMean(), order='C')
    other.gamma_store = np.copy(chain.gamma_store, order='C')
    other.eta_store = np.copy(chain.eta_store, order='C')
    return other


def _assign_rest(opts, report, table, flt, chain):
    """-r: haplotypes of the positions left out of the fit, with tau-only sweeps driven by the fitted
    chain's gamma / eta traces (bin/desman:181-206)."""
    rest, nmft = _rest_nmft(opts, flt, chain)
    nmft.factorize_tau()
    other = _rest_sampler(opts, chain, rest, nmft)
    for phase in ('burn-in', 'sampling'):
        logging.info('tau-only %s' % phase)
        other.updateTau()
    report.outPredFit(other, opts.genomes)
    report.output_collated_Tau(other, table)


def _assign_rest_batch(runs, tell):
    """_assign_rest of several replicate chains with their NMF fits and tau-only sweeps batched (equal shapes assumed)"""
    others, starts = [], []
    for k, r in enumerate(runs):
        tell(k)
        starts.append(_rest_nmft(r["opts"], r["flt"], r["chain"]))
    Init_NMFT.factorize_tau_batch([nmft for _, nmft in starts])
    for k, (r, (rest, nmft)) in enumerate(zip(runs, starts)):
        tell(k)
        nmft._log_trace(nmft.div_trace)
        other = _rest_sampler(r["opts"], r["chain"], rest, nmft)
        other.mt_state = r["chain"].mt_state                     # the tau-only sweeps continue the chain's GSL stream
        others.append(other)
    for phase in ('burn-in', 'sampling'):
        for k in range(len(runs)):
            tell(k)
            logging.info('tau-only %s' % phase)
        HaploSNP_Sampler.updateTau_batch(others, on_chain=lambda o: tell(others.index(o)))
    for k, (r, other) in enumerate(zip(runs, others)):
        tell(k)
        r["report"].outPredFit(other, r["opts"].genomes)
        r["report"].output_collated_Tau(other, r["table"])


def main(argv=None):
    opts = build_parser().parse_args(argv)
    if opts.assign_file is not None:
        # upstream this branch stops in ipdb.set_trace() after the whole run (bin/desman:213-214): there is nothing
        # to mirror, and the user should not pay for NMFT + 2 x no_iter Gibbs iterations to learn it
        sys.exit('desman: -a/--assign_file is not supported (dead in the reference: bin/desman:213-214)')
    if opts.eta_file is not None and not os.path.isfile(opts.eta_file):
        sys.exit("desman: can't open eta file '%s'" % opts.eta_file)
    if opts.genomes < 0:
        logging.error('the haplotype number must be positive, got %d' % opts.genomes)
        sys.exit(-1)
    ext = _extension_options(opts)
    report = Output_Results(opts.output_dir)
    table, flt, subsample = _load(opts, report)
    ref = _relabel_reference(opts, table, flt)
    chain = _fit(opts, flt, ext["pair_every"])
    _report(report, table, flt, chain, opts.genomes)
    _report_extensions(opts, ext, report, flt, chain, ref, subsample)
    if subsample is not None:
        _assign_rest(opts, report, table, flt, chain)
    sampletau.freeRNG()


def main_replicates(argv_list, on_chain=None):
    """The `desman` runs of several replicate chains (argv lists that differ in -s / -o only) with their Gibbs iterations
    batched: one set of kernel launches per iteration for all of them (HaploSNP_Sampler.update_batch).  Loading, the NMF
    start, the degenerate-haplotype merge and the result files are per chain, as in main(); replicates whose haplotype
    counts differ after the merge finish one by one.  ``on_chain(k)`` is called before chain k's own work (log routing).
    The mu/E pass of a batch is the aggregated sampler whatever the table size, so a chain's draws are those of a
    single run only where that run takes the aggregated pass too (same law either way)."""
    from . import _lib
    tell = on_chain if on_chain is not None else (lambda k: None)
    runs = []
    for k, argv in enumerate(argv_list):
        tell(k)
        opts = build_parser().parse_args(argv)
        if opts.assign_file is not None:
            sys.exit('desman: -a/--assign_file is not supported (dead in the reference: bin/desman:213-214)')
        ext = _extension_options(opts, replicates=True)      # (--pair-moves, --check-reps and --predictive are refused)
        report = Output_Results(opts.output_dir)
        table, flt, subsample = _load(opts, report)
        logging.info('sampler seed %d', opts.random_seed)
        rng = RandomState(opts.random_seed)
        nmft = Init_NMFT(flt.snps_filter, opts.genomes, rng, device=opts.device)
        runs.append(dict(opts=opts, report=report, table=table, flt=flt, subsample=subsample, rng=rng, nmft=nmft,
                         ref=_relabel_reference(opts, table, flt), ext=ext))
    # the NMF starts: together where the batched kernels apply (one shape, S <= 128, G <= 16), else one by one
    nm = [r["nmft"] for r in runs]
    done = False
    if len(nm) > 1 and len({(o.V, o.S, o.G) for o in nm}) == 1:
        try:
            Init_NMFT.factorize_batch(nm)
            done = True
        except _lib.DesmanHipError as e:
            logging.info('batched NMF start not available (%s): one by one' % e)
    for k, r in enumerate(runs):
        tell(k)
        logging.info('NMF-tensor initialisation')
        if done:
            r["nmft"]._log_trace(r["nmft"].div_trace)
        else:
            r["nmft"].factorize()
    for k, r in enumerate(runs):
        opts, flt, rng, nmft = r["opts"], r["flt"], r["rng"], r["nmft"]
        chain = HaploSNP_Sampler(flt.snps_filter, opts.genomes, rng, max_iter=opts.no_iter, device=opts.device, ctx=nmft._ctx)
        # (a chain's mu/E specification is its own in a batch too -- round 5 -- so a replicate that ends up alone, because its haplotype
        # count changed in removeDegenerate or its batched unit failed, draws what it would have drawn in the batch)
        chain.mt_state = _lib.mt_seed_state(opts.random_seed)       # what initRNG(); setRNG(seed) leave in the module's stream
        chain.tau = np.copy(nmft.get_tau(), order='C')
        chain.updateTauIndices()
        chain.gamma = np.copy(nmft.get_gamma(), order='C')
        chain.eta = np.copy(flt.eta, order='C')
        r["chain"] = chain
    chains = [r["chain"] for r in runs]

    def together(group):
        shapes = {(c.V, c.S, c.G) for c in group}
        if len(group) > 1 and len(shapes) == 1:
            HaploSNP_Sampler.update_batch(group, on_chain=lambda c: tell(chains.index(c)))
        else:
            for c in group:
                tell(chains.index(c))
                c.update()
    for k in range(len(runs)):
        tell(k)
        logging.info('Gibbs burn-in (batch of %d chains)' % len(runs))
    together(chains)
    for k, c in enumerate(chains):
        tell(k)
        c.removeDegenerate()
        logging.info('Gibbs sampling')
    by_g = {}
    for c in chains:
        by_g.setdefault(c.G, []).append(c)
    for group in by_g.values():
        together(group)
    for k, r in enumerate(runs):
        tell(k)
        _report(r["report"], r["table"], r["flt"], r["chain"], r["opts"].genomes)
        _report_extensions(r["opts"], r["ext"], r["report"], r["flt"], r["chain"], r["ref"], r["subsample"])
    # -r: the positions left out of the fit -- batched where the replicates still agree in shape
    rest_runs = [r for r in runs if r["subsample"] is not None]
    idx = {id(r): k for k, r in enumerate(runs)}
    groups = {}
    for r in rest_runs:
        n_rest = int((~np.asarray(r["flt"].selected, dtype=bool)).sum())
        groups.setdefault((r["chain"].G, n_rest, r["chain"].S), []).append(r)
    for group in groups.values():
        batched = False
        if len(group) > 1:
            # whatever the batched attempt drew from the chains' numpy streams before it gave up is handed back
            states = [r["chain"].randomState.get_state() for r in group]
            try:
                _assign_rest_batch(group, lambda j, g=group: tell(idx[id(g[j])]))
                batched = True
            except _lib.DesmanHipError as e:
                for r, st in zip(group, states):
                    r["chain"].randomState.set_state(st)
                logging.info('batched -r path not available (%s): one by one' % e)
        if not batched:
            for r in group:
                tell(idx[id(r)])
                sampletau.initRNG()
                sampletau.setRNGState(r["chain"].mt_state)          # the tau-only sweeps continue the chain's GSL stream
                _assign_rest(r["opts"], r["report"], r["table"], r["flt"], r["chain"])
                sampletau.freeRNG()
    return chains


if __name__ == "__main__":
    main()
