"""Result files of a `desman` run -- the on-disk half of the drop-in contract.

Same class / method names as desman/Output_Results.py (the driver and downstream scripts call them) and
byte-identical files (tests/test_host_cpu.py compares against files the reference class wrote); inside,
everything goes through two small helpers: one for haplotype tables (Position first, then 4 columns per
haplotype), one for per-sample abundance tables.
"""
import hashlib
import logging
import os
import shutil
import sys
import threading
import weakref

import numpy as np
import pandas as pd

_SELECTED_LOCK = threading.Lock()
_SELECTED_CACHE = {}        # (id of the table, rows, digest of the selection) -> (weak ref to the table, a file holding the text, its size)

LOG_FORMAT = '%(asctime)s:%(levelname)s:%(name)s:%(message)s'


def _table_bytes(flat, names, positions):
    """The text pandas' ``DataFrame.to_csv`` writes for a haplotype table (index = names, a Position column, then the columns
    0..n-1 of ``flat``), assembled without a Python-level loop over cells -- or None where that text is not plain enough to be
    assembled this way (the caller then lets pandas write it).  A table of a chain has few distinct values (0 / 1, or k / n_iter),
    so each distinct value is formatted once, exactly as pandas formats it (numpy's shortest round-trip text), and the cells are
    gathered as fixed-width byte fields whose padding is squeezed out at the end: V = 50k, G = 12 in 0.3 s instead of 2.9 s
    (Tau_Mean.csv) -- next to a GPU fit of about 2 s, the result files were a third of a chain's wall time."""
    flat = np.asarray(flat)
    pos = np.asarray(positions)
    if flat.ndim != 2 or flat.dtype.kind not in "iuf" or pos.dtype.kind not in "iu" or flat.shape[0] != len(names) or not flat.size:
        return None
    if flat.dtype.kind == "f" and (flat.dtype != np.float64 or not np.isfinite(flat).all()):
        return None
    if not all(type(n) is str and n and n.isascii() and not any(c in n for c in ',"\r\n\0') for n in names):
        return None                                       # (a non-ASCII contig name has no 'S' form: pandas writes it)
    n, nc = flat.shape
    if flat.dtype.kind == "f":                            # by bit pattern: 0.0 and -0.0 print differently
        inv, uniq = pd.factorize(np.ascontiguousarray(flat, dtype=np.float64).ravel().view(np.int64))
        uniq = np.asarray(uniq).view(np.float64)
    else:
        inv, uniq = pd.factorize(flat.ravel())
    if len(uniq) > 65536:
        return None
    as_bytes = lambda a: np.array(np.asarray(a).astype(str).tolist(), dtype="S")     # minimal field width
    ustr, nm, ps = as_bytes(uniq), np.array(list(names), dtype="S"), as_bytes(pos)
    k, kn, kp = ustr.dtype.itemsize, nm.dtype.itemsize, ps.dtype.itemsize
    row = np.zeros((n, kn + 1 + kp + 1 + nc * (k + 1)), dtype=np.uint8)
    row[:, :kn] = nm.view(np.uint8).reshape(n, kn)
    row[:, kn] = ord(",")
    row[:, kn + 1:kn + 1 + kp] = ps.view(np.uint8).reshape(n, kp)
    row[:, kn + 1 + kp] = ord(",")
    cells = row[:, kn + kp + 2:].reshape(n, nc, k + 1)
    cells[:, :, :k] = ustr[inv.reshape(n, nc)].view(np.uint8).reshape(n, nc, k)
    cells[:, :, k] = ord(",")
    cells[:, -1, k] = ord("\n")
    header = (",Position," + ",".join(str(i) for i in range(nc)) + "\n").encode()
    return header + row[row != 0].tobytes()


def rchop(text, suffix):
    return text[:-len(suffix)] if text.endswith(suffix) else text


class Output_Results:

    def __init__(self, outputDir):
        self.outputDir = outputDir
        os.makedirs(outputDir, exist_ok=True)
        self.log_file_name = outputDir + "/log_file.txt"
        logging.basicConfig(filename=self.log_file_name, level=logging.INFO, filemode='w', format=LOG_FORMAT)
        here = os.path.abspath(self.outputDir)
        logging.info("Results created in {0}".format(here))
        print("Up and running. Check {0} for progress".format(os.path.abspath(self.log_file_name)), file=sys.stderr)

    # ---- wiring
    def set_Variants(self, variants):
        self.variants = variants
        self.contig_names = variants.index.tolist()
        self.position = variants['Position']

    def set_Variant_Filter(self, variantFilter):
        self.variantFilter = variantFilter
        keep = variantFilter.selected_indices
        self.filtered_contig_names = [self.contig_names[i] for i in keep]
        self.filtered_position = self.position.to_numpy()[np.asarray(keep, dtype=np.int64)]

    def _path(self, name):
        return self.outputDir + "/" + name

    # ---- fit statistics: Fit,<G requested>,<G kept>,<lp*>,<mean deviance>
    def _write_fit(self, name, sampler, requested):
        line = "Fit,%d,%d,%f,%f\n" % (requested, sampler.G, sampler.lp_star, sampler.meanDeviance())
        with open(self._path(name), "w") as fh:
            fh.write(line)

    def set_haplo_SNP(self, haplo_SNP, genomes):
        self.haplo_SNP = haplo_SNP
        self._write_fit("fit.txt", haplo_SNP, genomes)
        logging.info("fit.txt written")

    def outPredFit(self, haplo_SNP, genomes):
        self._write_fit("fitP.txt", haplo_SNP, genomes)
        logging.info("fitP.txt written")

    # ---- haplotype tables
    def _haplotype_table(self, name, values, names, positions):
        """rows = positions, first column Position, then the flattened [G][4] block."""
        flat = np.reshape(values, (values.shape[0], -1))
        text = _table_bytes(flat, names, positions)
        if text is not None:
            with open(self._path(name), "wb") as fh:
                fh.write(text)
            return
        frame = pd.DataFrame(flat, index=names)
        frame['Position'] = positions
        order = frame.columns.tolist()
        frame[order[-1:] + order[:-1]].to_csv(self._path(name))

    def output_Filtered_Tau(self, tau):
        self._haplotype_table("Filtered_Tau_star.csv", np.reshape(tau, (self.haplo_SNP.V, self.haplo_SNP.G, 4)),
                              self.filtered_contig_names, self.filtered_position)
        logging.info("Filtered_Tau_star.csv written")

    def output_Tau_Mean(self, tauProb):
        self._haplotype_table("Tau_Mean.csv", np.reshape(tauProb, (self.haplo_SNP.V, self.haplo_SNP.G, 4)),
                              self.filtered_contig_names, self.filtered_position)
        logging.info("Tau_Mean.csv written")

    def output_collated_Tau(self, haplo_SNP_NS, full_variants):
        """-r: fitted and assigned positions merged back into input order."""
        total = haplo_SNP_NS.V + self.haplo_SNP.V
        G = self.haplo_SNP.G
        fitted = np.asarray(self.variantFilter.selected[:total], dtype=bool)
        star = np.zeros((total, G, 4), dtype=np.int64)
        prob = np.zeros((total, G, 4))
        star[fitted], star[~fitted] = self.haplo_SNP.tau_star, haplo_SNP_NS.tau_star
        prob[fitted], prob[~fitted] = self.haplo_SNP.probabilisticTau(), haplo_SNP_NS.probabilisticTau()
        all_names = full_variants.index.tolist()
        all_pos = full_variants['Position']
        rows = self.variantFilter.selected_indices_original
        names = [all_names[i] for i in rows]
        positions = all_pos.to_numpy()[np.asarray(rows, dtype=np.int64)]
        self._haplotype_table("Collated_Tau_star.csv", star, names, positions)
        self._haplotype_table("Collated_Tau_mean.csv", prob, names, positions)
        logging.info("Collated_Tau_star.csv / Collated_Tau_mean.csv written")

    # ---- abundance and error tables
    def _kept_sample_names(self):
        cols = self.variants.columns.values.tolist()
        n_samples = (len(cols) - 1) // 4
        every = [rchop(cols[1 + 4 * k], '-A') for k in range(n_samples)]
        return [every[k] for k in self.variantFilter.sample_indices]

    def _abundance_table(self, name, gamma):
        pd.DataFrame(gamma, index=self._kept_sample_names()).to_csv(self._path(name))
        logging.info(name + " written")

    def output_Gamma(self, gamma):
        self._abundance_table("Gamma_star.csv", gamma)

    def output_Gamma_Mean(self, gamma):
        self._abundance_table("Gamma_mean.csv", gamma)

    def output_Eta(self, eta):
        pd.DataFrame(eta).to_csv(self._path("Eta_star.csv"))
        logging.info("Eta_star.csv written")

    def output_Eta_Mean(self, eta):
        pd.DataFrame(eta).to_csv(self._path("Eta_mean.csv"))
        logging.info("Eta_mean.csv written")

    # ---- `desman --relabel`: the summaries with every stored iteration's labels matched to a reference (desman_amd/relabel.py)
    def output_Relabel(self, rel):
        """Relabel.csv: one row per stored iteration -- the summed distance to the reference under the iteration's own labels and under
        the best relabelling, whether the two differ in labels, and the relabelling itself (haplotype g -> label, space separated)"""
        perm = np.asarray(rel["perm"], dtype=np.int64)
        switched = (perm != np.arange(perm.shape[1])[None, :]).any(axis=1).astype(np.int64)
        frame = pd.DataFrame({"iter": np.arange(perm.shape[0]), "cost_identity": rel["cost_identity"], "cost_best": rel["cost_best"],
                              "switched": switched, "perm": [" ".join(str(x) for x in row) for row in perm]})
        frame.to_csv(self._path("Relabel.csv"), index=False)
        logging.info("Relabel.csv written: %d of %d stored iterations had switched labels" % (int(switched.sum()), perm.shape[0]))

    def output_Tau_Mean_relabelled(self, tauProb):
        self._haplotype_table("Tau_Mean_relabelled.csv", np.reshape(tauProb, (self.haplo_SNP.V, self.haplo_SNP.G, 4)),
                              self.filtered_contig_names, self.filtered_position)
        logging.info("Tau_Mean_relabelled.csv written")

    def output_Gamma_Mean_relabelled(self, gamma):
        self._abundance_table("Gamma_Mean_relabelled.csv", gamma)

    def output_SND_posterior(self, post):
        """SND_posterior.csv: per pair of haplotypes the posterior of their distance (positions that differ) and the MAP state's"""
        cols = [k for k in ("mean", "sd", "lo", "med", "hi", "map") if k in post]
        frame = pd.DataFrame({k: post[k] for k in cols})
        frame.insert(0, "h", post["pairs"][:, 1])
        frame.insert(0, "g", post["pairs"][:, 0])
        frame.to_csv(self._path("SND_posterior.csv"), index=False)
        logging.info("SND_posterior.csv written")

    def output_Haplotype_stability(self, stab):
        """Haplotype_stability.csv: per haplotype the mean and maximum fraction of positions that differ from the reference haplotype
        over the relabelled iterations, and in how many iterations its label had moved"""
        frame = pd.DataFrame({"haplotype": np.arange(len(stab["mean"])), "mean_diff": stab["mean"], "max_diff": stab["max"],
                              "moved": stab["moved"]})
        frame.to_csv(self._path("Haplotype_stability.csv"), index=False)
        logging.info("Haplotype_stability.csv written")

    # ---- `desman --diagnose`: convergence diagnostics of the stored iterations (desman_amd/diagnose.py)
    def output_Tau_MCSE(self, mcse):
        """Tau_MCSE.csv: the layout of Tau_Mean.csv, every cell the Monte Carlo standard error of that file's cell"""
        self._haplotype_table("Tau_MCSE.csv", np.reshape(mcse, (self.haplo_SNP.V, self.haplo_SNP.G, 4)),
                              self.filtered_contig_names, self.filtered_position)
        logging.info("Tau_MCSE.csv written")

    def output_Tau_diag(self, cells):
        """Tau_diag.csv: Contig, Position, then per haplotype g the columns ess_min_g, rhat_max_g, flips_g (HaploSNP_Sampler.tauDiagnostics),
        and one log line with the share of (position, haplotype) cells below diagnose.ESS_LOW or above diagnose.RHAT_HIGH"""
        from . import diagnose
        G = cells["ess_min"].shape[1]
        cols = {"Position": self.filtered_position}
        for g in range(G):
            cols["ess_min_%d" % g] = cells["ess_min"][:, g]
            cols["rhat_max_%d" % g] = cells["rhat_max"][:, g]
            cols["flips_%d" % g] = cells["flips"][:, g]
        frame = pd.DataFrame(cols, index=self.filtered_contig_names)
        frame.index.name = "Contig"
        frame.to_csv(self._path("Tau_diag.csv"))
        logging.info("Tau_diag.csv written: %.2f %% of %d (position, haplotype) cells have ess_min < %g or rhat_max > %g"
                     % (100.0 * diagnose.flagged_share(cells), cells["ess_min"].size, diagnose.ESS_LOW, diagnose.RHAT_HIGH))

    def output_Diag_scalars(self, diag):
        """Diag_scalars.csv: one row per scalar -- lp, ll, gamma_<sample>_<g> -- with mean, sd, mcse, ess, split_rhat"""
        names, samples = list(diag["names"]), self._kept_sample_names()
        G = (len(names) - 2) // max(len(samples), 1)
        names[2:] = ["gamma_%s_%d" % (s, g) for s in samples for g in range(G)]
        frame = pd.DataFrame({k: diag[k] for k in ("mean", "sd", "mcse", "ess", "split_rhat")}, index=names)
        frame.index.name = "scalar"
        frame.to_csv(self._path("Diag_scalars.csv"))
        logging.info("Diag_scalars.csv written")

    # ---- `desman --marginals`: Rao-Blackwellised tau marginals of the stored iterations (desman_amd/marginals.py)
    def output_Tau_marginals(self, marg, relabelled=False):
        """Tau_Mean_rb.csv (Tau_Mean_rb_relabelled.csv under a relabelling, as Tau_Mean.csv has Tau_Mean_relabelled.csv): the layout and
        row order of Tau_Mean.csv, every cell the average conditional probability of that base; Tau_rb_MCSE.csv: the layout of
        Tau_MCSE.csv, its Monte Carlo standard error; Tau_calls.csv: one row per (position, haplotype), position-major -- Contig, Position,
        haplotype, call, prob, star, agree, entropy (HaploSNP_Sampler.tauMarginals); and one log line with the expected number of wrong calls, the
        cells whose call has a probability below marginals.PROB_LOW and the dead cell-iterations"""
        from . import marginals
        V, G = self.haplo_SNP.V, self.haplo_SNP.G
        mean_name = "Tau_Mean_rb_relabelled.csv" if relabelled else "Tau_Mean_rb.csv"
        self._haplotype_table(mean_name, np.reshape(marg["p"], (V, G, 4)), self.filtered_contig_names, self.filtered_position)
        self._haplotype_table("Tau_rb_MCSE.csv", np.reshape(marg["mcse"], (V, G, 4)), self.filtered_contig_names, self.filtered_position)
        cells = marg["calls"]
        cols = {"Position": np.repeat(np.asarray(self.filtered_position), G), "haplotype": np.tile(np.arange(G), V)}
        for k in ("call", "prob", "star", "agree", "entropy"):
            cols[k] = np.reshape(cells[k], -1)
        frame = pd.DataFrame(cols, index=np.repeat(np.asarray(self.filtered_contig_names), G))
        frame.index.name = "Contig"
        frame.to_csv(self._path("Tau_calls.csv"))
        s = marg["summary"]
        logging.info("%s, Tau_rb_MCSE.csv, Tau_calls.csv written: %.2f of %d calls expected wrong, %d with probability below %g, "
                     "%d disagree with Tau_star, %d dead cell-iterations"
                     % (mean_name, s["expected_wrong"], s["cells"], s["low"], marginals.PROB_LOW, s["disagree"], s["dead"]))

    # ---- `desman --marginal-pairs`: the joint posterior of two haplotypes' bases (desman_amd/marginals.py)
    def output_Tau_pairs(self, pr):
        """SND_rb.csv: one row per pair -- g, h, dist (the expected number of positions at which the two differ), dist_mcse (batch
        means), differ (the share of positions with P(same base) < 0.5), star (the count distance of Tau_star); Tau_pairs.csv: one row
        per flagged (position, pair), position-major -- Contig, Position, g, h, pair (the most probable two bases, as letters), prob,
        p_same, swap, mi, kind (HaploSNP_Sampler.tauPairs); and one log line"""
        from . import marginals
        pairs = np.asarray(pr["pairs"])
        snd = pd.DataFrame({"g": pairs[:, 0], "h": pairs[:, 1], "dist": pr["dist"], "dist_mcse": pr["dist_mcse"], "differ": pr["differ"],
                            "star": pr["star_dist"]})
        snd.to_csv(self._path("SND_rb.csv"), index=False)
        v, p = np.nonzero(pr["flags"])
        t = pr["tables"]
        best = t["best"][v, p]
        letters = np.array(list("ACGT"))
        frame = pd.DataFrame({"Position": np.asarray(self.filtered_position)[v], "g": pairs[p, 0], "h": pairs[p, 1],
                              "pair": np.char.add(letters[best >> 2], letters[best & 3]), "prob": t["best_prob"][v, p],
                              "p_same": t["p_same"][v, p], "swap": t["swap"][v, p], "mi": t["mi"][v, p], "kind": t["kind"][v, p]},
                             index=np.asarray(self.filtered_contig_names)[v])
        frame.index.name = "Contig"
        frame.to_csv(self._path("Tau_pairs.csv"))
        kinds = t["kind"][v, p]
        near = int(np.argmin(pr["dist"])) if len(pairs) else -1
        logging.info("SND_rb.csv, Tau_pairs.csv written from every %d-th stored iteration: %d flagged (position, pair) rows (a call below %g), "
                     "%d of kind phase, %d of kind base; the closest pair is (%d, %d) at an expected distance of %.2f +- %.2f"
                     % (pr["stride"], len(v), marginals.PAIR_FLAG_LOW, int((kinds == "phase").sum()), int((kinds == "base").sum()),
                        pairs[near, 0], pairs[near, 1], pr["dist"][near], pr["dist_mcse"][near]))

    # ---- `desman --check`: posterior predictive fit per sample and per position (desman_amd/check.py)
    _FIT_COLUMNS = (("cells", "cells"), ("X2", "X2"), ("expected", "expected"), ("z", "z"), ("deviance", "deviance"))

    def output_Fit(self, samples, positions):
        """Fit_samples.csv: sample, cells, X2, expected, z, deviance; Fit_positions.csv: Contig, Position, then the same columns (keyed
        as Tau_Mean.csv keys its rows); and one log line with the number of samples and positions whose z exceeds check.Z_HIGH"""
        from . import check
        frame = pd.DataFrame({col: samples[key] for col, key in self._FIT_COLUMNS}, index=self._kept_sample_names())
        frame.index.name = "sample"
        frame.to_csv(self._path("Fit_samples.csv"))
        cols = {"Position": self.filtered_position}
        cols.update({col: positions[key] for col, key in self._FIT_COLUMNS})
        frame = pd.DataFrame(cols, index=self.filtered_contig_names)
        frame.index.name = "Contig"
        frame.to_csv(self._path("Fit_positions.csv"))
        logging.info("Fit_samples.csv / Fit_positions.csv written: %d of %d samples and %d of %d positions have z > %g"
                     % (check.flagged(samples), len(samples["z"]), check.flagged(positions), len(positions["z"]), check.Z_HIGH))

    def output_Fit_ppp(self, samples, positions):
        """Fit_samples_ppp.csv: sample, T_obs, T_rep, T_rep_sd, p, p_mcse; Fit_positions_ppp.csv: Contig, Position, the same columns and q
        (keyed as Fit_samples.csv / Fit_positions.csv); and one log line (check.ppp_summary)"""
        from . import check
        frame = pd.DataFrame({col: samples[col] for col in check.PPP_COLUMNS}, index=self._kept_sample_names())
        frame.index.name = "sample"
        frame.to_csv(self._path("Fit_samples_ppp.csv"))
        cols = {"Position": self.filtered_position}
        cols.update({col: positions[col] for col in check.PPP_COLUMNS + ("q",)})
        frame = pd.DataFrame(cols, index=self.filtered_contig_names)
        frame.index.name = "Contig"
        frame.to_csv(self._path("Fit_positions_ppp.csv"))
        s = check.ppp_summary(samples, positions)
        logging.info("Fit_samples_ppp.csv / Fit_positions_ppp.csv written: %d of %d samples and %d of %d positions have p < %g (a model "
                     "that fits expects at most %.2g and %.2g); %d positions have q < %g"
                     % (s["samples_low"], s["samples"], s["positions_low"], s["positions"], check.P_LOW, s["samples_expected"],
                        s["positions_expected"], s["positions_q"], check.Q_LOW))

    def output_Fit_cells(self, cell):
        """Fit_cells.csv: V x S, the posterior mean of Pearson's X per cell; rows keyed as Tau_Mean.csv's, one column per sample"""
        frame = pd.DataFrame(np.asarray(cell), index=self.filtered_contig_names, columns=self._kept_sample_names())
        frame.insert(0, "Position", self.filtered_position)
        frame.index.name = "Contig"
        frame.to_csv(self._path("Fit_cells.csv"))
        logging.info("Fit_cells.csv written")

    # ---- `desman --predictive`: position-marginal predictive density (desman_amd/predictive.py)
    def output_Predictive(self, pointwise_fit, pointwise_rest, summary):
        """Predictive_positions.csv: Contig, Position, kind, lppd, p_waic, elpd_waic -- the fitted positions (kind `fit`, keyed as
        Tau_Mean.csv keys its rows) and, ``pointwise_rest`` not None, the positions -r left out of the fit (kind `heldout`, in input
        order; p_waic empty, elpd_waic = lppd); Predictive_summary.csv: one row per kind from ``summary`` = {kind: predictive.summary}"""
        from . import predictive
        frames = [pd.DataFrame({"Contig": self.filtered_contig_names, "Position": self.filtered_position, "kind": "fit",
                                "lppd": pointwise_fit["lppd"], "p_waic": pointwise_fit["p_waic"], "elpd_waic": pointwise_fit["elpd_waic"]})]
        if pointwise_rest is not None:
            vf = self.variantFilter
            rows = np.asarray(vf.selected_indices_original, dtype=np.int64)
            rows = rows[~np.asarray(vf.selected, dtype=bool)[:len(rows)]]
            frames.append(pd.DataFrame({"Contig": [self.contig_names[i] for i in rows], "Position": self.position.to_numpy()[rows],
                                        "kind": "heldout", "lppd": pointwise_rest["lppd"], "p_waic": np.nan,
                                        "elpd_waic": pointwise_rest["lppd"]}))
        pd.concat(frames, ignore_index=True)[list(predictive.POSITION_COLUMNS)].to_csv(self._path(predictive.POSITIONS_FILE), index=False)
        rows = [predictive.summary_row(kind, summary[kind]) for kind in ("fit", "heldout") if kind in summary]
        pd.DataFrame(rows, columns=list(predictive.SUMMARY_COLUMNS)).to_csv(self._path(predictive.SUMMARY_FILE), index=False)
        logging.info("%s / %s written: %s" % (predictive.POSITIONS_FILE, predictive.SUMMARY_FILE, "; ".join(
            "%s elpd %.3f (se %.3f) over %d positions" % (r["kind"], r["elpd"], r["se"], r["n_positions"]) for r in rows)))

    def output_Selected_Variants(self):
        """the selected rows of the input table.  Every chain of a G-sweep writes the same file (the -r selection is drawn from
        a fixed seed, bin/desman:85-86): serialising 50 000 x 385 integers takes longer than the chain's GPU work, so within one
        process the text is produced once per (table, selection) and copied afterwards."""
        path = self._path("Selected_variants.csv")
        sel = np.asarray(self.variantFilter.selected, dtype=bool)
        key = (id(self.variants), sel.shape[0], hashlib.blake2b(np.packbits(sel).tobytes(), digest_size=16).digest())
        with _SELECTED_LOCK:
            prev = _SELECTED_CACHE.get(key)
            if prev is not None and prev[0]() is self.variants and os.path.isfile(prev[1]) and os.path.getsize(prev[1]) == prev[2] \
                    and os.path.abspath(prev[1]) != os.path.abspath(path):
                shutil.copyfile(prev[1], path)
            else:
                self.variants[sel].to_csv(path)
                while len(_SELECTED_CACHE) >= 4:
                    _SELECTED_CACHE.pop(next(iter(_SELECTED_CACHE)))
                _SELECTED_CACHE[key] = (weakref.ref(self.variants), path, os.path.getsize(path))
        logging.info("Selected_variants.csv written")
