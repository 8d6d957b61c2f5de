#!/usr/bin/env python3
"""Golden fixtures of the exact joint assignment (tests/golden/assign_tau_V*_S*_G*.npz), written by IMPORTING the reference
(the shims of make_golden.py: import_reference) and calling its own HaploSNP_Sampler.assignTau (HaploSNP_Sampler.py:233-261).

Per case: the inputs (counts, gamma_star, eta_star), the reference's ``conf`` and posterior draw, the full table
L[N][4^G] = sum_{s,b} x ln p_t from the reference's baseProbabilityGivenTau over its tauStates, and the texts pandas writes
for the reference's arrays by the DataFrame steps of bin/desman:219-240 (Assigned_Tau_star.csv / Assigned_Tau_conf.csv).

The tables are SHALLOW on purpose: at the project's usual synthetic depths (40-500 reads) every position has conf = 1.000 and
a comparison of conf, of the marginals or of the draw shows nothing.  One case carries a deep block as well (large |L|).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_assign.py
"""
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import make_golden as mg  # noqa: E402

# (N, S, G, seed, depth range of the shallow block, positions of a deep block (40-500 reads) appended to it)
CASES = [(40, 6, 3, 71, (0.5, 3), 0), (30, 8, 4, 72, (1, 7), 0), (16, 12, 5, 73, (1, 5), 6)]


def shallow_table(N, S, G, seed, lo_hi, n_deep):
    rs = np.random.RandomState(seed)
    gamma = rs.dirichlet(np.full(G, 0.5), size=S)
    eta = 0.04 * rs.dirichlet(np.ones(4), size=4) + 0.96 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    depth = rs.poisson(rs.uniform(lo_hi[0], lo_hi[1], size=(N, S)))
    if n_deep:
        depth[N - n_deep:] = rs.randint(40, 501, size=(n_deep, S))
    counts = np.zeros((N, S, 4), dtype=np.int64)
    for n in range(N):
        p = gamma @ eta[tau[n]]                          # [S][4]
        for s in range(S):
            counts[n, s] = rs.multinomial(depth[n, s], p[s] / p[s].sum())
    # the "fitted" parameters: close to the generating ones, not equal to them
    g_fit = gamma * rs.uniform(0.8, 1.25, size=gamma.shape)
    g_fit = np.maximum(g_fit / g_fit.sum(axis=1, keepdims=True), 1.0e-6)
    g_fit /= g_fit.sum(axis=1, keepdims=True)
    e_fit = 0.03 * rs.dirichlet(np.ones(4), size=4) + 0.97 * np.eye(4)
    return counts, np.ascontiguousarray(g_fit), np.ascontiguousarray(e_fit)


def writer_texts(assign_tau, conf, names, positions, G):
    """the two files of bin/desman:219-240 for these arrays, as text"""
    n = assign_tau.shape[0]
    star = pd.DataFrame(np.reshape(assign_tau, (n, G * 4)), index=names)
    cf = pd.DataFrame(conf, index=names)
    out = []
    for frame in (star, cf):
        frame['Position'] = positions
        cols = frame.columns.tolist()
        buf = io.StringIO()
        frame[cols[-1:] + cols[:-1]].to_csv(buf)
        out.append(buf.getvalue())
    return out


def main():
    _, hsnp, _ = mg.import_reference()
    for (N, S, G, seed, lo_hi, n_deep) in CASES:
        counts, gamma, eta = shallow_table(N, S, G, seed, lo_hi, n_deep)
        smp = hsnp.HaploSNP_Sampler(counts, G, np.random.RandomState(seed), max_iter=1)
        smp.gamma_star, smp.eta_star = gamma, eta
        ref_tau, ref_conf = smp.assignTau(counts.reshape(N, S * 4))
        T = smp.nTauStates
        logp = np.array([np.log(smp.baseProbabilityGivenTau(smp.tauStates[t], gamma, eta)) for t in range(T)])    # [T][S][4]
        L = np.array([[(logp[t] * counts[n]).sum() for t in range(T)] for n in range(N)])
        state_digits = np.argmax(smp.tauStates, axis=2)                                                           # [T][G]
        names = ["contig_%d" % (n // 7) for n in range(N)]
        positions = np.arange(N) * 13 + 5
        star_csv, conf_csv = writer_texts(ref_tau, ref_conf, names, pd.Series(positions, index=names), G)
        path = os.path.join(HERE, "assign_tau_V%d_S%d_G%d.npz" % (N, S, G))
        np.savez_compressed(path, counts=counts, gamma=gamma, eta=eta, G=G, conf=ref_conf, ref_draw=ref_tau.astype(np.int8), L=L,
                            state_digits=state_digits.astype(np.int8), names=np.array(names), positions=positions,
                            star_csv=star_csv, conf_csv=conf_csv, n_deep=n_deep,
                            note="reference HaploSNP_Sampler.assignTau; L from baseProbabilityGivenTau over tauStates")
        srt = np.sort(L, axis=1)
        print("%s: %d B, conf<0.99 at %.0f%%, min conf %.3f, smallest gap %.3g, max|L| %.4g, draws off the MAP %.0f%%"
              % (os.path.basename(path), os.path.getsize(path), 100 * (ref_conf < 0.99).mean(), ref_conf.min(),
                 (srt[:, -1] - srt[:, -2]).min(), np.abs(L).max(),
                 100 * (np.argmax(ref_tau, axis=2) != state_digits[np.argmax(L, axis=1)]).any(axis=1).mean()))


if __name__ == "__main__":
    main()
