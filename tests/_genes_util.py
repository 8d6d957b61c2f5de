"""Shared set-up of the accessory-gene (f4) tests: the synth_genes() data set of a golden fixture, reshaped
the way GeneAssign.main feeds Eta_Sampler (tests/golden/make_golden.py: gen_gene_assign), and synthetic cases of
any shape with the device object that holds them."""
import ast
import os

import numpy as np
from scipy.special import gammaln

from desman_amd.synth import synth_genes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    kw = dict(ast.literal_eval(str(z['synth_kw'])))
    C, S, G = int(z['C']), int(z['S']), int(z['G'])
    d = synth_genes(C, S, G, seed=int(z['synth_seed']), **kw)
    gm = d['gamma'] / d['gamma'].sum(axis=1)[:, None]                 # GeneAssign.py:226-228
    delta = gm * d['total_mean'][:, None]                            # :230
    gene_off = np.concatenate([[0], np.cumsum(np.bincount(d['gene_of'], minlength=C))]).astype(np.int32)
    variants = [np.ascontiguousarray(d['counts'][gene_off[c]:gene_off[c + 1]]) for c in range(C)]
    return dict(z=z, d=d, C=C, S=S, G=G, gamma=np.ascontiguousarray(gm), delta=np.ascontiguousarray(delta),
                delta_gs=np.ascontiguousarray(delta.T), gene_off=gene_off, variants=variants,
                eps=np.ascontiguousarray(d['epsilon']), cov=np.ascontiguousarray(d['cov']),
                seed=int(z['seed']), iters=int(z['iters']), tau_iter=int(z['tau_iter']))


def split(cat, gene_off):
    return [np.ascontiguousarray(cat[gene_off[c]:gene_off[c + 1]]).astype(np.int64) for c in range(len(gene_off) - 1)]


def _case(C, S, G, vmax, seed, **kw):
    d = synth_genes(C, S, G, seed=seed, vmax=vmax, **kw)
    gamma = np.ascontiguousarray(d['gamma'])
    delta = np.ascontiguousarray(gamma * d['total_mean'][:, None])
    off = np.concatenate([[0], np.cumsum(np.bincount(d['gene_of'], minlength=C))]).astype(np.int32)
    variants = [np.ascontiguousarray(d['counts'][off[c]:off[c + 1]]) for c in range(C)]
    return dict(d=d, C=C, S=S, G=G, gamma=gamma, delta=delta, delta_gs=np.ascontiguousarray(delta.T), gene_off=off,
                variants=variants, eps=np.ascontiguousarray(d['epsilon']), cov=np.ascontiguousarray(d['cov']))


def _device(k, eta, tau, max_eta):
    from desman_amd import _lib
    from oracle import ref_genes as rg
    dev = _lib.Genes(0)
    x = k['d']['counts']
    dev.set_data(x, k['gene_off'], k['cov'])
    per_v = (gammaln(x.sum(axis=2) + 1.0) - gammaln(x + 1.0).sum(axis=2)).sum(axis=1) if len(x) else np.zeros(0)
    mult = np.array([per_v[k['gene_off'][c]:k['gene_off'][c + 1]].sum() for c in range(k['C'])])
    prior = rg.eta_log_prior(max_eta, 0.01)
    dev.set_model(k['gamma'], k['eps'], k['delta_gs'], max_eta, prior, -gammaln(k['cov'] + 1.0).sum(axis=1), mult)
    dev.set_state(eta.astype(np.int32), tau)
    dev.seed(3)
    return dev, prior
