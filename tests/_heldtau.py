"""What the held-tau tests share (tests/test_held_tau_cpu.py, tests/test_gpu_held_tau.py): the held sweep and the held chain restated
from the oracle's existing pieces, and the recovery case both files run -- on the CPU first, so that what the GPU test asks is known to
hold for the restatement.

A held sweep over haplotypes 0 .. F-1 of G is cbind.sample_tau_u over ALL G haplotypes with a [V][G] uniform array whose free columns
carry the stream's words (the held columns carry anything), with the held digits put back afterwards: the held haplotypes are swept
last, so every free step sees them at their held values, and what the full sweep does to them afterwards is undone."""
import numpy as np

import _fixtau as F
from _philox import tau_uniforms
from oracle import cbind

RECOVERY_SHAPE, RECOVERY_SEED, RECOVERY_DEPTH_SCALE, RECOVERY_ITERS = (300, 12, 3), 0x4E0F3170A5C3D2E1, 1.0, 60


def held_sweep(tau, gamma, eta, counts, u_free, n_held):
    """(new one-hot tau, changed free (v, g) pairs): the oracle composition.  u_free = the V F uniforms, position-major"""
    tau = np.ascontiguousarray(tau, dtype=np.int64)
    V, G, _ = tau.shape
    Fr = G - n_held
    u = np.full((V, G), 0.5)
    u[:, :Fr] = np.asarray(u_free, dtype=np.float64).reshape(V, Fr)
    new = tau.copy()
    cbind.sample_tau_u(new, np.ascontiguousarray(gamma), np.ascontiguousarray(eta), np.ascontiguousarray(counts, dtype=np.int64), u.reshape(-1))
    new[:, Fr:] = tau[:, Fr:]
    return new, int((new[:, :Fr] != tau[:, :Fr]).any(axis=2).sum())


def philox_free_uniforms(ctr_seed, it, V, G, n_held):
    """the uniforms of the free steps of the sweep with counter ``it``: step (v, g) is keyed as the full sweep keys it"""
    return np.ascontiguousarray(tau_uniforms(ctr_seed, it, V, G).reshape(V, G)[:, :G - n_held]).reshape(-1)


def etas(kind, seed=0):
    """the three error matrices of the one-sweep tests: a random one without zeros, the identity, one with a zero row"""
    if kind == "identity":
        return np.eye(4)
    rng = np.random.default_rng(seed)
    e = np.ascontiguousarray(rng.dirichlet(np.ones(4), size=4) * 0.08 + 0.92 * np.eye(4))
    if kind == "zero-row":
        e[2] = 0.0
    return e


class RefCtx:
    """the calls of _lib.Context that held_tau.novel_chain and the chain tests make, served by the oracle's pieces in numpy: the held
    chain under mu/E specification ``spec`` with the sweep's uniforms from the GSL stream"""
    spec = 2

    def __init__(self, device=0):
        self.alpha, self.delta, self.epsilon = 0.1, 0.1, 1.0e-6
        self.it = 0

    def set_counts(self, x):
        self.counts = np.ascontiguousarray(x, dtype=np.int64)

    def set_priors(self, alpha, delta, epsilon):
        self.alpha, self.delta, self.epsilon = alpha, delta, epsilon

    def set_state(self, tau, gamma, eta):
        self.tau, self.gamma, self.eta = np.ascontiguousarray(tau, dtype=np.int64), np.ascontiguousarray(gamma), np.ascontiguousarray(eta)

    def seed(self, mt_seed, ctr_seed=None):
        self.mt, self.cseed = cbind.MT19937(mt_seed), ctr_seed

    def _lp(self, tau, g, e):
        idx = cbind.onehot_to_idx(tau)
        return cbind.loglik(idx, g, e, self.counts), cbind.logpost(idx, g, e, self.counts, self.alpha, self.delta)

    def gibbs_update_held_tau(self, n_iter, n_held, fix_eta=False):
        V, G, _ = self.tau.shape
        tr = dict(gamma=[], eta=[], ll=[], lp=[], nchange=[], tau=[])
        self.star = dict(tau=self.tau.copy(), gamma=self.gamma.copy(), eta=self.eta.copy(), lp=self._lp(self.tau, self.gamma, self.eta)[1], it=0)
        for k in range(n_iter):
            mu, E = F.stats(self.spec, cbind.onehot_to_idx(self.tau), self.gamma, self.eta, self.counts, self.cseed, self.it)
            g, e_new, _ = cbind.dirichlet_counter(mu, E, self.cseed, self.it, self.alpha, self.delta, self.epsilon)
            g = np.ascontiguousarray(g)
            self.tau, n = held_sweep(self.tau, g, self.eta, self.counts, self.mt.uniform(V * (G - n_held)), n_held)
            self.gamma = g
            if not fix_eta:
                self.eta = np.ascontiguousarray(e_new)
            self.it += 1
            ll, lp = self._lp(self.tau, self.gamma, self.eta)
            for key, val in (("gamma", self.gamma), ("eta", self.eta), ("ll", ll), ("lp", lp), ("nchange", n), ("tau", self.tau)):
                tr[key].append(val)
            if lp > self.star["lp"]:
                self.star = dict(tau=self.tau.copy(), gamma=self.gamma.copy(), eta=self.eta.copy(), lp=lp, it=k)
        self.trace = {key: np.array(val) for key, val in tr.items()}

    def get_trace(self):
        return self.trace

    def get_star(self):
        return self.star

    def close(self):
        pass


def recovery_case():
    """(counts [300,12,4], true digits [300,3], true gamma): three strains, none below 10 % in every sample, default depths of
    desman_amd/synth.py (40 .. 500 reads per sample and position)"""
    from desman_amd.synth import synth_counts
    V, S, G = RECOVERY_SHAPE
    for seed in range(900, 1000):
        counts, tau, gamma = synth_counts(V, S, G, seed=seed, depth_scale=RECOVERY_DEPTH_SCALE)
        if (gamma.max(axis=0) >= 0.10).all():
            return counts, tau.astype(np.int64), gamma
    raise AssertionError("no synthetic table with every strain at 10 % somewhere")


def recovery_run(context, spec=None):
    """the free MAP haplotype of the recovery chain (two true strains held, one free from the random start) and the third strain"""
    from desman_amd import held_tau
    counts, tau, _ = recovery_case()
    res = held_tau.novel_chain(counts, tau[:, 1:], 0.96 * np.eye(4) + 0.01, 1, n_iter=RECOVERY_ITERS, burn=RECOVERY_ITERS // 2,
                               seed=RECOVERY_SEED, context=context)
    return res, tau[:, 0]
