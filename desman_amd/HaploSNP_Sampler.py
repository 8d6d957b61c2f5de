"""Host mirror of desman/HaploSNP_Sampler.py for the path `bin/desman` drives.

Same class name, constructor signature, attributes and method names; the Gibbs
iterations run entirely on the device (dsm_ctx_gibbs_update).  V-sized arrays
are fetched from HBM only when asked for (tau_store is materialised lazily).
assignTau (dead in the reference's CLI, bin/desman:213-214) runs on the device as an
exact enumeration of the 4^G joint states (dsm_assign_tau, G <= 10); the tauStates
table it walks upstream is never built.
update_fixed_tau (the reduced runs of the reference's Chib estimators, :409-428)
runs on the device as well (dsm_ctx_gibbs_update_fixed_tau).
Not mirrored (never reached by the CLI): the pure-Python
samplers, Chib marginal likelihood, DIC.
"""
import logging

import numpy as np

from . import _lib
from . import fixed_tau as _fixed_tau
from . import check as _check
from . import diagnose as _diagnose
from . import marginals as _marginals
from . import predictive as _predictive
from . import relabel as _relabel
from . import sampletau as _sampletau


def _check_pair_every(pair_every):
    """pair_every of the constructor: an int >= 0 (0 = no pair moves; E = a pair pass after every E-th sweep of update())"""
    if isinstance(pair_every, bool) or not isinstance(pair_every, (int, np.integer)) or pair_every < 0:
        raise ValueError("pair_every must be an integer >= 0 (0 = no pair moves); got %r" % (pair_every,))
    return int(pair_every)


class HaploSNP_Sampler:

    def __init__(self, snps, G, randomState, fixed_tau=None, burn_iter=None, max_iter=None,
                 alpha_constant=0.1, delta_constant=0.1, epsilon=1.0e-6, device=0, ctx=None, pair_every=0):
        self.pair_every = _check_pair_every(pair_every)
        self.burn_iter = 250 if burn_iter is None else burn_iter
        self.max_iter = 250 if max_iter is None else max_iter
        self.randomState = randomState
        self.G = int(G)
        snps = np.asarray(snps)
        self.V, self.S = snps.shape[0], snps.shape[1]
        self.variants = np.array(snps, dtype=np.int64, order='C')
        self.epsilon = epsilon
        self.delta_constant = delta_constant
        self.delta = np.full(4, delta_constant)
        self.alpha_constant = alpha_constant
        self.alpha = np.full(self.G, alpha_constant)
        # the constructor consumes the caller's RNG exactly like the reference (:63, :72)
        self.gamma = self.randomState.dirichlet(self.alpha, size=self.S)
        if fixed_tau is None:
            tri = self.randomState.randint(0, 4, self.V * self.G).reshape(self.V, self.G)
            self.tau = np.zeros((self.V, self.G, 4), dtype=np.int64)
            np.put_along_axis(self.tau, tri[..., None], 1, axis=2)
        else:
            self.tau = np.reshape(fixed_tau, (self.V, self.G, 4)).astype(np.int64)
        self.tauIndices = np.zeros(self.V, dtype=np.int64)
        self.eta = 0.96 * np.identity(4) + 0.01 * np.ones((4, 4))
        self._alloc_stores()
        self.ll = 0.0
        self.lp = 0.0
        self._device = device
        self._ctx = ctx if ctx is not None else _lib.Context(device)
        self._ctx.set_counts(self.variants)
        self._ctx.set_priors(alpha_constant, delta_constant, epsilon)
        if ctx is None or self.pair_every > 0:      # (a context handed in keeps its own setting unless pair moves are asked for here)
            self._ctx.set_pair_moves(self.pair_every)
        self._tau_sum = None
        self._relabel = None
        self._diag = None
        self._fit = None
        self.relabel_ref = None         # the reference relabelling() matches the stored iterations to ([V,G] digits); None = tau_star
        self._have_trace = False
        self._keyed = False
        self.mt_state = None            # a GSL stream of the sampler's own (update_batch: several chains in one thread);
                                        # None = the stream of the sampletau module, as in the reference

    def _alloc_stores(self):
        self.gamma_store = np.zeros((self.max_iter, self.S, self.G))
        self.eta_store = np.zeros((self.max_iter, 4, 4))
        self.ll_store = np.zeros(self.max_iter)
        self.lp_store = np.zeros(self.max_iter)
        self.nchange_store = np.zeros(self.max_iter, dtype=np.int64)

    def calcK(self):
        return self.V * self.G + self.S * (self.G - 1)

    # ---- RNG plumbing: the tau uniforms continue the process-global GSL-compatible stream
    def _bind_rng(self):
        st = self.mt_state if self.mt_state is not None else _sampletau.getRNGState()   # raises if initRNG()/setRNG() were not called
        if not self._keyed:
            # key the counter-based streams (mu/E, gamma, eta) once per sampler object
            # a function of the stream position only: deterministic whatever else runs in the process
            key = ((int(st[0]) << 32) ^ int(st[1]) ^ (int(st[2]) << 16) ^ (0x9E3779B97F4A7C15 * (int(st[624]) + 1))) \
                & 0xFFFFFFFFFFFFFFFF
            self._ctx.seed(1, ctr_seed=key)
            self._keyed = True
        self._ctx.set_mt_state(st)

    def _release_rng(self):
        if self.mt_state is not None:
            self.mt_state = self._ctx.get_mt_state()
        else:
            _sampletau.setRNGState(self._ctx.get_mt_state())

    def _push_state(self):
        self._ctx.set_state(np.ascontiguousarray(self.tau, dtype=np.int64),
                            np.ascontiguousarray(self.gamma, dtype=np.float64),
                            np.ascontiguousarray(self.eta, dtype=np.float64))
        self.G = self._ctx.G

    # ---- checkpoint / resume (optional; the reference's hook, Output_Results.output_Pickled_haploSNP, is dead code)
    def save_checkpoint(self, path):
        """the chain between two update() calls: state, both stream positions, the key of the counter-based streams.  A sampler
        built on the same table that loads it continues bit for bit (tests/test_gpu_host.py)."""
        self._bind_rng()                                      # keys the counter streams if no update() has run yet
        self._release_rng()
        key, it = self._ctx.counters()                        # (no resident state needed: also valid before the first update())
        mt = self.mt_state if self.mt_state is not None else _sampletau.getRNGState()
        np.savez(path, tau=np.asarray(self.tau, dtype=np.int64), gamma=self.gamma, eta=self.eta, mt_state=np.asarray(mt, dtype=np.uint32),
                 ctr_seed=np.uint64(key), iter_ctr=np.uint32(it), G=self.G, own_stream=self.mt_state is not None,
                 screen=self._ctx.screen_state())

    def load_checkpoint(self, path):
        z = np.load(path)
        if int(z["G"]) != self.G or z["tau"].shape != (self.V, self.G, 4) or z["gamma"].shape != (self.S, self.G):
            raise ValueError("checkpoint of another shape: tau %s, gamma %s" % (z["tau"].shape, z["gamma"].shape))
        self.tau, self.gamma, self.eta = z["tau"].copy(), z["gamma"].copy(), z["eta"].copy()
        self.updateTauIndices()
        if bool(z["own_stream"]):
            self.mt_state = z["mt_state"].copy()
        else:
            _sampletau.setRNGState(z["mt_state"])             # the module's stream, as in the run that saved it
        ck = dict(tau=self.tau, gamma=self.gamma, eta=self.eta, mt_state=z["mt_state"], ctr_seed=z["ctr_seed"], iter_ctr=z["iter_ctr"])
        if "screen" in z.files:
            ck["screen"] = z["screen"]
        self._ctx.restore(ck)
        self._keyed = True                                    # the counter streams keep their key and position

    # ---- the Gibbs loop
    def update(self):
        """max_iter Gibbs iterations (HaploSNP_Sampler.py:334-365), on the device.  pair_every = E > 0: a pair pass follows the sweep of
        every iteration whose counter satisfies (iter_ctr + 1) mod E == 0."""
        self._push_state()
        self._bind_rng()
        self._ctx.gibbs_update(self.max_iter)
        self._release_rng()
        self._collect(prefix='nlp')

    @staticmethod
    def update_batch(samplers, on_chain=None):
        """update() of several chains of one shape on one device at once: one kernel launch per step of the iteration for
        all of them (dsm_batch_gibbs_update; the replicate chains of a G value, scripts/runDesman.sh:15-21).  Every sampler
        needs a GSL stream of its own (``mt_state``).  The mu/E pass of a batch is the aggregated sampler."""
        samplers = list(samplers)
        if any(getattr(s, "pair_every", 0) > 0 for s in samplers):
            raise ValueError("update_batch: pair moves (pair_every > 0) have no batched form; run such chains one by one with update()")
        n = samplers[0].max_iter
        if any(s.max_iter != n for s in samplers) or any(s.mt_state is None for s in samplers):
            raise ValueError("update_batch: samplers need equal max_iter and a GSL stream each (mt_state)")
        for s in samplers:
            s._push_state()
            s._bind_rng()
        _lib.Context.batch_gibbs_update([s._ctx for s in samplers], n)
        for s in samplers:
            if on_chain is not None:
                on_chain(s)
            s._release_rng()
            s._collect(prefix='nlp')

    @staticmethod
    def updateTau_batch(samplers, on_chain=None):
        """updateTau() of several chains of one shape at once (dsm_batch_update_tau); a GSL stream each (mt_state)"""
        samplers = list(samplers)
        n = samplers[0].max_iter
        if any(s.max_iter != n for s in samplers) or any(s.mt_state is None for s in samplers):
            raise ValueError("updateTau_batch: samplers need equal max_iter and a GSL stream each (mt_state)")
        for s in samplers:
            s._push_state()
            s._bind_rng()
        _lib.Context.batch_update_tau([s._ctx for s in samplers], [s.gamma_store[:n] for s in samplers],
                                      [s.eta_store[:n] for s in samplers])
        for s in samplers:
            if on_chain is not None:
                on_chain(s)
            s._release_rng()
            gs, es = s.gamma_store, s.eta_store
            s._collect(prefix='nll', keep_gamma_eta=True)
            s.gamma_store, s.eta_store = gs, es

    def updateTau(self):
        """tau-only sweeps driven by gamma_store / eta_store (HaploSNP_Sampler.py:383-407)."""
        self._push_state()
        self._bind_rng()
        self._ctx.update_tau(self.gamma_store[:self.max_iter], self.eta_store[:self.max_iter])
        self._release_rng()
        gs, es = self.gamma_store, self.eta_store
        self._collect(prefix='nll', keep_gamma_eta=True)
        self.gamma_store, self.eta_store = gs, es

    def update_fixed_tau(self, fix_eta=False, pool=-1):
        """max_iter iterations with tau held (HaploSNP_Sampler.py:409-428): sampleMu, sampleGamma, sampleEta and logPosterior per
        iteration, on the device (dsm_ctx_gibbs_update_fixed_tau).  Fills gamma_store, eta_store, ll_store, lp_store, the star state and
        lp; tau is unchanged and the GSL stream of the tau draws is not consumed.  The reference also keeps mu_store and E_store, the
        auxiliary counts of every iteration: they are not kept here (the sums live on the device for one iteration only).
        fix_eta: eta is held as well.  pool: 0 = on the table as it is, 1 = on the counts pooled per distinct tau word (the same law,
        other draws), -1 = pooled where that makes the table smaller."""
        self._push_state()
        self._bind_rng()
        self._ctx.gibbs_update_fixed_tau(self.max_iter, fix_eta=fix_eta, pool=pool)
        self._release_rng()
        self._collect(prefix='nlp')

    def update_held(self, n_held, fix_eta=False):
        """max_iter Gibbs iterations with the LAST n_held haplotypes held and the others sampled, on the device
        (dsm_ctx_gibbs_update_held_tau; the reference has no counterpart).  Fills the stores, the star state and lp as update() does;
        the GSL stream advances by V (G - n_held) words per iteration.  fix_eta: eta is held as well.  n_held = 0 is update(),
        n_held = G is update_fixed_tau(pool=0).  Pair moves (pair_every > 0) have no held form: 0 < n_held < G is refused then."""
        if self.pair_every > 0 and 0 < n_held < self.G:
            raise ValueError("update_held: pair moves (pair_every = %d) have no partly held form (0 < n_held < G)" % self.pair_every)
        self._push_state()
        self._bind_rng()
        self._ctx.gibbs_update_held_tau(self.max_iter, n_held, fix_eta=fix_eta)
        self._release_rng()
        self._collect(prefix='nlp')

    def _collect(self, prefix, keep_gamma_eta=False):
        tr = self._ctx.get_trace()
        n = self.max_iter
        self.ll_store[:n] = tr["ll"]
        self.lp_store[:n] = tr["lp"]
        self.nchange_store[:n] = tr["nchange"]
        if not keep_gamma_eta:
            self.gamma_store[:n] = tr["gamma"]
            self.eta_store[:n] = tr["eta"]
        tau, gamma, eta = self._ctx.get_state()
        self.tau = tau
        if not keep_gamma_eta:
            self.gamma, self.eta = gamma, eta
        star = self._ctx.get_star()
        self.tau_star, self.lp_star, self.iter_star = star["tau"], star["lp"], star["it"]
        if not keep_gamma_eta:
            self.gamma_star, self.eta_star = star["gamma"], star["eta"]
        if n > 0:
            self.ll, self.lp = float(tr["ll"][-1]), float(tr["lp"][-1])
        for it in range(0, n, 10):
            logging.info('Gibbs Iter %d, no. changed = %d, %s = %f' % (it, tr["nchange"][it], prefix, tr["lp"][it]))
        self._tau_sum = None
        self._relabel = None
        self._diag = None
        self._fit = None
        self._have_trace = True
        self.updateTauIndices()

    # ---- deterministic functions
    def logLikelihood(self, cGamma, cTau, cEta):
        self._ctx.set_state(np.ascontiguousarray(cTau, dtype=np.int64), np.ascontiguousarray(cGamma, dtype=np.float64),
                            np.ascontiguousarray(cEta, dtype=np.float64))
        return self._ctx.loglik()[0]

    def logPosterior(self, cGamma, cTau, cEta):
        self._ctx.set_state(np.ascontiguousarray(cTau, dtype=np.int64), np.ascontiguousarray(cGamma, dtype=np.float64),
                            np.ascontiguousarray(cEta, dtype=np.float64))
        return self._ctx.loglik()[1]

    def mapTauState(self, tauState):
        G = tauState.shape[0]
        w = 4 ** (G - 1 - np.arange(G, dtype=object))
        return int((np.argmax(tauState, axis=1).astype(object) * w).sum())

    def updateTauIndices(self):
        # base-4 index of the haplotype pattern (HaploSNP_Sampler.py:224-231); exact for G <= 31
        idx = np.argmax(self.tau, axis=2).astype(np.int64)
        if self.G <= 31:
            w = 4 ** (self.G - 1 - np.arange(self.G, dtype=np.int64))
            self.tauIndices = (idx * w[None, :]).sum(axis=1)
        else:
            self.tauIndices = np.array([self.mapTauState(self.tau[v]) for v in range(self.V)], dtype=object)

    # ---- positions that were not in the fit (HaploSNP_Sampler.py:233-261)
    def _assign(self, assignMatrix, seed):
        a = np.asarray(assignMatrix)
        counts = np.ascontiguousarray(np.reshape(a, (a.shape[0], self.S, 4)), dtype=np.int64)
        return _lib.assign_tau(counts, self.gamma_star, self.eta_star, seed=seed, device=self._device)

    @staticmethod
    def _onehot(state):
        out = np.zeros(state.shape + (4,), dtype=np.int64)
        np.put_along_axis(out, state.astype(np.int64)[..., None], 1, axis=2)
        return out

    def assignTau(self, assignMatrix):
        """(assignTau [N,G,4] one-hot, conf [N]) for the rows of assignMatrix [N, S*4] under gamma_star / eta_star: assignTau is one
        draw from the exact posterior over the 4^G joint states of each position, conf the posterior probability of its most
        probable state.  The draw is keyed by one randint of the sampler's randomState, so repeated calls differ as upstream."""
        seed = int(self.randomState.randint(0, 2 ** 31 - 1))
        res = self._assign(assignMatrix, seed)
        return self._onehot(res["draw_state"]), res["conf"]

    def assignTauExact(self, assignMatrix):
        """the deterministic part of the same posterior: dict of tau [N,G,4] (one-hot MAP state, ties to the lowest state index),
        conf [N], logz [N] (log normaliser) and marg [N,G,4] (P(tau_vg = a), the exact counterpart of tauMean)"""
        res = self._assign(assignMatrix, None)
        return dict(tau=self._onehot(res["map_state"]), conf=res["conf"], logz=res["logz"], marg=res["marg"])

    def assignTauSampled(self, assignMatrix, kept=_lib.SAMPLED_KEPT, burn=_lib.SAMPLED_BURN, seed=None, pair_every=0):
        """the same posterior by four private Gibbs chains per position (every G <= 32): dict of tau [N,G,4]
        (one-hot polished best state), map_ll, conf (Monte-Carlo), marg [N,G,4] (Rao-Blackwellised), spread [N] (the chains'
        disagreement: large where they sit in different modes) and draw [N,G,4].  seed=None: one randint of the sampler's randomState.
        pair_every = E > 0: joint moves of two haplotypes after every E-th sweep and in the polish (0: single-site moves only)."""
        if seed is None:
            seed = int(self.randomState.randint(0, 2 ** 31 - 1))
        a = np.asarray(assignMatrix)
        counts = np.ascontiguousarray(np.reshape(a, (a.shape[0], self.S, 4)), dtype=np.int64)
        res = _lib.assign_tau_sampled(counts, self.gamma_star, self.eta_star, seed=seed, burn=burn, kept=kept, device=self._device,
                                      pair_every=pair_every)
        return dict(tau=self._onehot(res["map_state"]), map_ll=res["map_ll"], conf=res["conf"], marg=res["marg"], spread=res["spread"],
                    draw=self._onehot(res["draw_state"]))

    # ---- samples that were not in the fit (no counterpart upstream)
    def fitGamma(self, snps=None, tau=None, eta=None, presence=False, max_iter=_lib.FIT_MAX_ITER, tol=_lib.FIT_TOL):
        """maximum-likelihood abundances with the haplotypes and the error matrix held fixed: a dict of gamma [S',G], loglik, deviance,
        iters, converged (and lr_absent [S',G] with presence) for the samples of snps [V,S',4] -- default: the chain's own counts, on
        the resident tensor -- under tau (default tau_star) and eta (default eta_star)"""
        tau = self.tau_star if tau is None else tau
        eta = self.eta_star if eta is None else eta
        if snps is None:
            return self._ctx.fit_gamma(eta, tau=tau, max_iter=max_iter, tol=tol, presence=presence)
        return _lib.fit_gamma(snps, tau, eta, max_iter=max_iter, tol=tol, presence=presence, device=self._device)

    def fitGammaEta(self, snps=None, tau=None, eta0=None, max_iter=_lib.FIT_MAX_ITER, tol=_lib.FIT_TOL):
        """abundances AND one error matrix of the samples of snps [V,S',4] -- default: the chain's own counts, on the resident tensor --
        fitted jointly with the haplotypes tau (default tau_star) held fixed, from eta0 (default eta_star): the dict of
        _lib.fit_gamma_eta (gamma, eta, loglik, loglik0, deviance, iters, converged, dead_rows, lr_eta)"""
        tau = self.tau_star if tau is None else tau
        eta0 = self.eta_star if eta0 is None else eta0
        if snps is None:
            return self._ctx.fit_gamma_eta(eta0, tau=tau, max_iter=max_iter, tol=tol)
        return _lib.fit_gamma_eta(snps, tau, eta0, max_iter=max_iter, tol=tol, device=self._device)

    def fitGammaInterval(self, level=0.95, snps=None, tau=None, eta=None, max_iter=_lib.FIT_MAX_ITER, tol=_lib.FIT_TOL, ctol=_lib.FIT_CTOL):
        """fitGamma() and the profile-likelihood intervals of its abundances at confidence ``level``: fitGamma's dict with lo [S',G],
        hi [S',G] and flags [S',G] added (_lib.fit_gamma_interval)"""
        tau = self.tau_star if tau is None else tau
        eta = self.eta_star if eta is None else eta
        res = self.fitGamma(snps=snps, tau=tau, eta=eta, max_iter=max_iter, tol=tol)
        kw = dict(level=level, max_iter=max_iter, tol=tol, ctol=ctol)
        if snps is None:
            res.update(self._ctx.fit_gamma_interval(eta, res["gamma"], tau=tau, **kw))
        else:
            res.update(_lib.fit_gamma_interval(snps, tau, eta, res["gamma"], device=self._device, **kw))
        return res

    def posteriorGamma(self, snps=None, tau=None, eta=None, n_iter=1000, burn=200, fix_eta=True, level=0.95,
                       seed=_fixed_tau.POSTERIOR_SEED, pool=-1):
        """the counterpart of fitGamma under the chain's Dirichlet prior: the posterior of the abundances of the samples of snps [V,S',4]
        -- default: the chain's own counts -- with tau (default tau_star) held and eta (default eta_star) held or, with fix_eta=False,
        sampled from it as the start.  A chain of its own (uniform gamma rows, stream key ``seed``: the same call gives the same bits;
        the sampler's chain and streams are not touched).  Dict of mean, sd, lo, med, hi [S',G] (quantiles (1 - level) / 2, 0.5,
        1 - (1 - level) / 2 of the kept draws), draws [n_iter - burn, S', G], ll, and eta_mean / eta_sd / eta_draws with fix_eta=False."""
        tau = self.tau_star if tau is None else tau
        eta = self.eta_star if eta is None else eta
        snps = self.variants if snps is None else snps
        return _fixed_tau.posterior_gamma(snps, tau, eta, n_iter=n_iter, burn=burn, fix_eta=fix_eta, level=level, seed=seed, pool=pool,
                                          alpha=self.alpha_constant, delta=self.delta_constant, epsilon=self.epsilon, device=self._device)

    def calculateSND(self, tau):
        """pairwise single-nucleotide differences between haplotypes (:712-730)."""
        idx = np.argmax(tau, axis=2)
        return (idx[:, :, None] != idx[:, None, :]).sum(axis=0)

    def compSND(self, tau1, tau2):
        i1, i2 = np.argmax(tau1, axis=2), np.argmax(tau2, axis=2)
        return (i1[:, :, None] != i2[:, None, :]).sum(axis=0)

    def variableTau(self, tau):
        idx = np.argmax(tau, axis=2)
        return (idx != idx[:, :1]).any(axis=1)

    def removeDegenerate(self):
        """merge haplotypes that are identical at every position (:771-832): the lower
        index survives, gamma columns are summed, survivors keep their order."""
        snd = self.calculateSND(self.tau)
        deleted = np.zeros(self.G, dtype=bool)
        absorbed = [[] for _ in range(self.G)]
        for g in range(self.G):
            for h in range(g + 1, self.G):
                if not deleted[h] and snd[g, h] == 0:
                    deleted[h] = True
                    absorbed[g].append(h)
        keep = [g for g in range(self.G) if not deleted[g]]
        gamma_new = np.zeros((self.S, len(keep)))
        for k, g in enumerate(keep):
            gamma_new[:, k] = self.gamma[:, g]
            for h in absorbed[g]:
                gamma_new[:, k] += self.gamma[:, h]
        self.tau = np.ascontiguousarray(self.tau[:, keep, :])
        self.gamma = gamma_new
        self.G = len(keep)
        self.alpha = np.full(self.G, self.alpha_constant)
        self.gamma_store = np.zeros((self.max_iter, self.S, self.G))
        self._have_trace = False
        self._tau_sum = None
        self._relabel = None
        self._diag = None
        self._fit = None
        self.updateTauIndices()

    # ---- posterior summaries of the last update() (HaploSNP_Sampler.py:463-483,834-839)
    def meanDeviance(self):
        return -2.0 * np.mean(self.ll_store)

    def gammaMean(self):
        return np.mean(self.gamma_store, axis=0)

    def etaMean(self):
        return np.mean(self.eta_store, axis=0)

    def _tausum(self):
        if self._tau_sum is None:
            if not self._have_trace:
                raise _lib.DesmanHipError("no update() has run: tau_store is empty")
            self._tau_sum = self._ctx.get_tau_sum()
        return self._tau_sum

    def tauMean(self):
        return self._tausum() / float(self.max_iter)

    def probabilisticTau(self):
        return self._tausum() / float(self.max_iter)

    # ---- the same summaries with every stored iteration's labels matched to a reference first (desman_amd/relabel.py)
    def _trace_ctx(self):
        if not self._have_trace:
            raise _lib.DesmanHipError("no update() has run: tau_store is empty")
        return self._ctx

    def traceSND(self, ref=None, self_=False):
        """[max_iter, G, Gr] distances of every stored iteration's haplotypes, from the trace on the device: to the haplotypes of
        ``ref`` ([V,Gr] digits or [V,Gr,4] one-hot; default tau_star), or -- self_ -- to each other within the iteration
        (calculateSND of every iteration)"""
        ctx = self._trace_ctx()
        if self_:
            return ctx.trace_snd(_lib.SND_SELF)
        return ctx.trace_snd(_lib.SND_STAR) if ref is None else ctx.trace_snd(_lib.SND_GIVEN, ref=ref)

    def relabelling(self, ref=None):
        """relabel.relabel_trace of the last update(): per stored iteration the permutation of its labels that brings it closest to
        ``ref`` (default: ``relabel_ref`` if set, else tau_star), with the costs before and after; kept until the next update()"""
        ref = self.relabel_ref if ref is None else ref
        if self._relabel is None or self._relabel[0] is not ref:
            self._relabel = (ref, _relabel.relabel_trace(self._trace_ctx(), ref))
        return self._relabel[1]

    def tauMeanRelabelled(self):
        """tauMean() with iteration t's haplotype g counted as label relabelling()['perm'][t, g]"""
        return self._ctx.get_tau_sum_perm(self.relabelling()["perm"]) / float(self.max_iter)

    def gammaMeanRelabelled(self):
        """gammaMean() with the columns of every iteration permuted likewise (eta has no haplotype index: etaMean() stands)"""
        return _relabel.gamma_mean_relabelled(self.gamma_store[:self.max_iter], self.relabelling()["perm"])

    def sndPosterior(self, level=0.95):
        """per pair g < h the mean, sd, lo, med, hi of the relabelled within-iteration distance, and the distance in tau_star (map).
        The pairs carry the labels of the relabelling: with ``relabel_ref`` set those are the reference's, and tau_star itself is
        matched to the reference like any iteration, so that map speaks of the same pair of strains as the other columns."""
        perm = self.relabelling()["perm"]
        snd_map = self.calculateSND(self.tau_star)
        if self.relabel_ref is not None:
            ref = _relabel._reference(self, self.relabel_ref)[1]
            own, _ = _relabel.min_cost_assignment(self.compSND(self.tau_star, self._onehot(ref)))   # tau_star's haplotype g is label own[g]
            inv = np.argsort(own)
            snd_map = snd_map[np.ix_(inv, inv)]
        return _relabel.snd_posterior(self._trace_ctx(), perm, level=level, snd_map=snd_map)

    def haplotypeStability(self):
        """per haplotype the mean and max over iterations of the fraction of positions that differ from the reference haplotype after
        relabelling, and the number of iterations in which its label was moved (relabel.haplotype_stability)"""
        return _relabel.haplotype_stability(self._trace_ctx(), self.relabelling())

    # ---- convergence diagnostics of the last update() from the resident trace (desman_amd/diagnose.py)
    def _diag_perm(self):
        """the relabelling the diagnostics are made under: relabelling()['perm'] when relabel_ref is set or a relabelling has been
        computed, else None (the labels as stored)"""
        return self.relabelling()["perm"] if self.relabel_ref is not None or self._relabel is not None else None

    def _diagnosed(self, what, batch_len, make):
        """``make(L, perm)`` kept per (what, L, relabelling) until the next update, as relabelling() is"""
        L = _diagnose.default_batch_len(self.max_iter) if batch_len is None else int(batch_len)
        perm = self._diag_perm()
        key = (what, L)
        if self._diag is None or self._diag[0] is not perm:
            self._diag = (perm, {})
        if key not in self._diag[1]:
            self._diag[1][key] = make(L, perm)
        return self._diag[1][key]

    def _tau_diag(self, batch_len):
        def make(L, perm):
            stats = self._trace_ctx().trace_batch_stats(L, perm=perm)
            return _diagnose.tau_diagnostics(stats), stats["flips"]
        return self._diagnosed("tau", batch_len, make)

    def tauMCSE(self, batch_len=None):
        """[V, G, 4]: the Monte Carlo standard error of tauMean() (of tauMeanRelabelled() under a relabelling) by batch means over the
        last N = B L stored iterations, L = batch_len (default floor(sqrt(max_iter)))"""
        return self._tau_diag(batch_len)[0]["mcse"]

    def tauDiagnostics(self, batch_len=None):
        """per (position, haplotype): ess_min over the bases with 0 < p < 1, rhat_max (split R-hat) over the bases, flips (iterations
        at which the base changed), base (the most frequent one) and its p (diagnose.cell_summary)"""
        d, flips = self._tau_diag(batch_len)
        return _diagnose.cell_summary(d, flips)

    def scalarDiagnostics(self, batch_len=None):
        """mean, sd, mcse, ess, split_rhat of lp, ll and every gamma[s][g] (gamma under the relabelling in force), in that order:
        dict of names (lp, ll, gamma_<s>_<g>) and one array per column"""
        def make(L, perm):
            n = self.max_iter
            g = _diagnose.relabel_gamma(self.gamma_store[:n], perm)
            series = np.concatenate([self.lp_store[:n, None], self.ll_store[:n, None], g.reshape(n, -1)], axis=1)
            d = _diagnose.scalar_diagnostics(series, L)
            d["names"] = ["lp", "ll"] + ["gamma_%d_%d" % (s, h) for s in range(g.shape[1]) for h in range(g.shape[2])]
            return d
        return self._diagnosed("scalars", batch_len, make)

    # ---- Rao-Blackwellised tau marginals of the last update() from the resident traces (desman_amd/marginals.py)
    def _star_labelled(self):
        """tau_star as [V, G] digits under the labels of the relabelling in force: with ``relabel_ref`` set tau_star is matched to the
        reference like any iteration (sndPosterior does the same), otherwise its labels are the stored ones"""
        star = _marginals.tau_digits(self.tau_star)
        if self.relabel_ref is None:
            return star
        ref = _relabel._reference(self, self.relabel_ref)[1]
        own, _ = _relabel.min_cost_assignment(self.compSND(self.tau_star, self._onehot(ref)))       # tau_star's haplotype g is label own[g]
        return star[:, np.argsort(own)]

    def tauMarginals(self, batch_len=None):
        """dict of p, mcse [V, G, 4] -- the average over the last N = B L stored iterations of the exact full conditional of every
        tau[v][g], and its batch-means Monte Carlo standard error (L = batch_len, default floor(sqrt(max_iter))) --, calls (per
        position and haplotype: call, prob, star, agree, entropy; marginals.calls), summary (marginals.summary) and dead; under the
        relabelling the diagnostics are made under; kept until the next update"""
        def make(L, perm):
            m = _marginals.rb_marginals(self._trace_ctx().trace_rb_marginals(L, perm=perm))
            m["calls"] = _marginals.calls(m["p"], self._star_labelled())
            m["summary"] = _marginals.summary(m["calls"], m["dead"])
            return m
        return self._diagnosed("rb", batch_len, make)

    def tauPairs(self, batch_len=None, stride=None):
        """the Rao-Blackwellised joint posterior of the bases of every two haplotypes (marginals.rb_pairs: J, p_same [V, P(, 4, 4)],
        dist, dist_mcse, differ [P], pairs, dead) from every stride-th stored iteration (None: marginals.pairs_stride), with tables
        (marginals.pair_tables of J), flags (marginals.pair_flags against the calls of tauMarginals) and star_dist (the count distance
        of tau_star under the same labels); under the relabelling the diagnostics are made under; kept until the next update"""
        def make(L, perm):
            K = _marginals.pairs_stride(self.max_iter, L) if stride is None else int(stride)
            m = _marginals.rb_pairs(self._trace_ctx().trace_rb_pairs(L, perm=perm, stride=K))
            m["stride"] = K
            m["tables"] = _marginals.pair_tables(m["J"])
            m["flags"] = _marginals.pair_flags(self.tauMarginals(L)["calls"]["prob"], m["pairs"])
            m["star_dist"] = _marginals.star_distance(self._star_labelled(), m["pairs"])
            return m
        return self._diagnosed(("rb_pairs", stride), batch_len, make)

    # ---- posterior predictive fit of the last update() from the resident traces (desman_amd/check.py)
    def fitCheck(self, cells=False):
        """(per-sample table, per-position table) -- with ``cells`` also the [V, S] posterior mean of Pearson's X per cell -- of the
        stored iterations: each table a dict of cells, X2, expected, variance, deviance and z (check.fit_scores).  Invariant to the
        haplotype labels, so no relabelling applies; kept until the next update."""
        if self._fit is None or (cells and "cell" not in self._fit):
            want = ("sample", "position", "cell") if cells else ("sample", "position")
            sums = self._trace_ctx().trace_fit_stats(0, self.max_iter, want=want)
            self._fit = _check.fit_scores(sums, self.max_iter, self.variants)
        f = self._fit
        return (f["sample"], f["position"], f["cell"]) if cells else (f["sample"], f["position"])

    def fitReplicates(self, reps=_check.REPS, stride=None, salt=0):
        """(per-sample table, per-position table) of posterior predictive p-values from ``reps`` replicate tables per used iteration
        (every ``stride``-th stored one; default: about check.N_USE of them): each a dict of T_obs, T_rep, T_rep_sd, p and p_mcse
        (check.ppp_table), the positions' also q, the Benjamini-Hochberg q-value over positions.  Invariant to the haplotype labels."""
        if reps < 1:
            raise ValueError("fitReplicates: at least 1 replicate is needed; got %d" % reps)
        stride = _check.default_stride(self.max_iter) if stride is None else int(stride)
        if stride < 1:
            raise ValueError("fitReplicates: the stride must be at least 1; got %d" % stride)
        ctx = self._trace_ctx()
        calls, _ = _check.ppp_batches(self.max_iter, stride)
        parts = [(ctx.trace_ppc(reps, it0=it0, n_it=n_it, stride=stride, salt=salt), counted) for it0, n_it, counted in calls]
        samples, positions = _check.ppp_table(parts, "sample"), _check.ppp_table(parts, "position")
        positions["q"] = _check.bh_qvalues(positions["p"])
        return samples, positions

    # ---- position-marginal predictive density of the last update() (desman_amd/predictive.py)
    def predictive(self, n_use=_predictive.N_USE, counts=None):
        """The pointwise table (predictive.pointwise: lppd, p_waic, elpd_waic per position) of about ``n_use`` evenly spaced stored
        iterations -- stride max(1, stored // n_use) -- for the positions of the fit or, ``counts`` [N, S, 4], for other positions of the
        same samples (held-out ones: their lppd is the honest score, p_waic does not apply).  Invariant to the haplotype labels."""
        if n_use < 1:
            raise ValueError("predictive: n_use must be at least 1; got %d" % n_use)
        stride = max(1, self.max_iter // int(n_use))
        res = self._trace_ctx().trace_predictive(counts=counts, it0=0, n_it=self.max_iter, stride=stride)
        return _predictive.pointwise(res, self.variants if counts is None else counts, self.G)

    @property
    def tau_store(self):
        """[max_iter, V, G, 4] int64, fetched from the device trace on demand."""
        out = np.empty((self.max_iter, self.V, self.G, 4), dtype=np.int64)
        for it in range(self.max_iter):
            out[it] = self._ctx.get_tau_at(it)
        return out
