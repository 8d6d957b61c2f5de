"""Adversarial tables for the two fp32 screens of the tau sweep (dsm_device.h: screen_certify, sweep_neartie_core):
tables in which ONE step, haplotype g* at position v*, has its uniform a chosen distance delta from an edge of its conditional CDF,
with delta down a ladder from 1e-2 to 1e-9 on both sides of the edge, and every other step beyond doubt.  The random tables of the other
suites put a uniform that close to an edge once in ~1e6 steps; a rounding budget of a screen that is too small shows nowhere else.

The uniform is the one the stream gives that step (oracle/cbind.py: MT19937, or tests/_philox.py).  The knob that moves the edge onto it
is gamma of g* in a PRIVATE sample, one in which only v* has reads: its gamma row touches no other position's conditional.  The knob is
solved by bisection on the step's conditional CDF (c_sample_tau.c:136-170 with its `(double)(float)` cast at :164) evaluated in mpmath at
60 digits, rounded to a double, and the table is then evaluated again, every step of it, at the doubles it holds: the achieved distance
and the exact draw are recorded, and every other step has its uniform farther than FAR from each of its edges.

Two kinds of step:
* totals: all haplotypes carry base b0 at v* and the three other bases have equal counts in every sample, so the three other candidates
  tie and weigh w = 3 x 2^-gap together -- the very bound screen_certify uses.  b0 = 3 puts the edge below `best` at w / (1 + w) next to a
  small uniform (the lower side of best's interval), b0 = 0 puts best's own edge 1 / (1 + w) next to a uniform near 1 (the upper side).
  The error matrix is a noisy one (0.7 on the diagonal) and the position has ~16000 reads, so that reads consistent with the state give
  totals of ~20000 bits (an fp32 ulp there is 2e-3), against the 1.4e-4 bits of slack that the screen's factor 3.0003 has over 3.  What
  these tables can and cannot tell: with the budget E taken out altogether the device draws a wrong base on the 1e-9 rung, with E / 4 it
  draws none -- the error of a GAP between two totals is far smaller than that of a total (presumably the candidates' sums run through nearly the
  same roundings; not examined), so the ladder detects a missing budget, not one that is merely too small by a factor of a few.  (The fp64 reference
  is still unambiguous at 1e-9: its own error on such a total, ~20000 x 2^-53, moves an edge at u <= 3e-5 by less than 1e-16.)
* near-tie: g* has gamma ~ 1e-3 in every sample (the recipe of tests/test_gpu_parity.py), its conditional is flat, and the private
  sample's few reads of a base nobody else carries move an inner edge C_1, C_2 or C_3 onto the uniform.

The uniform of a totals step is scanned for in [max(1e-6, 3 delta), max(3e-5, 30 delta)] (for 1 - u likewise), so that the three others'
weight w ~ u is never smaller than delta; at delta = 1e-2 that window is [1.5e-2, 5e-2], the one place above 1e-2.

The fixture tests/golden/screen_edges.npz is written by `python -m tests._screen_edges --write` (needs mpmath); reading it, rebuilding a
table from it and the float32 restatement of screen_certify need numpy only.  The restatement is a helper that says on which rungs the
screen as written would certify; it is not an oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from oracle import cbind  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "screen_edges.npz")
MP_DPS = 60
LADDER = (1e-2, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9)
FAR = 1.0e-3                                  # every step but the adversarial one: |u - edge| above this for its three edges
GMAX = 12
V = 10
TOTALS, NEARTIE = 0, 1
MT, PHILOX = 0, 1
ETA_NOISY = 0.6 * np.eye(4) + 0.1              # totals tables: rows sum to 1
ETA_SHARP = 0.96 * np.eye(4) + 0.01            # near-tie tables: the matrix of the parity recipe

# (kind, S, G, g*, stream): one S per tiling of tau_shape at G = 4; both ends of the carried prefix at S = 64 (the fp32 prefix form);
# three G at S = 24 and 64; the near-tie shapes; three shapes again on the Philox stream
SHAPES = [(TOTALS, S, 4, 2, MT) for S in (16, 32, 48, 96, 128, 192, 256, 384, 512)] + [(TOTALS, 64, 4, 0, MT), (TOTALS, 64, 4, 3, MT)] + \
         [(TOTALS, S, G, G // 2, MT) for S in (24, 64) for G in (2, 9, 12)] + \
         [(NEARTIE, 16, 4, 1, MT), (NEARTIE, 64, 5, 4, MT), (NEARTIE, 96, 4, 0, MT), (NEARTIE, 200, 3, 2, MT)] + \
         [(TOTALS, 16, 4, 2, PHILOX), (TOTALS, 64, 4, 3, PHILOX), (NEARTIE, 200, 3, 2, PHILOX)]


def shape_name(sh):
    kind, S, G, gs, rng = sh
    return "%s-S%d-G%d-g%d-%s" % ("totals" if kind == TOTALS else "neartie", S, G, gs, "mt" if rng == MT else "philox")


def tau_shape(S):
    """(lanes per position, samples per lane) of the sweep kernels (kernels_gibbs.hip: tau_shape)"""
    if S <= 16:
        return 16, 1
    if S <= 32:
        return 16, 2
    if S <= 48:
        return 16, 3
    if S <= 64:
        return 32, 2
    if S <= 96:
        return 32, 3
    need = (S + 63) // 64
    return 64, (need if need <= 4 else (6 if need <= 6 else 8))


# ------------------------------------------------------------------------------------------------------------------- the base tables
def _spread(S, n, skip):
    """n sample indices spread over 0 .. S - 1 (every lane and slot of the tiling gets some), without `skip`"""
    idx = [s for s in np.unique(np.linspace(0, S - 1, min(n, S)).round().astype(int)) if s != skip]
    return np.array(idx, dtype=np.int64)


def _pick(lst, n):
    """n members of a list, spread over it"""
    lst = np.asarray(lst, dtype=np.int64)
    return lst[np.unique(np.linspace(0, len(lst) - 1, min(n, len(lst))).round().astype(int))]


def base_table(sh):
    """Everything of a shape's tables that does not depend on the case: the ordinary positions (counts, start), gamma of the samples that
    are not private, the shares of the private row, eta, the private sample, and per variant of the adversarial position (totals: b0 = 3
    and b0 = 0; near-tie: private reads of base 3 and of base 0) its counts and its start row."""
    kind, S, G, gs, _ = sh
    rng = np.random.default_rng(1000 * S + 10 * G + gs + 7 * kind)
    sp = (7 * S) // 11                                              # the private sample
    others = [h for h in range(G) if h != gs]
    gamma = np.zeros((S, G))
    if kind == TOTALS:
        eta = ETA_NOISY.copy()
        # g* is a minor component (0.007) in the samples where the adversarial position has its reads -- reads consistent with the state
        # then leave its step near a tie of best and the rest, and the private sample sets the gap -- and an ordinary component in every
        # third sample, where the ordinary positions have theirs: their steps of g* are sharp, so that on the device the verdict of a
        # wavefront's step g* is the adversarial step's own (a step goes to fp64 when ANY position of the wavefront declines)
        gamma[:, gs] = 0.007
        gamma[:, others] = rng.dirichlet(np.full(len(others), 3.0), size=S) * 0.993
        rest = [s for s in range(S) if s != sp]
        smp, ss = _pick(rest[0::3], 24), _pick([s for i, s in enumerate(rest) if i % 3], 96)
        gamma[smp] = rng.dirichlet(np.full(G, 3.0), size=len(smp))
        depth = 400
    else:
        eta = ETA_SHARP.copy()
        gamma[:, gs] = rng.uniform(2.0e-4, 2.0e-3, size=S)
        gamma[:, others] = rng.dirichlet(np.full(len(others), 3.0), size=S) * (1.0 - gamma[:, gs])[:, None]
        depth, smp = 40, _spread(S, 24, sp)
    share = rng.dirichlet(np.full(G, 3.0))
    share[gs] = 0.0
    share = share / share.sum()
    # ordinary positions: reads in up to 24 samples, drawn from the mixture of a generating row; a quarter of the start is random
    tau_true = rng.integers(0, 4, size=(V, G))
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        p = gamma[smp] @ eta[tau_true[v]]
        for i, s in enumerate(smp):
            counts[v, s] = rng.multinomial(rng.poisson(depth), p[i] / p[i].sum())
    start = tau_true.copy()
    flip = rng.random((V, G)) < 0.25
    start[flip] = rng.integers(0, 4, size=int(flip.sum()))
    special = {}
    for b0 in (3, 0):
        x = np.zeros((S, 4), dtype=np.int64)
        if kind == TOTALS:
            # ~16000 reads over up to 96 samples, 70 % of base b0, the same number of each other base in a sample (the three others tie)
            per = 16000.0 / len(ss)
            for s in ss:
                m = max(1, int(round(0.10 * per + rng.uniform(-0.3, 0.3))))
                x[s, :] = m
                x[s, b0] = max(1, int(round(0.70 * per + rng.uniform(-0.5, 0.5))))
            x[sp, b0] = 40
            row = np.full(G, b0, dtype=np.int64)
        else:
            # the live haplotypes carry bases other than b0, the reads of the other samples follow their mixture; the private sample has
            # eight reads of b0, which only g* can explain
            row = np.array([(b0 + 1 + (i % 3)) % 4 for i in range(G)], dtype=np.int64)
            p = gamma[smp] @ eta[row]
            for i, s in enumerate(smp):
                x[s] = rng.multinomial(rng.poisson(depth), p[i] / p[i].sum())
            x[sp, b0] = 8
        special[b0] = (x, row)
    return dict(sh=sh, S=S, G=G, gs=gs, kind=kind, sp=sp, gamma=gamma, share=share, eta=eta, counts=counts, start=start, special=special)


def private_row(base, x):
    """gamma of the private sample as doubles: x for g*, the rest shared out among the others"""
    row = base["share"] * (1.0 - x)
    row[base["gs"]] = x
    return row


def table(base, b0, vstar, grow):
    """(counts int64 [V,S,4], tau one-hot, gamma, eta) of a case: position vstar is the adversarial one, the private row is grow"""
    counts = base["counts"].copy()
    idx = base["start"].copy()
    counts[vstar], idx[vstar] = base["special"][b0]
    gamma = base["gamma"].copy()
    gamma[base["sp"]] = grow[:base["G"]]
    return np.ascontiguousarray(counts), cbind.idx_to_onehot(idx), np.ascontiguousarray(gamma), np.ascontiguousarray(base["eta"])


# ------------------------------------------------------------------------------------------------------------------- the streams
def uniforms(rng, seed, G):
    """the V G uniforms of a table's first sweep, in the order cbind.sample_tau_u consumes them"""
    if rng == MT:
        return cbind.MT19937(int(seed)).uniform(V * G)
    from _philox import tau_uniforms
    return tau_uniforms(int(seed), 0, V, G)


def _scan(rng, start, G, n):
    """uniforms [n, V G] of seeds start .. start + n - 1"""
    if rng == MT:
        return np.stack([cbind.MT19937(start + i).uniform(V * G) for i in range(n)])
    import _philox as P
    i = np.arange(V * G, dtype=np.uint64)
    ctr = np.stack([i, np.zeros_like(i), np.zeros_like(i), np.full_like(i, P.STREAM_TAUU)], axis=1)
    seeds = np.arange(start, start + n, dtype=np.uint64)
    key = np.stack([seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)], axis=1)
    w = P.philox4x32_10(np.tile(ctr, (n, 1)), np.repeat(key, V * G, axis=0))[:, 0]
    return w.reshape(n, V * G).astype(np.float64) / 4294967296.0


# ------------------------------------------------------------------------------------------------------------------- mpmath
def _mp():
    import mpmath
    mpmath.mp.dps = MP_DPS
    return mpmath


def mp_edges(x, row, g, gamma, eta):
    """the three inner CDF edges of the step of haplotype g at a position with counts x [S,4] and bases row [G], exactly: the totals of
    c_sample_tau.c:136-169 (counts through float), normaliseLog4 and sample4's running sums without any rounding"""
    mp = _mp()
    G = len(row)
    tot = [mp.mpf(0)] * 4
    for s in np.nonzero(x.sum(axis=1))[0]:
        gm = [mp.mpf(float(gamma[s, h])) for h in range(G)]
        for b in np.nonzero(x[s])[0]:
            rest = mp.fsum(mp.mpf(float(eta[row[h], b])) * gm[h] for h in range(G) if h != g)
            c = mp.mpf(float(np.float32(x[s, b])))
            for a in range(4):
                tot[a] = tot[a] + c * mp.log(rest + mp.mpf(float(eta[a, b])) * gm[g])
    mx = max(tot)
    e = [mp.exp(t - mx) for t in tot]
    sm = mp.fsum(e)
    return (e[0] / sm, (e[0] + e[1]) / sm, (e[0] + e[1] + e[2]) / sm)


def _draw(edges, u):
    return 0 if u < edges[0] else 1 if u < edges[1] else 2 if u < edges[2] else 3


def mp_sweep(counts, idx, gamma, eta, u, cache=None, key=None):
    """one exact sweep: (new bases [V,G], signed distance u - nearest edge [V,G] as floats).  cache: edges of the ordinary positions by
    (key, v, g, row) -- their conditionals do not see the private row"""
    mp = _mp()
    idx = np.array(idx, dtype=np.int64)
    Vn, G = idx.shape
    dist = np.zeros((Vn, G))
    for v in range(Vn):
        for g in range(G):
            k = (key, v, g, tuple(idx[v])) if key is not None else None
            if cache is not None and k in cache:
                ed = cache[k]
            else:
                ed = mp_edges(counts[v], idx[v], g, gamma, eta)
                if cache is not None and k is not None:
                    cache[k] = ed
            uu = mp.mpf(float(u[v * G + g]))
            idx[v, g] = _draw(ed, uu)
            d = min((uu - e for e in ed), key=abs)
            dist[v, g] = float(d)
    return idx, dist


# ------------------------------------------------------------------------------------------------------------------- one case
def cases_of(sh):
    """the cases of a shape as (b0, edge k, side, delta): u - C_k = side * delta.  Totals: the lower side of best's interval (b0 = 3, the
    edge below it) and the upper (b0 = 0, its own edge).  Near-tie: the three inner edges in turn; private reads of base 3 move the
    edges over the lower half of (0, 1), of base 0 over the upper half."""
    out = []
    if sh[0] == TOTALS:
        for b0, k in ((3, 2), (0, 0)):
            for d in LADDER:
                for side in (1, -1):
                    out.append((b0, k, side, d))
    else:
        for k in (0, 1, 2):
            for i, d in enumerate(LADDER):
                for side in (1, -1):
                    out.append((3 if (i + k) % 2 == 0 else 0, k, side, d))
    return out


# Rungs taken out of a shape because the reference's own fp64 sweep does not give the exact draw there (its error, ~|l| 2^-53 on a
# total, reaches the distance): {shape name: (delta, ...)}.  Only the 1e-9 rung may ever be listed.  None is: the reference agrees with
# mpmath on every case of every shape.
DROPPED = {}


def _solve(f, lo, hi):
    """root of the monotone f on [lo, hi] by bisection in mpmath"""
    mp = _mp()
    lo, hi = mp.mpf(lo), mp.mpf(hi)
    flo, fhi = f(lo), f(hi)
    if not (flo < 0 < fhi or fhi < 0 < flo):
        return None
    for _ in range(190):
        mid = (lo + hi) / 2
        fm = f(mid)
        if (fm < 0) == (flo < 0):
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def _knob_edges(base, b0, k):
    """x -> edge C_k of the adversarial step with the private row at a real x (mpmath), the other samples' part computed once"""
    mp = _mp()
    xs, row = base["special"][b0]
    gs, sp, G, eta, gamma = base["gs"], base["sp"], base["G"], base["eta"], base["gamma"]
    rest_x = xs.copy()
    rest_x[sp] = 0
    fixed = [mp.mpf(0)] * 4
    for s in np.nonzero(rest_x.sum(axis=1))[0]:
        gm = [mp.mpf(float(gamma[s, h])) for h in range(G)]
        for b in np.nonzero(rest_x[s])[0]:
            rest = mp.fsum(mp.mpf(float(eta[row[h], b])) * gm[h] for h in range(G) if h != gs)
            c = mp.mpf(float(np.float32(rest_x[s, b])))
            for a in range(4):
                fixed[a] = fixed[a] + c * mp.log(rest + mp.mpf(float(eta[a, b])) * gm[gs])
    share = [mp.mpf(float(t)) for t in base["share"]]

    def edge(x):
        tot = list(fixed)
        for b in np.nonzero(xs[sp])[0]:
            rest = mp.fsum(mp.mpf(float(eta[row[h], b])) * share[h] * (1 - x) for h in range(G) if h != gs)
            c = mp.mpf(float(np.float32(xs[sp, b])))
            for a in range(4):
                tot[a] = tot[a] + c * mp.log(rest + mp.mpf(float(eta[a, b])) * x)
        mx = max(tot)
        e = [mp.exp(t - mx) for t in tot]
        return mp.fsum(e[:k + 1]) / mp.fsum(e)
    return edge


class Builder:
    """the cases of one shape; keeps what they share (base table, knob functions, the ordinary positions' exact edges)"""

    def __init__(self, sh):
        self.sh, self.base, self.cache, self.knob = sh, base_table(sh), {}, {}
        self.xr = (0.002, 0.9) if sh[0] == TOTALS else (1.0e-4, 9.0e-3)     # near-tie: g* stays rare (gamma <= 0.01 in every sample)

    def _edge_fn(self, b0, k):
        if (b0, k) not in self.knob:
            f = _knob_edges(self.base, b0, k)
            self.knob[(b0, k)] = (f, float(f(self.xr[0])), float(f(self.xr[1])))
        return self.knob[(b0, k)]

    def _window(self, b0, k, delta):
        """the uniforms looked for, as (lo, hi, mirrored): mirrored -> the window is on 1 - u"""
        if self.sh[0] == TOTALS:
            lo, hi = (1.5e-2, 5.0e-2) if delta == 1e-2 else (max(1.0e-6, 3.0 * delta), max(3.0e-5, 30.0 * delta))
            return lo, hi, b0 == 0
        _, e0, e1 = self._edge_fn(b0, k)
        lo, hi = min(e0, e1), max(e0, e1)
        return lo + 0.1 * (hi - lo) + delta, hi - 0.1 * (hi - lo) - delta, False

    def case(self, i):
        """case i of the shape: dict(seed, vstar, grow, dist, draw, ...), deterministic (the same scan, the same arithmetic)"""
        mp = _mp()
        b0, k, side, delta = cases_of(self.sh)[i]
        base, G, gs, rng = self.base, self.base["G"], self.base["gs"], self.sh[4]
        f, _, _ = self._edge_fn(b0, k)
        lo, hi, mirrored = self._window(b0, k, delta)
        seed0, chunk = 1 + 1000003 * i, 256
        for start in range(seed0, seed0 + 400 * chunk, chunk):
            us = _scan(rng, start, G, chunk)
            col = us[:, gs::G]
            w = 1.0 - col if mirrored else col
            for si, vstar in zip(*np.nonzero((w >= lo) & (w <= hi))):
                seed, u = start + int(si), us[si]
                ustar = mp.mpf(float(u[vstar * G + gs]))
                x = _solve(lambda t: ustar - f(t) - side * delta, *self.xr)
                if x is None:
                    continue
                grow = private_row(base, float(x))
                counts, tau, gamma, eta = table(base, b0, int(vstar), grow)
                idx0 = cbind.onehot_to_idx(tau).astype(np.int64)
                # the ordinary positions from the cache, the adversarial one afresh: every step but (v*, g*) far from its edges
                new, dist = mp_sweep(base["counts"], base["start"], gamma, eta, u, self.cache, key="ord")
                one, d1 = mp_sweep(counts[vstar:vstar + 1], idx0[vstar:vstar + 1], gamma, eta, u[vstar * G:(vstar + 1) * G])
                new[vstar], dist[vstar] = one[0], d1[0]
                far = np.abs(dist) > FAR
                far[vstar, gs] = True
                others_kept = all(one[0][h] == idx0[vstar, h] for h in range(gs))     # the rest mixture of the step is the built one
                ed = mp_edges(counts[vstar], np.concatenate([one[0][:gs], idx0[vstar, gs:]]), gs, gamma, eta)
                got = ustar - ed[k]
                if not (far.all() and others_kept and abs(got - side * delta) < 1e-3 * delta):
                    continue
                g12 = np.zeros(GMAX)
                g12[:G] = grow
                return dict(b0=b0, k=k, side=side, delta=delta, seed=seed, vstar=int(vstar), grow=g12, dist=float(got),
                            draw=int(_draw(ed, ustar)), new=new)
        raise RuntimeError("%s case %d: no stream position found" % (shape_name(self.sh), i))


# ------------------------------------------------------------------------------------------------------------------- the fixture
_CASE_FIELDS = (("b0", np.int64), ("k", np.int64), ("side", np.int64), ("delta", np.float64), ("seed", np.uint64), ("vstar", np.int64),
                ("dist", np.float64), ("draw", np.int64))


def write(path=FIXTURE):
    out = {}
    for si, sh in enumerate(SHAPES):
        b = Builder(sh)
        cs = [b.case(i) for i in range(len(cases_of(sh))) if cases_of(sh)[i][3] not in DROPPED.get(shape_name(sh), ())]
        for name, dt in _CASE_FIELDS:
            out["s%d_%s" % (si, name)] = np.array([c[name] for c in cs], dtype=dt)
        out["s%d_grow" % si] = np.stack([c["grow"] for c in cs])
        out["s%d_new" % si] = np.stack([c["new"] for c in cs]).astype(np.uint8)
        out.update(_base_arrays(si, b.base))
        print("%-28s %d cases, |u - edge| / delta - 1 at most %.1e" % (shape_name(sh), len(cs),
              max(abs(abs(c["dist"]) / c["delta"] - 1.0) for c in cs)), flush=True)
    out["shapes"] = np.array(SHAPES, dtype=np.int64)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    return path


_BASE_FIELDS = (("gamma", np.float64), ("share", np.float64), ("eta", np.float64), ("counts", np.int32), ("start", np.uint8))


def _base_arrays(si, base):
    """a base table as the fixture holds it: gamma, shares and eta as the doubles they are, counts and bases as small integers"""
    out = {"s%d_%s" % (si, name): np.asarray(base[name]).astype(dt) for name, dt in _BASE_FIELDS}
    out["s%d_sp" % si] = np.int64(base["sp"])
    for b0 in (3, 0):
        out["s%d_x%d" % (si, b0)] = base["special"][b0][0].astype(np.int32)
        out["s%d_row%d" % (si, b0)] = base["special"][b0][1].astype(np.uint8)
    return out


def _base_from(z, si, sh):
    base = dict(sh=sh, kind=sh[0], S=sh[1], G=sh[2], gs=sh[3], sp=int(z["s%d_sp" % si]))
    for name, dt in _BASE_FIELDS:
        a = z["s%d_%s" % (si, name)]
        base[name] = a if dt == np.float64 else a.astype(np.int64)
    base["special"] = {b0: (z["s%d_x%d" % (si, b0)].astype(np.int64), z["s%d_row%d" % (si, b0)].astype(np.int64)) for b0 in (3, 0)}
    return base


def load(path=FIXTURE):
    """[(shape, base table, [case dict, ...]), ...], all of it from the file"""
    z = np.load(path)
    assert [tuple(int(t) for t in r) for r in z["shapes"]] == SHAPES
    out = []
    for si, sh in enumerate(SHAPES):
        n = len(z["s%d_seed" % si])
        cs = [dict({name: z["s%d_%s" % (si, name)][i].item() for name, _ in _CASE_FIELDS}, grow=z["s%d_grow" % si][i],
                   new=z["s%d_new" % si][i]) for i in range(n)]
        out.append((sh, _base_from(z, si, sh), cs))
    return out


def case_table(base, c):
    return table(base, c["b0"], c["vstar"], c["grow"])


# The shape whose cases also run through the sweeps that have no screen (held sweep, gene sampler).  The gene sampler masks gamma by the
# gene's haplotypes and re-normalises every sample (Eta_Sampler.py:355-369), so a gene that all haplotypes carry sweeps on gamma / its row
# sums: the table's gamma moved in its last bits, which moves an edge by ~1e-20 -- the two nearest rungs stay the cases they are
# (tests/test_screen_edges_cpu.py checks the distance again at the masked gamma).
GENE_SHAPE = (TOTALS, 32, 4, 2, MT)


def masked_gamma(gamma):
    """maskGamma with every haplotype in the gene (oracle/ref_genes.py: mask_gamma)"""
    from oracle import ref_genes
    return np.ascontiguousarray(ref_genes.mask_gamma(gamma, np.ones(gamma.shape[1], dtype=np.int64)))


def gene_cases(cs):
    """the cases of GENE_SHAPE that the gene sampler runs: the 1e-8 and 1e-9 rungs, both edges, both sides"""
    return [(i, c) for i, c in enumerate(cs) if c["delta"] <= 1e-8]


# ------------------------------------------------------------------------------------------------------------------- screen_certify in float32
def screen_would_certify(x, row, g, gamma, eta, uw, S):
    """screen_certify (dsm_device.h) as written, in numpy float32, on totals formed as sweep_screen forms them (fp32 inputs, one fma per
    link, log2 in fp32): (certifies, best).  numpy's log2 is not the hardware's and the sums run in another order, so this says where on
    a ladder the verdict changes, not what the device does at a single borderline case."""
    f = np.float32
    G = len(row)
    _, NSL = tau_shape(S)
    e32, g32 = eta.astype(f), gamma.astype(f)
    s32 = np.zeros((S, 4), dtype=f)
    for h in range(G):
        if h != g:
            s32 = (e32[row[h]][None, :].astype(np.float64) * g32[:, h, None].astype(np.float64) + s32.astype(np.float64)).astype(f)
    c32 = np.zeros(4, dtype=f)
    xs = x.astype(f)
    for a in range(4):
        P = (e32[a][None, :].astype(np.float64) * g32[:, g, None].astype(np.float64) + s32.astype(np.float64)).astype(f)
        c32[a] = (xs * np.log2(P)).sum(dtype=f)
    xtot = f(xs.sum(dtype=f) * f(1.0001))
    best = int(np.argmax(c32))
    m = c32[best]
    second = max(c32[a] for a in range(4) if a != best)
    e2 = f((xtot * f(f(1.4427) * f(G + 4) + f(4.0)) + f(abs(m) + f(128.0)) * f(4 * NSL + 11)) * f(1.1920929e-7))
    t = f(f(3.0003) * np.exp2(min(f(second - m + e2), f(0.0)), dtype=f))
    u = f(f(uw) * f(2.3283064365386963e-10))
    ok = bool(abs(m) < f(3.0e38)) and bool(f(u * f(0.9999995)) > t) and bool(f(u * f(1.0000005)) < f(f(1.0) - t))
    return ok, best


if __name__ == "__main__":
    if "--write" in sys.argv:
        print(write())
    else:
        print("usage: python -m tests._screen_edges --write")
