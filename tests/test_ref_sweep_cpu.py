"""The oracle's tau sweep (oracle/desman_oracle.c: orc_sample_tau_u / orc_sample_tau, orc_initRNG / orc_setRNG) against the reference's OWN
compiled sweep (sampletau/c_sample_tau.c, unmodified, in oracle/_ref -- tests/_ref_sweep.py), exactly: tau element by element and nchange,
every sweep, no tolerance.  Every other exactness test of the project compares with that restatement; this file is what pins it: the
`(float)` cast of the counts, normaliseLog4 / sample4 with the forced last edge under -inf and NaN, "first 1 wins", the h != g order, the
process-global generator carried over between calls, seed 0 -> 4357.  Both sides are plain, non-contracted C: any difference is a bug."""
import numpy as np
import pytest

import _ref_sweep as R
from oracle import cbind


@pytest.fixture(scope="module")
def ref():
    return R.reference()


def oracle_sweeps(tau, pi, eta, counts, seed, n=R.N_SWEEPS, order="vg"):
    """n oracle sweeps on one MT19937 stream consumed in (v-major, g-minor) order -- or, order="gv", handed over transposed"""
    V, G, _ = tau.shape
    mt = cbind.MT19937(0 if seed is None else seed)
    t = tau.copy()
    out = []
    for _ in range(n):
        u = mt.uniform(V * G)
        if order == "gv":
            u = np.ascontiguousarray(u.reshape(G, V).T).reshape(-1)
        out.append((None, cbind.sample_tau_u(t, pi, eta, counts, u)))
        out[-1] = (t.copy(), out[-1][1])
    return out


# ------------------------------------------------------------------------------------------------------------------- shape grid
@pytest.mark.parametrize("start", ["random", "generating"])
@pytest.mark.parametrize("V", [1, 3, 40])
@pytest.mark.parametrize("G", [1, 2, 5, 12, 32])
@pytest.mark.parametrize("S", [1, 2, 16, 17, 130])
def test_oracle_sweep_is_the_reference_sweep(ref, S, G, V, start):
    counts, tau, pi, eta = R.state(V, S, G, start, seed=1000 * S + 10 * G + V)
    seed = 7 * S + G
    want = R.ref_sweeps(ref, tau, pi, eta, counts, seed)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, seed), want, "orc_sample_tau_u")
    # the oracle's own process-global generator, the same call sequence
    cbind.initRNG(); cbind.setRNG(seed)
    t = tau.copy()
    got = []
    for _ in range(R.N_SWEEPS):
        n = cbind.sample_tau(t, pi, eta, counts)
        got.append((t.copy(), n))
    cbind.freeRNG()
    R.assert_same(got, want, "orc_sample_tau")


# ------------------------------------------------------------------------------------------------------------------- generator
def _case(V=12, S=6, G=5, seed=77):
    return R.state(V, S, G, "random", seed)


def test_draws_continue_across_calls_without_reseeding(ref):
    """c_sample_tau call k starts where call k - 1 stopped: three calls of V G draws are one stream of 3 V G words -- and not three
    times the first V G (the sweeps from one start would then repeat themselves)"""
    counts, tau, pi, eta = _case()
    V, G, _ = tau.shape
    ref.c_initRNG(); ref.c_setRNG(31)
    u = cbind.MT19937(31).uniform(3 * V * G)
    outs = []
    for k in range(3):
        t, o = tau.copy(), tau.copy()                                 # every call from the same start: only the uniforms differ
        n = ref.c_sample_tau(t, pi, eta, counts)
        assert n == cbind.sample_tau_u(o, pi, eta, counts, u[k * V * G:(k + 1) * V * G]) and np.array_equal(t, o), k
        outs.append(t)
    ref.c_freeRNG()
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


def test_unseeded_stream_is_seed_4357_and_so_is_seed_0(ref):
    """gsl_rng_alloc leaves the default seed, which for mt19937 is 4357; c_setRNG(0) gives that stream too.  The oracle: MT19937(0),
    MT19937(4357), orc_initRNG alone, orc_setRNG(0)."""
    counts, tau, pi, eta = _case()
    unseeded = R.ref_sweeps(ref, tau, pi, eta, counts, None)
    R.assert_same(R.ref_sweeps(ref, tau, pi, eta, counts, 0), unseeded, "c_setRNG(0)")
    R.assert_same(R.ref_sweeps(ref, tau, pi, eta, counts, 4357), unseeded, "c_setRNG(4357)")
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 0), unseeded, "MT19937(0)")
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 4357), unseeded, "MT19937(4357)")
    assert not np.array_equal(R.ref_sweeps(ref, tau, pi, eta, counts, 1)[0][0], unseeded[0][0])
    for reseed in (False, True):
        cbind.initRNG()
        if reseed:
            cbind.setRNG(0)
        t = tau.copy()
        got = []
        for _ in range(R.N_SWEEPS):
            n = cbind.sample_tau(t, pi, eta, counts)
            got.append((t.copy(), n))
        cbind.freeRNG()
        R.assert_same(got, unseeded, "orc_initRNG" + (" + orc_setRNG(0)" if reseed else ""))


def test_reseeding_mid_stream(ref):
    """seed, sweep, sweep, seed again, sweep: the third sweep draws the words of the first; same calls to the oracle's global generator"""
    counts, tau, pi, eta = _case()
    V, G, _ = tau.shape
    u = cbind.MT19937(5).uniform(2 * V * G)
    ref.c_initRNG(); ref.c_setRNG(5)
    cbind.initRNG(); cbind.setRNG(5)
    t, o, e = tau.copy(), tau.copy(), tau.copy()
    for k, words in enumerate((u[:V * G], u[V * G:], u[:V * G])):
        if k == 2:
            ref.c_setRNG(5); cbind.setRNG(5)
        n = ref.c_sample_tau(t, pi, eta, counts)
        assert n == cbind.sample_tau(o, pi, eta, counts) and np.array_equal(t, o), k
        assert n == cbind.sample_tau_u(e, pi, eta, counts, words) and np.array_equal(t, e), k
    ref.c_freeRNG(); cbind.freeRNG()


def test_uniforms_are_consumed_position_major(ref):
    """cbind.MT19937(seed).uniform handed to the oracle as u[v G + g] is the reference's order of draws; the transposed order is another
    result (so the comparison can tell)"""
    counts, tau, pi, eta = _case(V=9, S=6, G=4, seed=78)
    want = R.ref_sweeps(ref, tau, pi, eta, counts, 12)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 12), want, "u[v G + g]")
    assert not np.array_equal(oracle_sweeps(tau, pi, eta, counts, 12, order="gv")[0][0], want[0][0])


# ------------------------------------------------------------------------------------------------------------------- (float) cast
def test_counts_go_through_float_before_the_product(ref):
    """c_sample_tau.c:164 on counts the cast rounds (tests/_ref_sweep.py: float_cast_table).  Not vacuous: a plain numpy fp64 evaluation
    of the same sweep with exact counts draws other bases at several steps -- steps whose uniform is far (> 1e-3) from every cdf edge of
    both evaluations, where summation order cannot matter -- and with the counts through float32 first it draws the reference's."""
    counts, tau, pi, eta = R.float_cast_table()
    V, G, _ = tau.shape
    want = R.ref_sweeps(ref, tau, pi, eta, counts, R.FLOAT_CAST_SEED)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, R.FLOAT_CAST_SEED), want, "float-cast table")
    u = cbind.MT19937(R.FLOAT_CAST_SEED).uniform(V * G)
    idx_cast, d_cast = R.numpy_sweep(tau, pi, eta, counts, u, cast=True)
    idx_exact, d_exact = R.numpy_sweep(tau, pi, eta, counts, u, cast=False)
    clear = (np.minimum(d_cast, d_exact) > 1e-3)[:, 0]
    differ = (idx_cast[:, 0] != idx_exact[:, 0]) & clear
    print("steps g = 0 decided by the cast: %d of %d" % (int(differ.sum()), V))
    assert differ.sum() >= 3
    ref_idx = cbind.onehot_to_idx(want[0][0])
    assert np.array_equal(ref_idx[clear, 0], idx_cast[clear, 0])
    assert (ref_idx[differ, 0] != idx_exact[differ, 0]).all()


# ------------------------------------------------------------------------------------------------------------------- degenerate operands
@pytest.mark.parametrize("kind", R.DEGENERATE)
def test_degenerate_operands_land_on_the_reference_base(ref, kind):
    """DESIGN.md sec. 4 "Degenerate inputs": -inf and NaN run through the candidate sums, the softmax and the inverse-cdf walk of the
    reference as plain IEEE arithmetic; the restatement walks the same way"""
    counts, tau, pi, eta, seed = R.degenerate_table(kind)
    want = R.ref_sweeps(ref, tau, pi, eta, counts, seed)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, seed), want, kind)
    if kind == "all_neg_inf_and_nan":                                 # the case is what it says (haplotype 0, the only one with abundance)
        _, logp = cbind.sample_tau_u(tau.copy(), pi, eta, counts, cbind.MT19937(seed).uniform(tau.shape[0] * tau.shape[1]), want_logp=True)
        assert np.isneginf(logp[0::2, 0, :]).all() and np.isnan(logp[1::2, 0, :]).any()
        assert (cbind.onehot_to_idx(want[0][0])[0::2, 0] == 3).all()  # NaN everywhere: no edge test holds, the last edge is forced


# ------------------------------------------------------------------------------------------------------------------- one-hot decoding
def test_rows_with_two_ones_decode_to_the_first(ref):
    """c_sample_tau.c:116-122 takes the first 1 of a row and breaks; a change clears that digit and sets the drawn one, so the second 1
    stays where it was.  (Rows without any 1 are left out: the reference reads its index array uninitialised there.)"""
    counts, tau, pi, eta = _case(V=20, S=6, G=5, seed=79)
    rs = np.random.RandomState(3)
    first = cbind.onehot_to_idx(tau)
    extra = rs.randint(4, size=first.shape)
    two = rs.rand(*first.shape) < 0.5
    tau[two, extra[two]] = 1                                          # a second 1 after or before the first (or on it: none added)
    assert (tau.sum(axis=2) == 2).sum() > 20 and (np.argmax(tau == 1, axis=2) != first).any()
    want = R.ref_sweeps(ref, tau, pi, eta, counts, 44)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 44), want, "two 1s")
    assert (want[-1][0].sum(axis=2) >= 2).any()


# ------------------------------------------------------------------------------------------------------------------- h != g order
def test_the_other_haplotypes_are_summed_in_ascending_order(ref):
    """c_sample_tau.c:138-147 adds the other haplotypes' terms to 0.0 with h ascending.  Another order moves a mixture value by an ulp at
    most -- which decides nothing on an ordinary table, so this one is built to be decided by it.  One sample, four haplotypes, all on
    base 0, abundances (2^-53, 1, 2^-53, 2^-53), error column of base 0 = (1, 1/2, 0, 0), 2^53 reads of base 0 (a float exactly).  For
    haplotype 0, ascending: (1 + 2^-53) + 2^-53 = 1 (each sum a tie, to even), every candidate's mixture rounds to 1 and all four totals
    are 2^53 log 1 = 0: a uniform draw.  Descending: (2^-53 + 2^-53) + 1 = 1 + 2^-52, candidate 0 rounds up to 1 + 2^-51, and the totals
    are about (4, 2, 2, 2): candidate 0 at 0.71.  So the first draws of the V positions are uniform over the four bases only if the order
    is the reference's."""
    V, G = 24, 4
    e = 2.0 ** -53
    pi = np.array([[e, 1.0, e, e]])
    eta = np.full((4, 4), 0.1)
    eta[:, 0] = [1.0, 0.5, 0.0, 0.0]
    counts = np.zeros((V, 1, 4), dtype=np.int64); counts[:, 0, 0] = 1 << 53
    tau = cbind.idx_to_onehot(np.zeros((V, G), dtype=np.uint8))
    assert ((0.0 + 1.0) + e) + e == 1.0 and ((0.0 + e) + e) + 1.0 == 1.0 + 2.0 ** -52      # what the table rests on
    want = R.ref_sweeps(ref, tau, pi, eta, counts, 3)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 3), want, "h ascending")
    u = cbind.MT19937(3).uniform(V * G).reshape(V, G)[:, 0]
    assert np.array_equal(cbind.onehot_to_idx(want[0][0])[:, 0], np.floor(u * 4).astype(np.uint8))   # four equal shares, edges 1/4, 1/2, 3/4
    assert ((u > 0.25) & (u < 0.7)).sum() >= 5                        # uniforms that the descending order would send to base 0


# ------------------------------------------------------------------------------------------------------------------- ties
def test_equal_candidates_fall_to_the_order_of_the_edges(ref):
    """Error rows 0 and 1 equal, rows 2 and 3 equal: candidates with the same total bit for bit, p0 == p1 and p2 == p3; which of them a
    uniform picks is the order of the cdf edges alone (sample4, c_sample_tau.c:72-91)"""
    counts, tau, pi, eta = _case(V=40, S=6, G=3, seed=80)
    eta[1] = eta[0]
    eta[3] = eta[2]
    want = R.ref_sweeps(ref, tau, pi, eta, counts, 9)
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, 9), want, "tied candidates")
    _, logp = cbind.sample_tau_u(tau.copy(), pi, eta, counts, cbind.MT19937(9).uniform(40 * 3), want_logp=True)
    assert np.array_equal(logp[..., 0], logp[..., 1]) and np.array_equal(logp[..., 2], logp[..., 3])
    assert len(np.unique(cbind.onehot_to_idx(want[0][0]))) == 4       # every base is drawn somewhere


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_uniform_exactly_on_an_edge_passes_it(ref, seed):
    """sample4 tests `u < edge`: a uniform EQUAL to the first edge belongs to the second candidate.  The first word of the stream is
    known, so the table is built around it (tests/_ref_sweep.py: eta_with_first_edge_at): one read, one haplotype, first edge == u."""
    s = seed
    while not 0.5 < cbind.MT19937(s).uniform(1)[0] < 0.7:             # the construction needs a first uniform in (0.5, 0.7)
        s += 1000
    u = float(cbind.MT19937(s).uniform(1)[0])
    eta = R.eta_with_first_edge_at(u)
    counts = np.zeros((1, 1, 4), dtype=np.int64); counts[0, 0, 0] = 1
    pi = np.ones((1, 1))
    tau = cbind.idx_to_onehot(np.zeros((1, 1), dtype=np.uint8))
    want = R.ref_sweeps(ref, tau, pi, eta, counts, s, n=1)
    assert cbind.onehot_to_idx(want[0][0])[0, 0] == 1 and want[0][1] == 1
    R.assert_same(oracle_sweeps(tau, pi, eta, counts, s, n=1), want, "u on the first edge")
