"""Every instantiation of the NMFT update kernels (desman_amd/csrc/kernels_nmft.hip) against the C oracle, at the smallest shapes
that reach it: nmft_mfma_kernel / nmft_mfma_fix_kernel<NT,KB> and their batched twins (32 pairs), nmft_persist_kernel with 4 and
with 12 wavefronts (18 + 12), nmft_split_kernel<NT,KB,4> (the 19 that wide_shape admits), the two-pass kernels at more than 16
haplotypes and where the split kernel's LDS refuses, and pass B at the LDS limit (S = 512, G = 26, 27, 32).

The tables and a Python restatement of the dispatch rules are in tests/_nmft_forms.py; every case asserts through
Context.nmft_debug_path (dsm_nmft_debug_path) that the library takes the kernel the case was written for.  A run is factorize /
factorize_tau of 7 updates (odd: the pair buffers end swapped), then factorize_tau of 5 on the same context; per call: update
count = the oracle's, objective trace rtol 1e-9, factors rtol 1e-6 / atol 1e-12, gamma untouched when fixed, get_tau = arg-max
of the device's own factor, objective rel 1e-9.  The forms of a shape (three-launch loop under every form of the gamma / control
step, persistent loop, batch) agree bit for bit."""
import numpy as np
import pytest

import _nmft_forms as nf
from desman_amd import _lib
from oracle import cbind

pytestmark = pytest.mark.gpu


_CUS = []


def _cus():
    """compute units of device 0, as the library's dispatch rules see them (dsm_nmft_debug_path reports the count it asked with)"""
    if not _CUS:
        c = _lib.Context(0)
        c.set_counts(np.ones((8, 2, 4), dtype=np.int64))
        c.nmft_set(np.full((32, 2), 0.25), np.full((2, 2), 0.5))
        _CUS.append(c.nmft_debug_path()["cus"])
        c.close()
        assert _CUS[0] >= 1
    return _CUS[0]


def _ctx(counts, start, persist=-1, fused=-1):
    c = _lib.Context(0)
    c.set_counts(counts)
    c.set_nmft_persist(persist)
    c.set_nmft_fused(fused)
    c.nmft_set(*start)
    return c


def _state(c, n, tr):
    tau, gam = c.nmft_get()
    return n, np.asarray(tr), tau, gam, c.nmft_get_tau(), c.nmft_objective()


def _two_calls(c, fix, n_first):
    """factorize (fix: factorize_tau) of n_first updates, then factorize_tau of N_UPD_TAU on the same context"""
    first = _state(c, *c.nmft_factorize(n_first, nf.MIN_CHANGE, fix))
    second = _state(c, *c.nmft_factorize(nf.N_UPD_TAU, nf.MIN_CHANGE, True))
    return first, second


def _batch_two_calls(ctxs, fix, n_first):
    res = _lib.Context.batch_nmft_factorize(ctxs, n_first, nf.MIN_CHANGE, fix)
    first = [_state(c, n, tr) for c, (n, tr) in zip(ctxs, res)]
    res = _lib.Context.batch_nmft_factorize(ctxs, nf.N_UPD_TAU, nf.MIN_CHANGE, True)
    return first, [_state(c, n, tr) for c, (n, tr) in zip(ctxs, res)]


def _same_bits(a, b):
    assert a[0] == b[0] and a[5] == b[5]
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x, y)


def _check_call(got, ref, F, V, S, G, gam_before, fix, what):
    """one call of the device against the same call of the oracle (ref = oracle_call(...) from the same factors)"""
    n, tr, tau, gam, onehot, div = got
    n_ref, tr_ref, tc, gc, obj_ref = ref
    assert n == n_ref and len(tr) == n + 1
    np.testing.assert_allclose(tr, tr_ref, rtol=1e-9)
    np.testing.assert_allclose(tau, tc, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(gam, gc, rtol=1e-6, atol=1e-12)
    if fix:
        assert np.array_equal(gam, gam_before)
    assert np.array_equal(onehot, cbind.idx_to_onehot(cbind.nmft_get_tau(tau, G)))
    assert div == pytest.approx(obj_ref, rel=1e-9)


def _check_two_calls(run, ref_first, F, V, S, G, gam0, fix, what):
    first, second = run
    _check_call(first, ref_first, F, V, S, G, gam0, fix, what + " call 1")
    # the second call starts from the device's own factors: so does the oracle's
    ref_second = nf.oracle_call(F, first[2], first[3], True, nf.N_UPD_TAU)
    _check_call(second, ref_second, F, V, S, G, first[3], True, what + " call 2")


def _assert_path(c, V, S, G, fix, cus, persist=True, **more):
    got = c.nmft_debug_path(fix)
    want = dict(nf.expected_path(V, S, G, fix, cus, persist), **more)
    assert {k: got[k] for k in want} == want, (got, want)
    return got


# ---------------------------------------------------------------- mfma, and the persistent loop's four-wavefront form
@pytest.mark.parametrize("nt,kb,S,G", nf.MFMA_CASES, ids=nf.MFMA_IDS)
def test_mfma_every_instantiation(nt, kb, S, G):
    V, cus = nf.V_MFMA, _cus()
    counts, F, starts, refs = nf.case_data(V, S, G, K=2)
    for fix in (False, True):
        runs = {}
        for fused in (0, 1, 3):                             # the three-launch loop under every form of the gamma / control step
            c = _ctx(counts, starts[0], persist=0, fused=fused)
            # (13 workgroup partials: the update kernel's own step only where it is asked for)
            _assert_path(c, V, S, G, fix, cus, persist=False, family="mfma", NT=nt, KB=kb, gstep=(fused == 3 and not fix))
            runs[fused] = _two_calls(c, fix, nf.N_UPD)
            c.close()
        _check_two_calls(runs[0], refs[0][fix], F, V, S, G, starts[0][1], fix, "three-launch fix=%d" % fix)
        for fused in (1, 3):
            _same_bits(runs[fused][0], runs[0][0]); _same_bits(runs[fused][1], runs[0][1])
        # the default call: the persistent loop where the gate says so
        c = _ctx(counts, starts[0])
        want_persist = kb <= 3 and (nt <= 4 or (nt <= 6 and fix))
        p = _assert_path(c, V, S, G, fix, cus)
        assert p["family"] == ("persist" if want_persist else "mfma") and (p["NWV"] == 4) == want_persist
        assert c.nmft_debug_path(True)["family"] == ("persist" if kb <= 3 and nt <= 6 else "mfma")      # (the second call)
        dflt = _two_calls(c, fix, nf.N_UPD)
        c.close()
        _same_bits(dflt[0], runs[0][0]); _same_bits(dflt[1], runs[0][1])
        # a batch of two chains with different starts: each ends where its own single run does
        ctxs = [_ctx(counts, st) for st in starts]
        b_first, b_second = _batch_two_calls(ctxs, fix, nf.N_UPD)
        for c in ctxs:
            c.close()
        _same_bits(b_first[0], runs[0][0]); _same_bits(b_second[0], runs[0][1])
        c = _ctx(counts, starts[1], persist=0, fused=0)
        single1 = _two_calls(c, fix, nf.N_UPD)
        c.close()
        _same_bits(b_first[1], single1[0]); _same_bits(b_second[1], single1[1])
        _check_call(single1[0], refs[1][fix], F, V, S, G, starts[1][1], fix, "chain 1 fix=%d" % fix)


# ---------------------------------------------------------------- the persistent loop, twelve wavefronts
@pytest.mark.parametrize("nt,kb,S,G", nf.P12_CASES, ids=nf.P12_IDS)
def test_persistent_twelve_wavefronts(nt, kb, S, G):
    cus = _cus()
    V = nf.v_p12(cus)                                       # one quad more than the four-wavefront form holds on this device
    counts, F, starts, refs = nf.case_data(V, S, G, K=1, n_first=nf.N_UPD_P12)
    for fix in (False, True):
        c = _ctx(counts, starts[0])
        p = _assert_path(c, V, S, G, fix, cus, family="persist", NT=nt, KB=kb, NWV=nf.P_WAVES)
        assert p["grid"] == nf.ceil_div(nf.ceil_div(V, 4), nf.P_WAVES) <= cus
        pers = _two_calls(c, fix, nf.N_UPD_P12)
        c.close()
        c = _ctx(counts, starts[0], persist=0)
        # (cus + 1 > 128 workgroup partials: with gamma updating the default is the update kernel's own gamma / control step)
        _assert_path(c, V, S, G, fix, cus, persist=False, family="mfma", NT=nt, KB=kb, gstep=not fix)
        loop = _two_calls(c, fix, nf.N_UPD_P12)
        c.close()
        _same_bits(pers[0], loop[0]); _same_bits(pers[1], loop[1])
        _check_two_calls(pers, refs[0][fix], F, V, S, G, starts[0][1], fix, "persistent fix=%d" % fix)


# ---------------------------------------------------------------- split
def test_split_refusals_take_the_two_pass_kernels():
    """385..512 samples with 13..16 haplotypes: wide_shape refuses for LDS (two padded gamma matrices) -- asserted through the query;
    test_two_pass_every_class runs these shapes"""
    cus = _cus()
    assert len(nf.SPLIT_REFUSED) == 4
    for _, _, S, G in nf.SPLIT_REFUSED:
        counts, F, starts, _ = nf.case_data(nf.V_SPLIT, S, G, K=1, n_first=1)
        c = _ctx(counts, starts[0])
        for fix in (False, True):
            _assert_path(c, nf.V_SPLIT, S, G, fix, cus, family="two-pass")
        c.close()


@pytest.mark.parametrize("nt,kb,S,G", nf.SPLIT_CASES, ids=nf.SPLIT_IDS)
def test_split_every_instantiation(nt, kb, S, G):
    V, cus = nf.V_SPLIT, _cus()
    counts, F, starts, refs = nf.case_data(V, S, G, K=2)
    for fix in (False, True):
        singles = []
        for k in range(2):
            c = _ctx(counts, starts[k])
            # two exchange buffers in every instantiation wide_shape admits (tests/test_nmft_forms_cpu.py)
            _assert_path(c, V, S, G, fix, cus, family="split", NT=nt, KB=kb, NCB=4, xpar=True, gstep=False)
            singles.append(_two_calls(c, fix, nf.N_UPD))
            c.close()
        ctxs = [_ctx(counts, st) for st in starts]
        b_first, b_second = _batch_two_calls(ctxs, fix, nf.N_UPD)
        for c in ctxs:
            c.close()
        for k in range(2):
            _same_bits(b_first[k], singles[k][0]); _same_bits(b_second[k], singles[k][1])
        _check_two_calls(singles[0], refs[0][fix], F, V, S, G, starts[0][1], fix, "split fix=%d" % fix)
        _check_call(singles[1][0], refs[1][fix], F, V, S, G, starts[1][1], fix, "chain 1 fix=%d" % fix)


# ---------------------------------------------------------------- two-pass
def _two_pass_case(S, G):
    V, cus = nf.V_TWO, _cus()
    counts, F, starts, refs = nf.case_data(V, S, G, K=2)
    spad, gm = nf.pass_a_form(S, G)
    for fix in (False, True):
        ctxs = [_ctx(counts, st) for st in starts]
        for c in ctxs:
            _assert_path(c, V, S, G, fix, cus, family="two-pass", NT=spad, KB=gm, VT=nf.pass_b_tile(V, S, G)[0])
        # no batch on these shapes -- and the contexts work one by one afterwards
        with pytest.raises(_lib.DesmanHipError, match="do not apply to this shape"):     # DSM_ERR_UNSUPPORTED's message
            _lib.Context.batch_nmft_factorize(ctxs, nf.N_UPD, nf.MIN_CHANGE, fix)
        runs = [_two_calls(c, fix, nf.N_UPD) for c in ctxs]
        for c in ctxs:
            c.close()
        _check_two_calls(runs[0], refs[0][fix], F, V, S, G, starts[0][1], fix, "two-pass fix=%d" % fix)
        _check_call(runs[1][0], refs[1][fix], F, V, S, G, starts[1][1], fix, "chain 1 fix=%d" % fix)


@pytest.mark.parametrize("S,G", nf.TWO_CASES, ids=nf.TWO_IDS)
def test_two_pass_every_class(S, G):
    _two_pass_case(S, G)


@pytest.mark.parametrize("S,G", nf.TWO_LDS_CASES, ids=nf.TWO_LDS_IDS)
def test_two_pass_at_the_lds_limit_of_pass_b(S, G):
    """S = 512: 26 haplotypes fill the 160 KB at the three variants per step the sample count asks for (161 152 B); from 27 on
    (165 456 B) the launcher lowers the variants per step -- two, then one from 31 on -- instead of refusing the shape, up to
    both documented limits at once (S = 512, G = 32: 150 048 B)"""
    vt, lds = nf.pass_b_tile_unlowered(S, G)
    assert vt == 3 and (lds <= nf.LDS_MAX) == (G <= nf.G_FIT_512)
    _two_pass_case(S, G)


def test_debug_path_needs_nmft_set_and_honours_the_switches():
    from desman_amd.synth import synth_counts
    from oracle import ref_numpy as rn
    cus = _cus()
    V, S, G = 203, 33, 5
    counts, _, _ = synth_counts(V, S, G, seed=3)
    c = _lib.Context(0)
    c.set_counts(counts)
    with pytest.raises(_lib.DesmanHipError):
        c.nmft_debug_path()
    c.nmft_set(*rn.nmft_random_initialize(np.random.RandomState(4), V, S, G))
    assert c.nmft_debug_path()["family"] == "persist" and c.nmft_debug_path()["NWV"] == 4
    c.set_nmft_persist(0)
    assert _assert_path(c, V, S, G, False, cus, persist=False)["gstep"] is False
    c.set_nmft_fused(3)
    assert c.nmft_debug_path(False)["gstep"] is True and c.nmft_debug_path(True)["gstep"] is False
    c.set_timing(True)                                       # per-launch events: never the persistent loop
    c.set_nmft_persist(1)
    assert c.nmft_debug_path()["family"] == "mfma"
    c.close()
