"""CPU companion of tests/test_gpu_nmft_forms.py: the case tables of tests/_nmft_forms.py reach every instantiation the dispatch of
desman_amd/csrc/kernels_nmft.hip has (by the Python restatement of its rules, which the GPU test holds against the library), and
the oracle alone stays finite on every case and runs the requested number of updates."""
import numpy as np
import pytest

import _nmft_forms as nf

CUS = 256                           # any CU count will do here: the GPU test takes the device's


def test_mfma_table_reaches_all_32_instantiations_and_both_edges():
    assert len(nf.MFMA_CASES) == 34 and len(set(c[:2] for c in nf.MFMA_CASES)) == 32
    assert {nf.mfma_shape(S, G) for _, _, S, G in nf.MFMA_CASES} == {(nt, kb) for nt in range(1, 9) for kb in range(1, 5)}
    for nt, kb, S, G in nf.MFMA_CASES:
        assert nf.mfma_shape(S, G) == (nt, kb)
    for nt in range(1, 9):          # every NT: a case with 15 padded columns and one with none
        assert {S for n, _, S, _ in nf.MFMA_CASES if n == nt} == {16 * nt - 15, 16 * nt}
    for kb in range(1, 5):
        assert {G for _, k, _, G in nf.MFMA_CASES if k == kb} - {3} == {4 * kb - 3, 4 * kb}
    assert any(kb == 1 and G == 3 for _, kb, _, G in nf.MFMA_CASES)      # KB = 1 with padded columns and a run of full length
    assert nf.ceil_div(nf.V_MFMA, 4) == 51 and nf.V_MFMA % 4 == 3 and 51 % 4 == 3


def test_persistent_tables_reach_all_18_plus_12_instantiations():
    four, twelve = set(), set()
    for nt, kb, S, G in nf.MFMA_CASES:
        for fix in (False, True):
            p = nf.persist_shape(nf.V_MFMA, S, G, fix, CUS)
            want = kb <= 3 and (nt <= 4 or (nt <= 6 and fix))
            assert (p is not None) == want
            if p:
                assert p[:3] == (nt, kb, 4)
                four.add((nt, kb))
            assert nf.expected_path(nf.V_MFMA, S, G, fix, CUS)["family"] == ("persist" if want else "mfma")
            assert nf.expected_path(nf.V_MFMA, S, G, fix, CUS, persist=False)["family"] == "mfma"
    assert four == {(nt, kb) for nt in range(1, 7) for kb in range(1, 4)} and len(four) == 18
    for cus in (64, 228, 256, 304):
        V = nf.v_p12(cus)
        for nt, kb, S, G in nf.P12_CASES:
            for fix in (False, True):
                p = nf.persist_shape(V, S, G, fix, cus)
                assert p is not None and p[:3] == (nt, kb, nf.P_WAVES) and 2 <= p[3] <= cus and p[4] <= nf.LDS_MAX
                twelve.add((nt, kb))
            assert nf.persist_shape(V - 4, S, G, False, cus)[2] == 4             # one quad fewer: the four-wavefront form
    assert twelve == {(nt, kb) for nt in range(1, 5) for kb in range(1, 4)} and len(twelve) == 12


def test_split_table_reaches_every_instantiation_wide_shape_admits():
    admitted = {(nt, kb) for nt in (3, 4, 5, 6, 8) for kb in range(1, 5) if nf.split_lds(nt, kb, 4, False) <= nf.LDS_MAX}
    assert admitted == {(nt, kb) for nt in (3, 4, 5, 6, 8) for kb in range(1, 5)} - {(8, 4)} and len(admitted) == 19
    got = set()
    for nt, kb, S, G in nf.SPLIT_CASES:
        assert nf.wide_shape(S, G) == (nt, kb, 4) and nf.mfma_shape(S, G) is None
        got.add((nt, kb))
    assert got == admitted
    for nt, kb in admitted:         # both sample edges and both haplotype edges of every instantiation
        assert {S for n, k, S, _ in nf.SPLIT_CASES if (n, k) == (nt, kb)} == {S for n, S in nf.SPLIT_S if n == nt}
        assert {G for n, k, _, G in nf.SPLIT_CASES if (n, k) == (nt, kb)} - {3} == {max(1, 4 * kb - 3), 4 * kb}
    # refused for LDS alone: 385..512 samples with 13..16 haplotypes -- the two-pass list has them
    assert sorted((S, G) for _, _, S, G in nf.SPLIT_REFUSED) == [(385, 13), (385, 16), (512, 13), (512, 16)]
    assert set((S, G) for _, _, S, G in nf.SPLIT_REFUSED) <= set(nf.TWO_CASES)
    assert len(nf.SPLIT_CASES) == 78
    # the exchange buffers: two wherever wide_shape admits the shape.  The one-buffer form of nmft_split_body would serve (8, 4) alone,
    # which needs 166 592 B even so and is refused: no public call reaches it (the GPU test asserts the flag of every case).
    assert {nf.split_xpar(nt, kb, 4) for nt, kb in got} == {True}
    assert [(nt, kb) for nt in (3, 4, 5, 6, 8) for kb in range(1, 5) if not nf.split_xpar(nt, kb, 4)] == [(8, 4)]
    assert nf.split_lds(8, 4, 4, False) == 166592
    assert nf.ceil_div(nf.V_SPLIT, 4) == 12 and nf.V_SPLIT % 4 == 1


def test_two_pass_table_reaches_the_listed_classes():
    forms = {}
    for S, G in nf.TWO_CASES + nf.TWO_LDS_CASES:
        e = nf.expected_path(nf.V_TWO, S, G, False, CUS)
        assert e["family"] == "two-pass" and e["lds"] <= nf.LDS_MAX
        forms.setdefault((e["KB"], e["NT"]), set()).add(e["VT"])
    assert set(forms) == {(32, 32), (32, 64), (32, 128), (32, 256), (16, 256)}      # (GM, SPAD): nmft_pass_a_kernel<32,256> at every SPAD, <16,512> at 256
    assert set.union(*forms.values()) == {1, 2, 3, 5, 6, 8}                             # variants per step of pass B
    assert any(S > 256 for S, G in nf.TWO_CASES if G > 16)                          # SPAD = 256 walked twice
    # the LDS limit at S = 512
    assert nf.G_FIT_512 == 26
    assert [nf.pass_b_tile(nf.V_TWO, 512, G)[0] for G in (26, 27, 30, 31, 32)] == [3, 2, 2, 1, 1]
    assert nf.pass_b_tile_unlowered(512, 27) == (3, 165456) and nf.pass_b_tile(nf.V_TWO, 512, 32)[2] == 150048
    # a shape that fits at the variants per step its sample count asks for keeps them
    for S in range(1, 513):
        for G in range(1, 33):
            vt0, lds0 = nf.pass_b_tile_unlowered(S, G)
            vt, _, lds = nf.pass_b_tile(nf.V_TWO, S, G)
            assert lds <= nf.LDS_MAX and ((vt, lds) == (vt0, lds0) if lds0 <= nf.LDS_MAX else vt < vt0)


def test_pass_a_instantiations_for_up_to_8_haplotypes_are_out_of_reach():
    """every shape with G <= 8 and S <= 512 has a one-pass kernel, so nmft_pass_a_kernel<4,1024> and <8,512> are never launched
    through dsm_nmft_factorize / dsm_nmft_objective"""
    for S in range(1, 513):
        for G in range(1, 9):
            assert nf.mfma_shape(S, G) is not None or nf.wide_shape(S, G) is not None


def _oracle_two_calls(V, S, G, n_first):
    _, F, starts, refs = nf.case_data(V, S, G, K=2, n_first=n_first)
    for (tau0, gam0), ref in zip(starts, refs):
        for fix in (False, True):
            n, tr, tc, gc, _ = ref[fix]
            assert len(tr) == n + 1
            if nf.stops_early(G):
                assert n == 2 and abs(tr[-1] - tr[-2]) <= nf.MIN_CHANGE
            elif not fix:
                assert n == n_first                    # gamma updating: every requested update runs
            else:
                assert 2 <= n <= n_first
            if fix:
                assert np.array_equal(gc, gam0)
            n2, tr2, _, gc2, _ = nf.oracle_call(F, tc, gc, True, nf.N_UPD_TAU)
            assert len(tr2) == n2 + 1 and np.array_equal(gc2, gc)
            assert n2 == 1 if nf.stops_early(G) else n2 >= 1
            assert min(tr.min(), tr2.min()) > nf.OBJ_FLOOR


@pytest.mark.parametrize("nt,kb,S,G", nf.MFMA_CASES, ids=nf.MFMA_IDS)
def test_oracle_is_finite_on_mfma_cases(nt, kb, S, G):
    _oracle_two_calls(nf.V_MFMA, S, G, nf.N_UPD)


@pytest.mark.parametrize("nt,kb,S,G", nf.P12_CASES, ids=nf.P12_IDS)
def test_oracle_is_finite_on_persist12_cases(nt, kb, S, G):
    _oracle_two_calls(nf.v_p12(CUS), S, G, nf.N_UPD_P12)


@pytest.mark.parametrize("nt,kb,S,G", nf.SPLIT_CASES, ids=nf.SPLIT_IDS)
def test_oracle_is_finite_on_split_cases(nt, kb, S, G):
    _oracle_two_calls(nf.V_SPLIT, S, G, nf.N_UPD)


@pytest.mark.parametrize("S,G", nf.TWO_CASES + nf.TWO_LDS_CASES, ids=nf.TWO_IDS + nf.TWO_LDS_IDS)
def test_oracle_is_finite_on_two_pass_cases(S, G):
    _oracle_two_calls(nf.V_TWO, S, G, nf.N_UPD)
