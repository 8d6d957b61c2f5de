"""The numpy Philox of tests/_philox.py -- the independent side of the Philox-mode chain tests (tests/test_gpu_philox.py) -- against the
C oracle's orc_philox4x32_10 and the Random123 known answers, and the property of Philox those tests lean on: a wrong counter or key
word gives an unrelated stream, so a sweep drawn from it is another sweep.  CPU only."""
import numpy as np
import pytest

from desman_amd.synth import synth_counts, random_state
from oracle import cbind

from _philox import CTR_SEEDS, STREAM_TAUU, philox4x32_10, tau_uniforms, wrong_tau_uniforms


def _oracle(ctr, key):
    ctr, key = np.asarray(ctr).reshape(-1, 4), np.asarray(key).reshape(-1, 2)
    return np.array([cbind.philox4x32_10(c, key[i % len(key)]) for i, c in enumerate(ctr)], dtype=np.uint32)


def test_known_answers():
    """the three Random123 kat_vectors of philox4x32-10 (tests/test_oracle_golden.py has them for the oracle)"""
    kat = [([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        got = philox4x32_10([ctr], key)
        assert got.dtype == np.uint32 and got.shape == (1, 4)
        assert got[0].tolist() == want
        assert cbind.philox4x32_10(ctr, key).tolist() == want
    # all three in one call, a key per counter
    got = philox4x32_10([k[0] for k in kat], [k[1] for k in kat])
    assert got.tolist() == [k[2] for k in kat]


def test_random_counters_and_keys_match_the_oracle():
    rng = np.random.default_rng(20261018)
    n = 10000
    ctr = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64)
    # words with the top bit set in every position, all ones, and zeros, whatever the generator drew
    ctr[:8] = [[0x80000000, 0, 0, 0], [0, 0x80000000, 0, 0], [0, 0, 0x80000000, 0], [0, 0, 0, 0x80000000],
               [0xFFFFFFFF] * 4, [0x80000000] * 4, [0, 0, 0, 0], [0xFFFFFFFF, 0, 0xFFFFFFFF, 0]]
    key[:8] = [[0, 0], [0x80000000, 0], [0, 0x80000000], [0xFFFFFFFF, 0xFFFFFFFF], [0x80000000, 0x80000000], [0, 0], [0xFFFFFFFF, 0], [0, 0xFFFFFFFF]]
    assert (ctr >> 31).any(axis=0).all() and (key >> 31).any(axis=0).all()
    assert np.array_equal(philox4x32_10(ctr, key), _oracle(ctr, key))
    # one key for all counters
    assert np.array_equal(philox4x32_10(ctr[:500], key[3]), _oracle(ctr[:500], key[3]))


@pytest.mark.parametrize("it", [0, 1, 2 ** 31, 2 ** 32 - 1])
@pytest.mark.parametrize("seed", CTR_SEEDS)
def test_tau_uniforms_are_the_scalar_construction(seed, it):
    """tau_uniforms against the construction of tests/test_gpu_edges.py, counter [i, 0, it, 'TAUU'] and key [lo32(seed), hi32(seed)],
    word 0 as u32 / 2^32 -- at iteration counters with the top bit set as well (no sign anywhere)"""
    V, G = 37, 5
    key = [seed & 0xFFFFFFFF, seed >> 32]
    want = np.array([cbind.philox4x32_10([i, 0, it, 0x54415555], key)[0] for i in range(V * G)], dtype=np.float64) / 2 ** 32
    got = tau_uniforms(seed, it, V, G)
    assert got.dtype == np.float64 and got.shape == (V * G,)
    assert np.array_equal(got, want)
    assert (got >= 0.0).all() and (got < 1.0).all()
    assert STREAM_TAUU == int.from_bytes(b"TAUU", "big")
    # a shard's uniforms are the slice of the whole table's: keyed by the global position
    assert np.array_equal(tau_uniforms(seed, it, V - 11, G, v_off=11), want[11 * G:])


@pytest.mark.parametrize("seed", CTR_SEEDS)
def test_a_wrong_counter_or_key_word_is_another_stream_and_another_sweep(seed):
    """What makes the chain tests able to fail: the streams of the three mistakes (counter one ahead, high key word dropped, key words
    swapped) differ from the right one in > 99 % of their words (equal words have probability 2^-32 each), and an oracle sweep drawn from
    any of them ends on other haplotypes.  The key 777 has no high word: dropping it is no mistake there, which is why the chain
    tests run the other keys too."""
    V, S, G = 400, 16, 5
    counts, _, _ = synth_counts(V, S, G, seed=60)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=61)
    # with tens of reads in every sample nearly every step's conditional is all but certain and the sweep hardly depends on its
    # uniforms: the same haplotypes from either stream (which is why the chain tests plant positions without reads)
    same = tau0.copy()
    cbind.sample_tau_u(same, gamma0, eta0, counts, tau_uniforms(seed, 0, V, G))
    other = tau0.copy()
    cbind.sample_tau_u(other, gamma0, eta0, counts, tau_uniforms(seed, 1, V, G))
    assert (cbind.onehot_to_idx(same) != cbind.onehot_to_idx(other)).mean() < 0.01
    counts[3::4] = 0                                              # a position without reads: uniform conditionals, the uniform alone decides
    names = set()
    for it in (0, 1, 2 ** 31):
        right = tau_uniforms(seed, it, V, G)
        ref = tau0.copy()
        cbind.sample_tau_u(ref, gamma0, eta0, counts, right)
        for name, u in wrong_tau_uniforms(seed, it, V, G).items():
            names.add(name)
            assert (u != right).mean() > 0.99, (name, it)
            other = tau0.copy()
            cbind.sample_tau_u(other, gamma0, eta0, counts, u)
            # 100 positions x 5 haplotypes drawn from the uniform alone, each another base with probability 3/4
            assert (cbind.onehot_to_idx(other) != cbind.onehot_to_idx(ref))[3::4].mean() > 0.6, (name, it)
    assert names == ({"it + 1", "high key word dropped", "key words swapped"} if seed >> 32 else {"it + 1", "key words swapped"})
    assert len(wrong_tau_uniforms(CTR_SEEDS[0], 0, V, G)) == 3        # the first key tells all three mistakes
