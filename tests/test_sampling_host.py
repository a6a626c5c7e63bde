"""Host checks of the draw-level sampling reference (oracle.sampling: splitmix64, seed_for_uniform, HeadRef, beam_reference) that
the GPU sampling tests pin the device head to.  No GPU."""
import numpy as np
import pytest
import torch

import oracle.sampling as osamp

SETTINGS = [(0.1, 0.7, 0), (0.1, 0.7, 50), (0.7, 0.9, 0), (1.0, 0.9, 50), (1.0, 1.0, 0), (2.0, 1.0, 1), (2.0, 0.7, 50),
            (1.0, 0.9, 96)]


def test_splitmix64_inverse_round_trips():
    rng = np.random.default_rng(0)
    words = [int(w) for w in rng.integers(0, 2 ** 63, 2000, dtype=np.int64)] + [0, 1, osamp.M64, 1 << 63]
    for w in words:
        assert osamp.splitmix64_inv(osamp.splitmix64(w)) == w
        assert osamp.splitmix64(osamp.splitmix64_inv(w)) == w
    assert osamp.splitmix64(0) == 0xE220A8397B1DCDAF                  # the published first output of splitmix64 seeded with 0


def test_seed_for_uniform_aims_the_draw():
    for row in (0, 1, 63, 127):
        for step in (0, 1, 7, 1000):
            for k in (0, 1, 7, 12345, (1 << 23) + 5, (1 << 24) - 8, (1 << 24) - 1):
                seed = osamp.seed_for_uniform(k, row, step)
                got, u = osamp.draw_uniform(seed, row, step)
                assert got == k and u == k / 2 ** 24
                if row != 0:                                         # the same seed aims no other row
                    assert osamp.draw_uniform(seed, 0, step)[0] != k or k == 0


def _rows(V, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, V, generator=g) * 2.0).numpy().astype(np.float32)


@pytest.mark.parametrize("temperature,top_p,top_k", SETTINGS)
def test_draw_reference_frequencies_match_distribution(temperature, top_p, top_k):
    """Over an even grid of N uniforms the fp64 CDF-inversion picks each token with the probability of
    oracle.sampling_distribution (HF's warpers), to within 1 / N: the draw rule and the kept set are HF's."""
    V, N = 96, 4096
    u = (np.arange(N) + 0.5) / N
    for row in _rows(V, 4, 11):
        ref = osamp.HeadRef(row, temperature, top_p, top_k)
        assert not ref.tie_cut
        pick, decisive, lo, hi = ref.draw(u)
        freq = np.bincount(pick, minlength=V) / N
        want = osamp.sampling_distribution(torch.from_numpy(row)[None].double(), temperature, top_p, top_k)[0].numpy()
        assert np.all((want > 0) == ref.kept) and ref.undecided == 0
        assert np.abs(freq - want).max() <= 1.0 / N + 1e-12, (temperature, top_p, top_k)
        assert decisive.mean() > 0.99
        assert np.all((lo <= pick) & (pick <= hi))


def test_draw_reference_edges():
    """The first and last grid points pick the first and last kept token in index order; a flat row at top_p 1 is exact
    (margin 0) and its draw is floor(u V); the nucleus cut inside a tie makes a row non-decisive; -inf entries are never kept."""
    V = 1001
    row = _rows(V, 1, 3)[0]
    ref = osamp.HeadRef(row, 0.1, 0.7, 50)
    kept = np.nonzero(ref.kept)[0]
    pick, decisive, _, _ = ref.draw(np.array([0.0, 7 / 2 ** 24, 1 - 1 / 2 ** 24]))
    assert pick[0] == pick[1] == kept[0] and pick[2] == kept[-1] and decisive.all()
    flat = osamp.HeadRef(np.zeros(V, np.float32), 0.7, 1.0, 0)
    assert flat.g_draw == 0.0 and flat.kept.all()
    u = (np.arange(0, 2 ** 24, 4099) + 0.0) / 2 ** 24
    pick, decisive, _, _ = flat.draw(u)
    assert np.array_equal(pick, np.floor(u * V).astype(int))
    assert decisive.mean() > 0.99
    assert osamp.HeadRef(np.zeros(V, np.float32), 1.0, 0.9, 0).tie_cut
    neg = row.copy()
    neg[::3] = -np.inf
    r = osamp.HeadRef(neg, 1.0, 1.0, 0)
    assert not r.maybe[::3].any() and r.kept[1::3].all()


def test_beam_reference_returns_distinct_kept_ids():
    V, K = 96, 2
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(K, V, generator=g) * 2.0).numpy()
    for t, p, k in ((1.0, 0.9, 0), (0.1, 0.7, 50), (1.5, 1.0, 6)):
        M = 2 * K
        kept = [osamp.HeadRef(logits[b], t, p, k, min_keep=M // K).maybe for b in range(K)]
        for step in range(20):
            ids, _ = osamp.beam_reference(logits, np.array([0.0, -0.7]), t, p, k, M, 5, step, 0)
            assert len(set(ids.tolist())) == M
            assert all(kept[i // V][i % V] for i in ids.tolist())
    u = osamp.beam_uniforms(5, 3, 1, V)
    assert u.dtype == np.float32 and float(u.min()) > 0 and float(u.max()) < 1
