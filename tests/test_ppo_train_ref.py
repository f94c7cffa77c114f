"""rng.permutation against its written-out restatement, and the restated running-statistics update
(tests/ppo_train_ref.py, the checker of the device kernel) against the textbook mean and variance."""
import numpy as np
import pytest

import ppo_train_ref as T
from pupperv3_mjx import rng


@pytest.mark.parametrize("partitionable", [True, False])
@pytest.mark.parametrize("n", [1, 2, 5, 4096])
def test_permutation_equals_the_written_out_shuffle(n, partitionable):
    key = rng.PRNGKey(17 + n)
    got = rng.permutation(key, n, partitionable)
    want, _ = T.permutation(key, n, partitionable)
    assert got.dtype == np.int32 and got.shape == (n,)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.sort(got), np.arange(n))  # a permutation


def test_permutation_differs_between_keys_and_layouts():
    a, b = rng.permutation(rng.PRNGKey(1), 4096), rng.permutation(rng.PRNGKey(2), 4096)
    assert np.mean(a != b) > 0.99
    assert np.mean(a != np.arange(4096)) > 0.99
    assert np.any(rng.permutation(rng.PRNGKey(1), 4096, False) != a)


@pytest.mark.parametrize("n, rounds", [(1, 0), (5, 1), (4096, 2)])
def test_permutation_round_count(monkeypatch, n, rounds):
    calls = []
    split = rng.split
    monkeypatch.setattr(rng, "split", lambda *a, **k: calls.append(1) or split(*a, **k))
    rng.permutation(rng.PRNGKey(3), n)
    assert len(calls) == rounds
    assert T.permutation(rng.PRNGKey(3), n)[1] == rounds


def test_chained_updates_equal_one_update_and_the_textbook_statistics():
    rs = np.random.RandomState(0)
    x = rs.normal(loc=rs.uniform(-2, 2, size=72), scale=rs.uniform(0.1, 3, size=72), size=(3001, 72))
    count, mean, sv, _ = T.initial_state(72)
    whole = T.normalizer_update(x, 3001, mean, sv)
    h = 1234
    m1, s1, _ = T.normalizer_update(x[:h], h, mean, sv)
    halves = T.normalizer_update(x[h:], 3001, m1, s1)
    textbook = (x.mean(axis=0), ((x - x.mean(axis=0)) ** 2).sum(axis=0), x.std(axis=0))
    for name, a, b, c in zip(("mean", "summed_variance", "std"), whole, halves, textbook):
        scale = np.abs(c).max()
        assert np.abs(a - b).max() <= 1e-12 * scale, name
        assert np.abs(a - c).max() <= 1e-12 * scale, name


def test_update_clips_the_std_and_f32_keeps_its_dtype():
    x = np.tile(np.array([[0.5, -1.25, 3.0]]), (64, 1))
    _, mean, sv, _ = T.initial_state(3, np.float32)
    m, s, sd = T.normalizer_update(x, 64, mean, sv, dtype=np.float32)
    np.testing.assert_array_equal(m, x[0].astype(np.float32))
    assert np.all(s == 0) and np.all(sd == np.float32(T.STD_MIN)) and sd.dtype == np.float32
    y = np.random.RandomState(1).normal(size=(500, 3))
    assert np.all(T.normalizer_update(y, 500, mean, sv, std_max=0.5)[2] == 0.5)


def test_clip_by_global_norm():
    g = [np.array([3.0, 0.0]), np.array([[4.0]])]
    norm, same = T.clip_by_global_norm(g, 10.0)
    assert norm == 5.0 and all(np.array_equal(a, b) for a, b in zip(g, same))
    norm, cl = T.clip_by_global_norm(g, 1.0)
    assert norm == 5.0
    np.testing.assert_allclose(np.concatenate([a.ravel() for a in cl]), [0.6, 0.0, 0.8], rtol=1e-15)
