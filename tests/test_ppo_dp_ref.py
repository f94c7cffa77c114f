"""tests/ppo_dp_ref.py, the numpy statement of the learner's cross-rank reduction contract, against
what it restates: the one-GPU normaliser update on the concatenated rows, and the order of the
rank sum."""
import numpy as np
import pytest

import ppo_dp_ref as DP
import ppo_train_ref as T

F = np.float32


def _err(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("shards", [(5,), (12, 12), (16, 16, 8), (1, 40, 3, 7)])
@pytest.mark.parametrize("chained", [False, True])
def test_ranks_formula_is_the_update_on_the_concatenated_rows_in_f64(shards, chained):
    """In f64 the two differ by the association of sums of at most 51 terms and by dividing each
    rank's sum where the one-GPU form divides the total: a few roundings of 2^-53 each, relative to the
    largest term.  The columns are offset (|mean| up to 2) and spread (std 0.1 .. 3), so no result is a
    cancelled remainder, and 1e-13 of the largest entry leaves two orders of margin over 51 * 2^-53."""
    D = 36
    rs = np.random.RandomState(sum(shards) + chained)
    loc, scale = rs.uniform(-2, 2, size=D), rs.uniform(0.1, 3, size=D)
    xs = [rs.normal(loc=loc, scale=scale, size=(n, D)).astype(F) for n in shards]
    count, mean, sv, _ = T.initial_state(D)
    if chained:
        y = rs.normal(loc=loc, scale=scale, size=(200, D))
        mean, sv, _ = T.normalizer_update(y, 200, mean, sv)
        count = 200
    count += sum(shards)
    want = T.normalizer_update(np.concatenate(xs), count, mean, sv)
    got = DP.normalizer_update_ranks(xs, count, mean, sv)
    for name, a, b in zip(("mean", "summed_variance", "std"), got, want):
        assert _err(a, b) <= 1e-13, (name, _err(a, b))


def test_one_rank_is_the_one_gpu_update_in_f32_bitwise():
    x = np.random.RandomState(0).normal(loc=1.5, size=(37, 36)).astype(F)
    _, mean, sv, _ = T.initial_state(36, F)
    want = T.normalizer_update(x, 37, mean, sv, dtype=F)
    got = DP.normalizer_update_ranks([x], 37, mean, sv, dtype=F)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_reduce_ranks_adds_in_rank_order():
    """f32 columns whose sum depends on the association: 1e8 + 1 rounds to 1e8."""
    cols = np.array([[1e8, 1.0, -1e8],    # rank order: (1e8 + 1) - 1e8 = 0; exact: 1
                     [1e8, -1e8, 1.0],    # rank order: 1
                     [1.0, 1e8, -1e8],    # rank order: 0
                     [3.0, 4.5, -1.5]], F)  # exact: 6
    got = DP.reduce_ranks([cols[:, r] for r in range(3)])
    assert got.dtype == F
    np.testing.assert_array_equal(got, np.array([0.0, 1.0, 0.0, 6.0], F) / F(3))
    exact = cols.astype(np.float64).sum(axis=1) / 3
    assert got[0] != F(exact[0]) and got[2] != F(exact[2])
    right_first = (cols[:, 0] + (cols[:, 1] + cols[:, 2]).astype(F)).astype(F) / F(3)
    assert got[2] != right_first[2]  # 1 + (1e8 - 1e8) = 1


def test_reduce_ranks_of_one_rank_is_the_array_itself():
    a = np.random.RandomState(1).normal(size=100).astype(F)
    a[:3] = [0.0, -0.0, 1e-45]  # signed zero and a denormal keep their bits
    np.testing.assert_array_equal(DP.reduce_ranks([a]).view(np.uint32), a.view(np.uint32))


def test_reduce_ranks_rounds_each_step_to_f32():
    a = [np.array([1.0], F), np.array([2.0 ** -24], F), np.array([2.0 ** -24], F)]
    # (1 + 2^-24) rounds to 1 (ties to even), twice; in f64 the sum is 1 + 2^-23
    np.testing.assert_array_equal(DP.reduce_ranks(a), np.array([1.0], F) / F(3))
