"""The PPO evaluation restatement (tests/ppo_eval_ref.py) against hand-written answers and float64, and
ppo.eval_schedule against worked examples.  No GPU."""
import math

import numpy as np
import pytest

import ppo_eval_ref as R

U = 2.0 ** -24  # f32 unit roundoff


def _metrics(n, scale):
    """metrics [n][19] with column c of env i = scale * (c + 1) * (i + 1): exact in f32 for small scales"""
    return (scale * np.outer(np.arange(1, n + 1), np.arange(1, 20))).astype(np.float32)


def test_known_answers_three_envs_four_steps():
    """env 0 is done at step 1 (and sees done = 0, then 1 again later); env 1 is never done; env 2 is
    done at the last step.  Sums stop after the done step, episode_steps freezes there, active stays 0."""
    reward = np.array([[1, 10, 100], [2, 20, 200], [4, 40, 400], [8, 80, 800]], np.float32)
    done = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 1]], np.float32)
    # the episode counter the env reports: it restarts after env 0's done step
    steps = np.array([[1, 1, 1], [2, 2, 2], [1, 3, 3], [2, 4, 4]], np.float32)
    acc = R.reset(3)
    assert acc.shape == (22, 3) and np.array_equal(acc[R.ACTIVE], [1, 1, 1]) and not acc[:20].any() and not acc[21].any()
    for t in range(4):
        acc = R.accumulate(acc, reward[t], done[t], _metrics(3, 2.0 ** t), steps[t])
    assert np.array_equal(acc[19], [3, 150, 1500])          # reward: env 0 stops after step 1
    assert np.array_equal(acc[R.ACTIVE], [0, 1, 0])         # env 0 stays inactive after a later done = 0
    assert np.array_equal(acc[R.STEPS], [2, 4, 4])          # frozen at the first done
    for c in range(19):                                     # metrics: 1 + 2 (+ 4 + 8) times (c + 1)(i + 1)
        assert np.array_equal(acc[c], [3 * (c + 1), 15 * (c + 1) * 2, 15 * (c + 1) * 3])
    out = R.reduce(acc)
    assert out.shape == (42,) and out.dtype == np.float32
    assert out[19] == np.float32(np.float32(1653) / np.float32(3)) and out[20] == np.float32(np.float32(10) / np.float32(3))
    assert abs(out[21 + 19] - np.std([3.0, 150.0, 1500.0])) < 1e-3


def test_products_and_sums_round_separately():
    """x * active and the running sum are two f32 roundings: 1 + 2^-24 stays 1 (round to even), where
    one rounding of the exact sum of the three terms would not."""
    acc = R.reset(1)
    m = np.zeros((1, 19), np.float32)
    for r in (1.0, 2.0 ** -24, 2.0 ** -24):
        acc = R.accumulate(acc, np.float32([r]), np.float32([0]), m, np.float32([1]))
    assert acc[19, 0] == np.float32(1.0)


@pytest.mark.parametrize("action_repeat", [1, 3])
@pytest.mark.parametrize("step0", [0, 4])
def test_row_chain_equals_the_per_step_restatement(step0, action_repeat):
    rs = np.random.RandomState(7 + step0 + action_repeat)
    n, K = 37, 9
    reward = rs.normal(size=(K, n)).astype(np.float32)
    done = (rs.uniform(size=(K, n)) < 0.2).astype(np.float32)
    # an accumulator that has already seen step0 steps (some envs inactive, some sums non-zero)
    acc0 = R.reset(n)
    if step0:
        acc0[19] = rs.normal(size=n).astype(np.float32)
        acc0[R.ACTIVE] = (rs.uniform(size=n) < 0.7).astype(np.float32)
        acc0[R.STEPS] = np.where(acc0[R.ACTIVE] != 0, step0 * action_repeat, 2 * action_repeat).astype(np.float32)
    rows = R.accumulate_rows(acc0, reward, done, step0, action_repeat)
    per = acc0.copy()
    zeros = np.zeros((n, 19), np.float32)
    for t in range(K):
        # the counter of an env that was reset step0 steps before row 0 and not done since
        per = R.accumulate(per, reward[t], done[t], zeros, np.full(n, (step0 + t + 1) * action_repeat, np.float32))
    for c in (19, R.ACTIVE, R.STEPS):
        assert np.array_equal(rows[c].view(np.uint32), per[c].view(np.uint32)), c
    assert np.array_equal(rows[:19], acc0[:19])  # the row chain leaves the metrics columns alone
    assert (rows[R.ACTIVE] == 0).any() and (rows[R.ACTIVE] == 1).any()


@pytest.mark.parametrize("n", [1, 63, 1025, 4096, 5000])
def test_reduce_against_float64(n):
    """mean: within (ceil(N / 1024) + 10 + 2) u mean|x| of float64, the standard bound of the
    summation order (an element passes through at most L = ceil(N / 1024) lane additions and 10 tree
    levels; one more rounding in the quotient, one unit for the second-order terms), u = 2^-24.

    std, from the same order.  Let m^ be the f32 mean and delta the bound above, so |m^ - m| <= delta.
    d_i = fl(x_i - m^) and fl(d_i d_i) carry three roundings per term; the sum of these non-negative
    terms adds at most (L + 10) u relative, the quotient by N one more: the computed variance is
    V' (1 + theta) with |theta| <= (L + 14) u and V' = mean (x_i - m^)^2 = V + (m^ - m)^2 exactly,
    because the deviations from the true mean sum to zero.  sqrt(V + delta^2) <= sqrt(V) + delta, the
    root halves theta and adds its own rounding, hence
        |std^ - std| <= delta + (std + delta) ((L + 14) / 2 + 1 + 1) u
    with the last unit again covering the second-order terms."""
    rs = np.random.RandomState(n)
    acc = R.reset(n)
    acc[:20] = (rs.normal(size=(20, n)) * np.logspace(-2, 3, 20)[:, None] + rs.normal(size=(20, 1))).astype(np.float32)
    acc[R.STEPS] = rs.randint(1, 1001, size=n).astype(np.float32)
    out = R.reduce(acc)
    L = math.ceil(n / 1024)
    for k in range(21):
        col = acc[k if k < 20 else R.STEPS].astype(np.float64)
        delta = (L + 10 + 2) * U * np.abs(col).mean()
        assert abs(float(out[k]) - col.mean()) <= delta, (k, out[k], col.mean())
        sd = col.std()
        assert abs(float(out[21 + k]) - sd) <= delta + (sd + delta) * ((L + 14) / 2 + 2) * U, (k, out[21 + k], sd)


def test_reduce_order_is_lanes_then_tree():
    """The order matters and is the stated one: element i of lane i % 1024, lanes met pairwise at
    distance 512, 256, ..  With x[0] = 1 and x[1 .. 1024] = u: lane 0 adds x[1024] first, 1 + u -> 1
    (ties to even); the tree's first level adds lane 512's u to it, again -> 1, while every other
    pair doubles exactly, so the later levels add 2 u, 4 u, .. 512 u: 1 + 1022 u, two u short of the
    exact 1 + 1024 u."""
    x = np.full(1025, U, np.float32)
    x[0] = 1.0
    got = R.lane_tree_sum(x)
    assert got == np.float32(1.0 + 1022 * U)
    assert got != np.float32(np.sum(x.astype(np.float64)))


def test_eval_schedule_worked_examples():
    from pupperv3_mjx import ppo
    s = ppo.eval_schedule(1_000_000, 4096, 20, 1, num_evals=1)
    assert (s["steps_per_iteration"], s["num_evals_after_init"], s["iterations_per_epoch"]) == (81920, 1, 13)
    assert not s["eval_before_training"] and s["eval_steps"] == [13 * 81920] and s["total_iterations"] == 13
    s = ppo.eval_schedule(1_000_000, 4096, 20, 1, num_evals=2)
    assert s["num_evals_after_init"] == 1 and s["iterations_per_epoch"] == 13
    assert s["eval_before_training"] and s["eval_steps"] == [0, 1064960]
    s = ppo.eval_schedule(1_000_000, 4096, 20, 1, num_evals=5)  # 1e6 / (4 * 81920) = 3.05 -> 4
    assert s["num_evals_after_init"] == 4 and s["iterations_per_epoch"] == 4 and s["total_iterations"] == 16
    assert s["eval_steps"] == [0, 327680, 655360, 983040, 1310720]
    s = ppo.eval_schedule(70, 6, 3, 1, num_evals=3)  # not a multiple: 70 / (2 * 18) = 1.94 -> 2
    assert s["iterations_per_epoch"] == 2 and s["eval_steps"] == [0, 36, 72]
    s = ppo.eval_schedule(72, 6, 3, 2, num_evals=3)  # action_repeat counts env steps: 36 per iteration
    assert s["steps_per_iteration"] == 36 and s["iterations_per_epoch"] == 1 and s["eval_steps"] == [0, 36, 72]
    with pytest.raises(ValueError):
        ppo.eval_schedule(0, 6, 3)
