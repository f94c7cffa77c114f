"""tests/ppo_metrics_ref.py (the f32 restatement of the PPO metrics kernels) against a plain float64
walk of Brax's EpisodeWrapper lines, against ppo_eval_ref.reduce on one shard, and the rank sum's
order."""
import numpy as np
import pytest

import ppo_eval_ref as R
import ppo_metrics_ref as M
from pupperv3_mjx import _abi, _lib

F, U = np.float32, np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _rows(seed, K, n, p_done=0.3):
    rs = np.random.RandomState(seed)
    reward = (rs.normal(size=(K, n)) * 10.0 ** rs.randint(-2, 3, size=(K, n))).astype(F)
    done = (rs.uniform(size=(K, n)) < p_done).astype(F)
    trunc = (done * (rs.uniform(size=(K, n)) < 0.5)).astype(F)
    carry = np.stack([rs.normal(size=n) * 3, rs.randint(0, 40, size=n) * 3.0, rs.uniform(size=n) < 0.3]).astype(F)
    return carry, reward, done, trunc


def _wrapper_walk(carry, reward, done, trunc, action_repeat):
    """EpisodeWrapper.step in float64, env by env: episode_metrics *= (1 - prev_done) after adding the
    step's reward and action_repeat; the finished episodes' records are read at the done steps."""
    K, n = reward.shape
    cnt, sret, slen, strunc, mags = 0, 0.0, 0.0, 0.0, 0.0
    ends = np.zeros(n, int)
    for i in range(n):
        ret, ln, pd = (float(c) for c in carry[:, i])
        for t in range(K):
            ret = (ret + float(reward[t, i])) * (1.0 - pd)
            ln = (ln + action_repeat) * (1.0 - pd)
            if done[t, i]:
                cnt += 1
                ends[i] += 1
                sret += ret
                slen += ln
                strunc += float(trunc[t, i])
                mags += abs(ret)
            mags += abs(float(reward[t, i]))
            pd = float(done[t, i])
    return cnt, sret, slen, strunc, mags, ends


@pytest.mark.parametrize("K, n, ar", [(1, 1, 1), (9, 65, 3), (20, 1500, 1)])
def test_episode_rows_follow_the_episode_wrapper(K, n, ar):
    carry, reward, done, trunc = _rows(100 * K + n, K, n)
    new, part = M.episode_rows(carry, reward, done, trunc, ar)
    out = M.episode_out4(part)
    cnt, sret, slen, strunc, mags, ends = _wrapper_walk(carry, reward, done, trunc, ar)
    assert out[0] == cnt == done.sum() and out[2] == slen and out[3] == strunc == trunc.sum()
    np.testing.assert_array_equal(part[0], ends)
    # f32 summation error: every addition rounds a partial sum below `mags` once (half an ulp, 2^-24
    # relative); a number passes through at most K additions of its env's return, K of its env's sum,
    # n / 1024 of its lane and the tree's 10
    assert abs(float(out[1]) - sret) <= (2 * K + 10 + n // 1024 + 1) * 2.0 ** -24 * mags
    np.testing.assert_array_equal(new[2], done[-1])
    if n >= 65:
        assert (ends >= 2).any()
        assert (done[1:] * done[:-1]).any() or K == 1  # consecutive dones: the second contributes ret = 0
    # without truncation rows: the same but the last number
    _, part0 = M.episode_rows(carry, reward, done, None, ar)
    np.testing.assert_array_equal(_bits(part0[:3]), _bits(part[:3]))
    np.testing.assert_array_equal(part0[3], np.zeros(n, F))


def test_a_done_step_restarts_the_record_one_step_late():
    """One env, by hand: rewards 1, 2, 4, 8, 16; done at steps 1 and 2; action_repeat 2."""
    carry = np.array([[0.5], [4.0], [0.0]], F)
    reward = np.array([[1], [2], [4], [8], [16]], F)
    done = np.array([[0], [1], [1], [0], [0]], F)
    new, part = M.episode_rows(carry, reward, done, done * 0, 2)
    # step 1 ends an episode of return 0.5 + 1 + 2 and length 4 + 2 + 2; step 2 (the step after a
    # done) is wiped and done again: an episode of return 0 and length 0; step 3 follows a done too
    # and is wiped; step 4 starts the record: 16 and 2
    np.testing.assert_array_equal(part[:, 0], [2, 3.5, 8, 0])
    np.testing.assert_array_equal(new[:, 0], [16, 2, 0])
    b = M.episode_begin(np.array([[7, 0, 1.5, 9]], F), [1.0], _abi.EP_SUM_REWARD, _abi.EP_LENGTH)
    np.testing.assert_array_equal(b[:, 0], [1.5, 9, 1])


def test_rank_sum_order_and_identity():
    g = np.array([[1.0, 2.0 ** 24], [2.0 ** -24, 1.0], [2.0 ** -24, 1.0]], F)
    np.testing.assert_array_equal(_bits(M.sum_gathered(g[:1])), _bits(g[0]))
    # ((1 + 2^-24) + 2^-24) = 1 in f32, while 1 + (2^-24 + 2^-24) would be 1 + 2^-23; likewise
    # ((2^24 + 1) + 1) = 2^24 and not 2^24 + 2
    np.testing.assert_array_equal(M.sum_gathered(g), np.array([1.0, 2.0 ** 24], F))
    rs = np.random.RandomState(0)
    x = rs.normal(size=(5, 22)).astype(F)
    want = x[0]
    for r in range(1, 5):
        want = (want + x[r]).astype(F)
    np.testing.assert_array_equal(_bits(M.sum_gathered(x)), _bits(want))


@pytest.mark.parametrize("n", [1, 10, 1025, 2500])
def test_eval_chain_on_one_shard_is_the_reduce(n):
    rs = np.random.RandomState(n)
    acc = (rs.normal(size=(R.WORDS, n)) * 10.0 ** rs.randint(-2, 3, size=(R.WORDS, n))).astype(F)
    np.testing.assert_array_equal(_bits(M.eval_chain([acc])), _bits(R.reduce(acc)))
    s = M.column_sums(acc)
    assert s[21] == n and s[20] == R.lane_tree_sum(acc[R.STEPS])


def test_eval_chain_over_ragged_shards_weighs_every_env_equally():
    rs = np.random.RandomState(5)
    acc = rs.normal(size=(R.WORDS, 10)).astype(F)
    out = M.eval_chain([acc[:, :4], acc[:, 4:8], acc[:, 8:]])
    whole = acc[:R.NCOL].astype(np.float64)
    np.testing.assert_allclose(out[:R.NCOL], whole.mean(1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(out[R.NOUT:R.NOUT + R.NCOL], whole.std(1), rtol=0, atol=1e-6)
    unweighted = np.mean([acc[19, :4].mean(), acc[19, 4:8].mean(), acc[19, 8:].mean()])
    assert abs(out[19] - unweighted) > 1e-3  # not the mean of the shard means


def test_the_library_binds_the_metrics_entry_points():
    L = _lib.load()
    for name in ("pp3_sum_gathered_f32", "pp3_eval_column_sums", "pp3_eval_finish", "pp3_episode_stats_begin",
                 "pp3_episode_stats_rows"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    # argument errors come before any HIP call: they hold without a GPU
    assert L.pp3_sum_gathered_f32(0, None, 1, 4, None, None) == _abi.ERR_ARG
    assert b"pp3_sum_gathered_f32" in L.pp3_ppo_last_error()
    assert L.pp3_episode_stats_rows(0, 1, 1, 1, None, None, None, 1, None, None, None, None) == _abi.ERR_ARG
