"""numpy f32 restatement of the PPO metrics kernels (include/pupper_hip.h, "PPO metrics"): the training
episode statistics of a collected batch, the rank-ordered sum of gathered vectors and the evaluation
reduce cut for a sum over ranks.  Every product, sum and difference is rounded to f32 on its own, in
the header's order; the one-workgroup sums are ppo_eval_ref.lane_tree_sum."""
import numpy as np

import ppo_eval_ref as R

f32 = np.float32


def episode_begin(episode, done, sum_word, length_word):
    """carry [3][n] = (ret, len, pd) from the env's episode record [n][stride] and done [n]."""
    episode = np.asarray(episode, f32)
    return np.stack([episode[:, sum_word], episode[:, length_word], np.asarray(done, f32).reshape(-1)]).astype(f32)


def episode_rows(carry, reward, done, truncation, action_repeat):
    """The row chain: carry [3][n], reward / done / truncation [K][n] (truncation None: zeros)
    -> (the carry after the rows, part [4][n] = per-env episodes, returns, lengths, truncated)."""
    ret, ln, pd = (np.array(c, f32) for c in np.asarray(carry, f32))
    n = ret.shape[0]
    cnt, sret, slen, strunc = (np.zeros(n, f32) for _ in range(4))
    rep = f32(action_repeat)
    for t in range(len(reward)):
        r, d = np.asarray(reward[t], f32), np.asarray(done[t], f32)
        tr = np.zeros(n, f32) if truncation is None else np.asarray(truncation[t], f32)
        keep = (f32(1) - pd).astype(f32)
        ret = ((ret + r).astype(f32) * keep).astype(f32)
        ln = ((ln + rep).astype(f32) * keep).astype(f32)
        hit = d != 0
        cnt = np.where(hit, (cnt + f32(1)).astype(f32), cnt)
        sret = np.where(hit, (sret + ret).astype(f32), sret)
        slen = np.where(hit, (slen + ln).astype(f32), slen)
        strunc = np.where(hit, (strunc + tr).astype(f32), strunc)
        pd = d.copy()
    return np.stack([ret, ln, pd]).astype(f32), np.stack([cnt, sret, slen, strunc]).astype(f32)


def episode_out4(part):
    """(episodes, sum of returns, sum of lengths, truncated episodes): each row of part summed over the envs."""
    return np.array([R.lane_tree_sum(row) for row in np.asarray(part, f32)], f32)


def sum_gathered(gathered):
    """[world][count] -> [count]: ((g_0 + g_1) + g_2) + .., from rank 0's value."""
    g = np.asarray(gathered, f32)
    out = g[0].copy()
    for r in range(1, g.shape[0]):
        out = (out + g[r]).astype(f32)
    return out


def _column(acc, k):
    return np.asarray(acc, f32)[k if k < R.NCOL else R.STEPS]


def column_sums(acc, mean21=None):
    """One shard's 22: the sums of the 21 reduced columns (mean21: of their squared deviations), then n."""
    out = np.zeros(R.NOUT + 1, f32)
    for k in range(R.NOUT):
        col = _column(acc, k)
        if mean21 is not None:
            d = (col - f32(mean21[k])).astype(f32)
            col = (d * d).astype(f32)
        out[k] = R.lane_tree_sum(col)
    out[R.NOUT] = f32(np.asarray(acc).shape[1])
    return out


def finish(sums22, which, out42):
    """which 0: the means into out42[:21]; which 1: the stds into out42[21:]; -> a new out42."""
    out = np.array(out42, f32)
    s = np.asarray(sums22, f32)
    q = (s[:R.NOUT] / s[R.NOUT]).astype(f32)
    if which == 0:
        out[:R.NOUT] = q
    else:
        out[R.NOUT:] = np.sqrt(q).astype(f32)
    return out


def eval_chain(shards):
    """The evaluation reduce over ranks: `shards` = each rank's accumulator [22][n_r], in rank order
    -> f32 [42] (every rank's result)."""
    out = np.zeros(2 * R.NOUT, f32)
    total = sum_gathered(np.stack([column_sums(a) for a in shards]))
    out = finish(total, 0, out)
    total = sum_gathered(np.stack([column_sums(a, out[:R.NOUT]) for a in shards]))
    return finish(total, 1, out)
