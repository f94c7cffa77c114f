"""numpy f32 restatement of the PPO evaluation kernels (include/pupper_hip.h, "PPO evaluation"): every
product and sum is rounded to f32 on its own, in the header's order.  The accumulator is [22][n]:
columns 0 .. 19 episode_metrics (total_dist, the 18 reward terms, reward), 20 active, 21 episode_steps."""
import numpy as np

NCOL, ACTIVE, STEPS, WORDS, NOUT, LANES = 20, 20, 21, 22, 21, 1024
f32 = np.float32


def reset(n):
    acc = np.zeros((WORDS, n), f32)
    acc[ACTIVE] = 1
    return acc


def accumulate(acc, reward, done, metrics, steps):
    """One wrapper step: reward, done, steps [n], metrics [n][>= 19] -> a new accumulator."""
    acc = np.array(acc, f32)
    active = acc[ACTIVE].copy()
    x = np.concatenate([np.asarray(metrics, f32)[:, :NCOL - 1].T, np.asarray(reward, f32)[None]])
    acc[STEPS] = np.where(active != 0, np.asarray(steps, f32), acc[STEPS])
    prod = (x * active[None]).astype(f32)
    acc[:NCOL] = (acc[:NCOL] + prod).astype(f32)
    acc[ACTIVE] = (active * (f32(1) - np.asarray(done, f32))).astype(f32)
    return acc


def accumulate_rows(acc, reward, done, step0, action_repeat):
    """The row chain: reward, done [K][n]; only the reward column, active and episode_steps move."""
    acc = np.array(acc, f32)
    em, active, es = acc[NCOL - 1].copy(), acc[ACTIVE].copy(), acc[STEPS].copy()
    for t in range(len(reward)):
        es = np.where(active != 0, f32((step0 + t + 1) * action_repeat), es).astype(f32)
        em = (em + (np.asarray(reward[t], f32) * active).astype(f32)).astype(f32)
        active = (active * (f32(1) - np.asarray(done[t], f32))).astype(f32)
    acc[NCOL - 1], acc[ACTIVE], acc[STEPS] = em, active, es
    return acc


def lane_tree_sum(x):
    """The one-workgroup sum: lane i adds x[i], x[i + 1024], .. ascending from 0, then the binary tree."""
    x = np.asarray(x, f32)
    lanes = np.zeros(LANES, f32)
    for j in range(0, len(x), LANES):
        row = x[j:j + LANES]
        lanes[:len(row)] = (lanes[:len(row)] + row).astype(f32)
    s = LANES // 2
    while s:
        lanes[:s] = (lanes[:s] + lanes[s:2 * s]).astype(f32)
        s //= 2
    return lanes[0]


def reduce(acc):
    """-> f32 [42]: mean[21], then the population std[21], of the 20 metrics columns and episode_steps."""
    acc = np.asarray(acc, f32)
    n = f32(acc.shape[1])
    out = np.zeros(2 * NOUT, f32)
    for k in range(NOUT):
        col = acc[k if k < NCOL else STEPS]
        mean = f32(lane_tree_sum(col) / n)
        d = (col - mean).astype(f32)
        var = f32(lane_tree_sum((d * d).astype(f32)) / n)
        out[k], out[NOUT + k] = mean, f32(np.sqrt(var))
    return out
