"""The parts of Brax's training_step around the loss, as include/pupper_hip.h states them (above
pp3_learner_normalizer_update), in numpy.  TEST INFRASTRUCTURE: the checker of csrc/pp3_learn.hip's
normaliser update and gradient clip and of rng.permutation, not a host path of the product
(tests/test_ppo_train_ref.py pins it against the textbook mean and variance)."""
import numpy as np

from pupperv3_mjx import rng

STD_MIN, STD_MAX = 1e-6, 1e6  # brax's defaults


def normalizer_update(obs, count_new, mean, summed_variance, std_min=STD_MIN, std_max=STD_MAX, dtype=np.float64):
    """One running_statistics.update in `dtype` (every operation rounded to it), two passes:
    -> (mean', summed_variance', std').  obs [rows, D]; count_new = the old count + rows."""
    x, mean, sv = (np.asarray(a, dtype=dtype) for a in (obs, mean, summed_variance))
    c = dtype(count_new)
    d_old = x - mean
    mean2 = mean + d_old.sum(axis=0, dtype=dtype) / c
    sv2 = sv + (d_old * (x - mean2)).sum(axis=0, dtype=dtype)
    std2 = np.clip(np.sqrt(np.maximum(sv2, dtype(0)) / c), dtype(std_min), dtype(std_max))
    assert mean2.dtype == dtype and sv2.dtype == dtype and std2.dtype == dtype
    return mean2, sv2, std2


def initial_state(D, dtype=np.float64):
    """Brax's initial running statistics: (count, mean, summed_variance, std)."""
    return 0, np.zeros(D, dtype), np.zeros(D, dtype), np.ones(D, dtype)


def clip_by_global_norm(grads, max_norm):
    """optax.clip_by_global_norm in f64 on a list of arrays: -> (norm, clipped list)."""
    g = [np.asarray(a, dtype=np.float64) for a in grads]
    norm = float(np.sqrt(sum(float((a * a).sum()) for a in g)))
    if norm < max_norm:
        return norm, g
    return norm, [(a / norm) * max_norm for a in g]


def permutation(key, n, partitionable=True):
    """jax.random.permutation(key, n) written out: _shuffle's rounds of split / random bits / stable sort."""
    x = np.arange(n, dtype=np.int32)
    rounds = 0
    while (2 ** 32 - 1) ** rounds < max(1, n) ** 3:  # the smallest r with r ln(2^32 - 1) >= 3 ln n, in integers
        rounds += 1
    key = np.asarray(key, dtype=np.uint32)
    for _ in range(rounds):
        pair = rng.split(key, 2, partitionable)
        key, sub = pair[0], pair[1]
        bits = rng.random_bits32(sub, n, partitionable)
        x = x[np.argsort(bits, kind="stable")]
    return x, rounds
