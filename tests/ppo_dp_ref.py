"""The learner's cross-rank reduction contract (include/pupper_hip.h, "PPO learner across ranks") in
numpy.  TEST INFRASTRUCTURE: the checker of pp3_learner_reduce_gathered / pp3_learner_allreduce_grads
and pp3_learner_normalizer_update_ranks, not a host path of the product (tests/test_ppo_dp_ref.py pins
it against the one-GPU restatement of tests/ppo_train_ref.py)."""
import numpy as np

from ppo_train_ref import STD_MAX, STD_MIN

F = np.float32


def reduce_ranks(arrays):
    """pmean as the contract states it: element-wise (((a_0 + a_1) + a_2) + ..) / world in f32, every
    addition and the quotient rounded to f32 on its own; one rank: the array itself."""
    arrays = [np.asarray(a, dtype=F) for a in arrays]
    s = arrays[0].copy()
    for a in arrays[1:]:
        s = (s + a).astype(F)
    if len(arrays) > 1:
        s = (s / F(len(arrays))).astype(F)
    assert s.dtype == F
    return s


def normalizer_update_ranks(obs_list, count_new, mean, summed_variance, dtype=np.float64, std_min=STD_MIN,
                            std_max=STD_MAX):
    """One running_statistics.update across ranks in `dtype` (every operation rounded to it):
    obs_list[r] [rows_r, D] are rank r's rows, count_new = the old count + sum_r rows_r.
    -> (mean', summed_variance', std')."""
    mean, sv = (np.asarray(a, dtype=dtype) for a in (mean, summed_variance))
    xs = [np.asarray(x, dtype=dtype) for x in obs_list]
    c = dtype(count_new)
    t = None
    for x in xs:
        term = (x - mean).sum(axis=0, dtype=dtype) / c
        t = term if t is None else t + term
    mean2 = mean + t
    v = None
    for x in xs:
        term = ((x - mean) * (x - mean2)).sum(axis=0, dtype=dtype)
        v = term if v is None else v + term
    sv2 = sv + v
    std2 = np.clip(np.sqrt(np.maximum(sv2, dtype(0)) / c), dtype(std_min), dtype(std_max))
    assert mean2.dtype == dtype and sv2.dtype == dtype and std2.dtype == dtype
    return mean2, sv2, std2
