"""f32 numpy restatement of pp3_gae's recurrence (include/pupper_hip.h; Brax PPO's compute_gae as
compute_ppo_loss calls it): every *, + and - a separate f32 rounding in the contract's association.
TEST INFRASTRUCTURE: the checker of csrc/pp3_ppo.hip, not a host path of the product."""
import numpy as np

F = np.float32


def gae(reward, done, truncation, values, bootstrap, discount, lam, reward_scaling, intermediates=None):
    """(vs, adv), each f32 [K, ...], from f32 arrays [K, ...] and bootstrap [...].  `intermediates`: a
    list that receives every rounded intermediate array (for the subnormal check of the GPU test)."""
    reward, done, truncation, values = (np.asarray(a, dtype=F) for a in (reward, done, truncation, values))
    bootstrap = np.asarray(bootstrap, dtype=F)
    discount, lam, reward_scaling, one = F(discount), F(lam), F(reward_scaling), F(1.0)
    K = reward.shape[0]
    vs = np.empty_like(values)
    adv = np.empty_like(values)
    keep = intermediates.append if intermediates is not None else (lambda a: None)
    vnext = bootstrap.copy()
    vsnext = bootstrap.copy()
    acc = np.zeros_like(bootstrap)
    for t in range(K - 1, -1, -1):
        v = values[t]
        tm = one - truncation[t]
        term = done[t] * tm
        omt = one - term
        g = discount * omt
        r = reward[t] * reward_scaling
        gv = g * vnext
        s = r + gv
        d0 = s - v
        delta = d0 * tm
        gt = g * tm
        gl = gt * lam
        ga = gl * acc
        acc = delta + ga
        vs[t] = acc + v
        gvs = g * vsnext
        s2 = r + gvs
        d2 = s2 - v
        adv[t] = d2 * tm
        for a in (tm, term, omt, g, r, gv, s, d0, delta, gt, gl, ga, acc, vs[t], gvs, s2, d2, adv[t]):
            assert a.dtype == F
            keep(np.array(a))
        vnext = v
        vsnext = vs[t]
    return vs, adv
