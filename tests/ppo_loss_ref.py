"""The PPO learner's contract (include/pupper_hip.h, above pp3_learner_create) in torch on the CPU,
the dtype a parameter, gradients by autograd; Adam in f32 numpy and the normaliser fold in f64 numpy.
TEST INFRASTRUCTURE: the checker of csrc/pp3_learn.hip, not a host path of the product
(tests/test_ppo_loss_ref.py pins it: finite differences, the GAE part against ppo_ref.gae, the
log-prob against export.normal_tanh_log_prob).

Batch arrays are the minibatch itself: obs_all [K+1, B, D], raw_action / eps [K, B, 12], log_prob /
reward / done / truncation [K, B] (numpy, or torch tensors on any device).  Networks: a list of (kernel [in, out], bias [out]) per layer and
the hidden activation's name; the last layer is linear."""
import math

import numpy as np
import torch

HP = dict(discount=0.97, gae_lambda=0.95, reward_scaling=1.0, clipping_epsilon=0.3, entropy_cost=1e-2,
          normalize_advantage=True, min_std=0.001, var_scale=1.0)
METRICS = ("total_loss", "policy_loss", "v_loss", "entropy_loss")


def activate(z, name):
    if name == "relu":
        return torch.clamp(z, min=0)
    if name == "elu":
        return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0)))
    if name == "tanh":
        return torch.tanh(z)
    if name == "sigmoid":
        return torch.sigmoid(z)
    if name == "linear":
        return z
    raise ValueError(name)


def mlp(x, layers, activation, pre=None):
    """The last layer's output; `pre` (a list) receives every hidden pre-activation."""
    h = x
    for i, (k, b) in enumerate(layers):
        z = h @ k + b
        if i == len(layers) - 1:
            return z
        if pre is not None:
            pre.append(z.detach())
        h = activate(z, activation)


def gae(reward, done, truncation, values, bootstrap, discount, lam, reward_scaling):
    """The pp3_gae recurrence (tests/ppo_ref.gae's association) on tensors of one dtype."""
    K = reward.shape[0]
    vs, adv = [None] * K, [None] * K
    vnext, vsnext, acc = bootstrap, bootstrap, torch.zeros_like(bootstrap)
    for t in range(K - 1, -1, -1):
        v = values[t]
        tm = 1 - truncation[t]
        term = done[t] * tm
        g = discount * (1 - term)
        r = reward[t] * reward_scaling
        delta = ((r + g * vnext) - v) * tm
        acc = delta + (((g * tm) * lam) * acc)
        vs[t] = acc + v
        adv[t] = ((r + g * vsnext) - v) * tm
        vnext, vsnext = v, vs[t]
    return torch.stack(vs), torch.stack(adv)


def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-torch.abs(x)))


def log_prob(logits, raw, min_std, var_scale):
    loc, s = logits[..., :12], logits[..., 12:]
    scale = (softplus(s) + min_std) * var_scale
    zr = (raw - loc) / scale
    terms = (-0.5 * zr * zr - torch.log(scale) - 0.5 * math.log(2 * math.pi)
             - 2.0 * (math.log(2.0) - raw - softplus(-2.0 * raw)))
    return terms.sum(-1)


def as_params(layers, dtype):
    return [(torch.tensor(np.asarray(k), dtype=dtype, requires_grad=True),
             torch.tensor(np.asarray(b), dtype=dtype, requires_grad=True)) for k, b in layers]


def loss(policy, value, activation, batch, dtype=torch.float64, normalizer=None, targets=None, **hp):
    """-> (metrics dict of tensors, aux dict).  policy / value: as_params lists.  `targets` = (vs, adv)
    replaces the GAE (finite differences hold them fixed, as the gradient does)."""
    hp = {**HP, **hp}
    t = lambda a: a.to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype)
    obs = t(batch["obs_all"])
    if normalizer is not None:
        obs = (obs - t(normalizer[0])) / t(normalizer[1])
    pre = []
    values = mlp(obs, value, activation, pre)[..., 0]
    baseline, bootstrap = values[:-1], values[-1]
    if targets is None:
        with torch.no_grad():
            vs, adv = gae(t(batch["reward"]), t(batch["done"]), t(batch["truncation"]), baseline.detach(),
                          bootstrap.detach(), hp["discount"], hp["gae_lambda"], hp["reward_scaling"])
    else:
        vs, adv = (t(a) for a in targets)
    adv_raw = adv
    if hp["normalize_advantage"]:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    logits = mlp(obs[:-1], policy, activation, pre)
    logp = log_prob(logits, t(batch["raw_action"]), hp["min_std"], hp["var_scale"])
    rho = torch.exp(logp - t(batch["log_prob"]))
    eps_c = hp["clipping_epsilon"]
    policy_loss = -torch.minimum(rho * adv, torch.clamp(rho, 1 - eps_c, 1 + eps_c) * adv).mean()
    v_loss = 0.25 * ((vs - baseline) ** 2).mean()
    loc, s = logits[..., :12], logits[..., 12:]
    scale = (softplus(s) + hp["min_std"]) * hp["var_scale"]
    a = loc + scale * t(batch["eps"])
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(scale) + 2.0 * (math.log(2.0) - a - softplus(-2.0 * a))).sum(-1)
    entropy_loss = -hp["entropy_cost"] * ent.mean()
    total = policy_loss + v_loss + entropy_loss
    metrics = dict(total_loss=total, policy_loss=policy_loss, v_loss=v_loss, entropy_loss=entropy_loss)
    aux = dict(vs=vs, adv=adv, adv_raw=adv_raw, rho=rho, logp=logp, logits=logits, pre=pre, baseline=baseline)
    return metrics, aux


def loss_and_grad(policy_layers, value_layers, activation, batch, dtype=torch.float64, normalizer=None, **hp):
    """numpy in, numpy out: (metrics {name: float}, {"policy" | "value": [(dkernel, dbias)]}, aux as numpy)."""
    pol, val = as_params(policy_layers, dtype), as_params(value_layers, dtype)
    metrics, aux = loss(pol, val, activation, batch, dtype, normalizer, **hp)
    flat = [p for kb in pol + val for p in kb]
    grads = torch.autograd.grad(metrics["total_loss"], flat, allow_unused=True)
    grads = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for g, p in zip(grads, flat)]
    pairs = [(grads[2 * i], grads[2 * i + 1]) for i in range(len(pol) + len(val))]
    out_aux = {k: (v.detach().numpy() if k != "pre" else [z.numpy() for z in v]) for k, v in aux.items()}
    return ({k: float(v.detach()) for k, v in metrics.items()}, {"policy": pairs[:len(pol)], "value": pairs[len(pol):]},
            out_aux)


F = np.float32


def adam(p, g, m, v, lr, b1, b2, eps, t):
    """One optax.adam step in f32 numpy, every operation rounded on its own in the header's
    association; c1, c2 as the host passes them.  -> (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    lr, b1, b2, eps = F(lr), F(b1), F(b2), F(eps)
    c1, c2 = F(1.0 - float(b1) ** t), F(1.0 - float(b2) ** t)
    one = F(1.0)
    m2 = b1 * m + (one - b1) * g
    v2 = b2 * v + ((one - b2) * g) * g
    p2 = p - (lr * (m2 / c1)) / (np.sqrt(v2 / c2) + eps)
    assert m2.dtype == F and v2.dtype == F and p2.dtype == F
    return p2, m2, v2


def fold(kernel, bias, mean, std):
    """pp3_policy_load_params' layer 0 in f64: W' = W / std[k], b' = b - sum_k (mean / std)[k] W[k]."""
    kernel, bias, mean, std = (np.asarray(a, dtype=np.float64) for a in (kernel, bias, mean, std))
    return kernel / std[:, None], bias - (mean / std) @ kernel


# ---- test cases: random nets and minibatches, and the conditions a parity case must meet ----
def random_net(rs, in_dim, hidden, out):
    sizes = [in_dim, *hidden, out]
    return [(rs.normal(scale=1 / np.sqrt(sizes[i]), size=(sizes[i], sizes[i + 1])).astype(F),
             rs.normal(scale=0.1, size=sizes[i + 1]).astype(F)) for i in range(len(sizes) - 1)]


def random_case(seed, K, B, in_dim, hidden, activation, with_normalizer, **hp):
    """A minibatch with at least one done and one truncation row, old log-probs = the f64 reference's
    log-prob + N(0, 0.3^2) (so all four clip cases can occur).  f32 values throughout."""
    rs = np.random.RandomState(seed)
    case = dict(K=K, B=B, in_dim=in_dim, activation=activation, hp={**HP, **hp},
                policy=random_net(rs, in_dim, hidden, 24), value=random_net(rs, in_dim, hidden, 1),
                normalizer=((rs.normal(scale=0.5, size=in_dim).astype(F), rs.uniform(0.5, 2.0, size=in_dim).astype(F))
                            if with_normalizer else None))
    done = (rs.uniform(size=(K, B)) < 0.2).astype(F)
    trunc = np.zeros((K, B), F)
    done[0, 0] = 1.0
    done[K - 1, B - 1] = trunc[K - 1, B - 1] = 1.0
    batch = dict(obs_all=rs.normal(size=(K + 1, B, in_dim)).astype(F), raw_action=rs.normal(scale=0.8, size=(K, B, 12)).astype(F),
                 reward=rs.normal(size=(K, B)).astype(F), done=done, truncation=trunc,
                 eps=rs.normal(size=(K, B, 12)).astype(F), log_prob=np.zeros((K, B), F))
    _, _, aux = loss_and_grad(case["policy"], case["value"], activation, batch, torch.float64, case["normalizer"], **case["hp"])
    batch["log_prob"] = (aux["logp"] + rs.normal(scale=0.3, size=(K, B))).astype(F)
    case["batch"] = batch
    return case


def reference(case, dtype):
    return loss_and_grad(case["policy"], case["value"], case["activation"], case["batch"], dtype, case["normalizer"],
                         **case["hp"])


def meets_conditions(case, aux):
    """On the f64 reference: every ReLU / ELU hidden pre-activation |z| >= 1e-4, every |rho - (1 +- eps)| >=
    1e-3, each of the four clip cases (rho high or low x advantage sign) present, std(adv) > 0."""
    e = case["hp"]["clipping_epsilon"]
    if case["activation"] in ("relu", "elu") and any(np.abs(z).min() < 1e-4 for z in aux["pre"]):
        return False
    rho, adv = aux["rho"], aux["adv"]
    if min(np.abs(rho - (1 + e)).min(), np.abs(rho - (1 - e)).min()) < 1e-3:
        return False
    hi, lo = rho > 1 + e, rho < 1 - e
    if not all(np.any(m) for m in (hi & (adv > 0), hi & (adv < 0), lo & (adv > 0), lo & (adv < 0))):
        return False
    return bool(aux["adv_raw"].std() > 0)


def cases_meeting_conditions(count, **kw):
    """The first `count` seeds (ascending from 0) whose case meets the conditions: [(case, f64 reference)]."""
    out, seed = [], 0
    while len(out) < count:
        case = random_case(seed, **kw)
        ref = reference(case, torch.float64)
        if meets_conditions(case, ref[2]):
            out.append((case, ref))
        seed += 1
        assert seed < 4000, "no seeds meet the conditions at this shape"
    return out


def rel_err(x, ref):
    """max |x - ref| / max |ref|"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def tensor_errors(metrics, grads, ref_metrics, ref_grads):
    """{name: rel_err} over the four metrics and every parameter tensor's gradient of both nets."""
    out = {k: rel_err(metrics[k], ref_metrics[k]) for k in METRICS}
    for net in ("policy", "value"):
        for i, ((dk, db), (rk, rb)) in enumerate(zip(grads[net], ref_grads[net])):
            out[f"{net}.{i}.kernel"] = rel_err(dk, rk)
            out[f"{net}.{i}.bias"] = rel_err(db, rb)
    return out
