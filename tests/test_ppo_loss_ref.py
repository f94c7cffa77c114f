"""Pins tests/ppo_loss_ref.py, the torch restatement of the PPO learner's contract, without the
device: its autograd gradient against central differences, its parts against the project's other
restatements (ppo_ref.gae, export.normal_tanh_log_prob, export.fold_in_normalization), the two
properties of the clipped surrogate, and the argument checks of the learner's entry points that need
no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_loss_ref as R
import ppo_ref
from pupperv3_mjx import _lib, export


def _case(seed=0, K=3, B=4, hidden=(6,), activation="tanh", with_normalizer=True, **hp):
    return R.random_case(seed, K=K, B=B, in_dim=36, hidden=hidden, activation=activation,
                         with_normalizer=with_normalizer, **hp)


def _flat(grads):
    return np.concatenate([a.ravel() for net in ("policy", "value") for kb in grads[net] for a in kb])


def test_autograd_gradient_equals_central_differences():
    """f64, 36 -> 6 -> 24 / 36 -> 6 -> 1: every parameter, the targets held fixed as the gradient holds them."""
    case = _case()
    _, grads, aux = R.reference(case, torch.float64)
    got = _flat(grads)
    targets = (aux["vs"], aux["adv_raw"])
    tensors = [np.asarray(a, dtype=np.float64) for net in ("policy", "value") for kb in case[net] for a in kb]
    n_pol = len(case["policy"])

    def total(ts):
        pairs = [(ts[2 * i], ts[2 * i + 1]) for i in range(len(ts) // 2)]
        with torch.no_grad():
            m, _ = R.loss(R.as_params(pairs[:n_pol], torch.float64), R.as_params(pairs[n_pol:], torch.float64),
                          case["activation"], case["batch"], torch.float64, case["normalizer"], targets=targets,
                          **case["hp"])
        return float(m["total_loss"])

    h, fd = 1e-6, []
    for a in tensors:
        flat = a.reshape(-1)  # a view: the perturbation is seen through `tensors`
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = total(tensors)
            flat[i] = keep - h
            dn = total(tensors)
            flat[i] = keep
            fd.append((up - dn) / (2 * h))
    fd = np.array(fd)
    assert got.shape == fd.shape == (36 * 6 + 6 + 6 * 24 + 24 + 36 * 6 + 6 + 6 + 1,)
    assert np.abs(got).max() > 1e-3
    assert np.abs(got - fd).max() <= 1e-7 * np.abs(got).max() + 1e-9, np.abs(got - fd).max()


def test_gae_part_equals_ppo_ref_bit_for_bit():
    case = _case(seed=3, K=5, B=7)
    b = case["batch"]
    _, _, aux = R.reference(case, torch.float32)
    want_vs, want_adv = ppo_ref.gae(b["reward"], b["done"], b["truncation"], aux["baseline"],
                                    _bootstrap(case), 0.97, 0.95, 1.0)
    case["hp"]["normalize_advantage"] = False
    _, _, aux = R.reference(case, torch.float32)
    np.testing.assert_array_equal(aux["vs"], want_vs)
    np.testing.assert_array_equal(aux["adv"], want_adv)
    assert b["done"].sum() >= 2 and b["truncation"].sum() >= 1


def _bootstrap(case):
    t = torch.float32
    obs = torch.as_tensor(case["batch"]["obs_all"], dtype=t)
    mean, std = case["normalizer"]
    with torch.no_grad():
        v = R.mlp((obs - torch.as_tensor(mean, dtype=t)) / torch.as_tensor(std, dtype=t), R.as_params(case["value"], t),
                  case["activation"])
    return v[-1, :, 0].numpy()


def test_log_prob_equals_export():
    case = _case(seed=4)
    _, _, aux = R.reference(case, torch.float64)
    want = export.normal_tanh_log_prob(aux["logits"], case["batch"]["raw_action"], 0.001, 1.0)
    np.testing.assert_allclose(aux["logp"], want, rtol=1e-13, atol=1e-13)


def test_policy_loss_vanishes_for_unchanged_parameters():
    """new = old parameters (rho = 1), normalised advantages: policy_loss = -mean(adv) = 0 to rounding."""
    case = _case(seed=5, K=4, B=9)
    _, _, aux = R.reference(case, torch.float64)
    case["batch"]["log_prob"] = aux["logp"]  # (f64: rho is exactly 1)
    m, _, aux = R.reference(case, torch.float64)
    assert np.all(aux["rho"] == 1.0)
    assert np.abs(aux["adv"]).max() > 0.5
    assert abs(m["policy_loss"]) < 1e-14


def test_clipped_rows_contribute_exactly_zero_policy_gradient():
    case = _case(seed=6, K=6, B=16)
    pol, val = R.as_params(case["policy"], torch.float64), R.as_params(case["value"], torch.float64)
    m, aux = R.loss(pol, val, case["activation"], case["batch"], torch.float64, case["normalizer"], **case["hp"])
    (g,) = torch.autograd.grad(m["policy_loss"], aux["logits"])
    rho, adv, e = aux["rho"].detach().numpy(), aux["adv"].detach().numpy(), case["hp"]["clipping_epsilon"]
    clipped = ((rho > 1 + e) & (adv > 0)) | ((rho < 1 - e) & (adv < 0))
    assert ((rho > 1 + e) & (adv > 0)).any() and ((rho < 1 - e) & (adv < 0)).any() and (~clipped).any()
    g = g.numpy()
    assert np.all(g[clipped] == 0.0)
    live = ~clipped & (adv != 0)
    assert np.all(np.abs(g[live]).max(axis=-1) > 0)


def test_adam_restatement_is_optax_adam():
    rs = np.random.RandomState(0)
    p, g, m, v = (rs.normal(size=257).astype(np.float32).astype(np.float64) for _ in range(4))
    v = (np.abs(v) * 1e-2).astype(np.float32).astype(np.float64)
    for t in (1, 3):
        p2, m2, v2 = R.adam(p, g, m, v, 3e-4, 0.9, 0.999, 1e-8, t)
        m64 = 0.9 * m + 0.1 * g
        v64 = 0.999 * v + 0.001 * g * g
        p64 = p - 3e-4 * (m64 / (1 - 0.9 ** t)) / (np.sqrt(v64 / (1 - 0.999 ** t)) + 1e-8)
        np.testing.assert_allclose(m2, m64, rtol=1e-6, atol=2e-7)  # (sums that cancel: 1 ulp of the terms)
        np.testing.assert_allclose(v2, v64, rtol=2e-5)  # (1 - f32(0.999) is 1.3e-5 off 0.001)
        np.testing.assert_allclose(p2 - p, p64 - p, rtol=1e-4, atol=2.0 ** -22)  # (1 ulp of |p| < 4)


def test_fold_restatement_is_the_export_fold():
    rs = np.random.RandomState(1)
    k, b, mean, std = rs.normal(size=(36, 5)), rs.normal(size=5), rs.normal(size=36), rs.uniform(0.5, 2, size=36)
    fk, fb = R.fold(k, b, mean, std)
    ek, eb = export.fold_in_normalization(k, b, mean, std)
    np.testing.assert_allclose(fk, ek, rtol=1e-15)
    np.testing.assert_allclose(fb, eb, rtol=1e-12, atol=1e-14)
    x = rs.normal(size=(3, 36))
    np.testing.assert_allclose(x @ fk + fb, ((x - mean) / std) @ k + b, rtol=1e-12, atol=1e-12)


def test_learner_entry_points_refuse_bad_arguments_without_gpu_work():
    """The checks that come before any HIP call."""
    L = _lib.load()
    h = C.c_void_p()
    one = (C.c_int32 * 1)(24)
    lin = (C.c_int32 * 1)(0)
    w = (C.c_float * (37 * 24))()
    vone = (C.c_int32 * 1)(1)
    # a policy that is not 24 wide, a value net that is not 1 wide, a null blob, max_rows
    assert L.pp3_learner_create(0, 36, 1, vone, lin, w, 1, vone, lin, w, 0.001, 1.0, 64, C.byref(h)) == 1
    assert L.pp3_learner_create(0, 36, 1, one, lin, w, 1, one, lin, w, 0.001, 1.0, 64, C.byref(h)) == 1
    assert L.pp3_learner_create(0, 36, 1, one, lin, None, 1, vone, lin, w, 0.001, 1.0, 64, C.byref(h)) == 1
    assert L.pp3_learner_create(0, 36, 1, one, lin, w, 1, vone, lin, w, 0.001, 1.0, 1, C.byref(h)) == 1
    assert L.pp3_learner_create(0, 36, 1, one, lin, w, 1, vone, lin, w, 0.001, 0.0, 64, C.byref(h)) == 1
    assert b"pp3_learner_create" in L.pp3_learn_last_error()
    assert L.pp3_ppo_loss_grad(None, 1, 1, 1, 0, *([None] * 9), 0.97, 0.95, 1.0, 0.3, 0.01, 1, None, None) == 1
    assert L.pp3_adam_step(None, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, None) == 1
    assert L.pp3_policy_load_params(None, None, 36, 1, one, None, None, None) == 1
    assert L.pp3_learner_buffers(None, 0, 0, None, None) == 1
    assert L.pp3_learner_destroy(None) == 0
