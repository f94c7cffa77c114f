"""PPO value targets without a GPU: the f32 restatement of pp3_gae's recurrence (tests/ppo_ref.py)
against known answers in exactly representable numbers, the critic's export
(export.convert_value_params) and the argument checks of the new entry points that return before
any HIP call."""
import ctypes as C

import numpy as np
import pytest

import ppo_ref
from pupperv3_mjx import _lib, export
from test_export import _brax_like_params


def _kat(K, done=(), trunc=(), reward=1.0, values=3.0, bootstrap=4.0, discount=0.5, lam=0.5, scaling=2.0):
    d = np.zeros((K, 1), np.float32)
    tr = np.zeros((K, 1), np.float32)
    for t in done:
        d[t] = 1
    for t in trunc:
        tr[t] = 1
    vs, adv = ppo_ref.gae(np.full((K, 1), reward, np.float32), d, tr, np.full((K, 1), values, np.float32),
                          np.full((1,), bootstrap, np.float32), discount, lam, scaling)
    assert vs.dtype == np.float32 and adv.dtype == np.float32
    return vs[:, 0].tolist(), adv[:, 0].tolist()


@pytest.mark.parametrize("kw,vs,adv", [
    (dict(K=3), [3.6875, 3.75, 4.0], [0.875, 1.0, 1.0]),
    (dict(K=3, done=(1,)), [3.25, 2.0, 4.0], [0.0, -1.0, 1.0]),
    (dict(K=3, done=(1,), trunc=(1,)), [3.5, 3.0, 4.0], [0.5, 0.0, 1.0]),
    (dict(K=1), [4.0], [1.0]),
], ids=["no_done", "done_t1", "done_and_truncation_t1", "one_step"])
def test_restatement_known_answers(kw, vs, adv):
    """reward 1, reward_scaling 2, values 3, bootstrap 4, discount 0.5, lambda 0.5: every number is
    exactly representable, so equality is exact.  A termination cuts the bootstrap (g = 0); a
    truncation also zeroes the step's own delta and advantage and stops the accumulation."""
    got_vs, got_adv = _kat(**kw)
    assert got_vs == vs
    assert got_adv == adv


def test_lambda_one_is_the_discounted_return():
    """lambda = 1, no done: vs[t] = sum_k discount^k r_{t+k} + discount^(K-t) * bootstrap."""
    vs, adv = _kat(3, reward=1.0, values=0.0, bootstrap=0.0, discount=0.5, lam=1.0, scaling=1.0)
    assert vs == [1.75, 1.5, 1.0]
    assert adv == [1.75, 1.5, 1.0]


def test_restatement_rounds_every_operation():
    """A fused multiply-add of r + g * vnext would keep the product's low bits; the restatement
    does not: with g * vnext = (1 + 2^-12)^2 the 2^-24 term is rounded away before the sum."""
    x = np.float32(1 + 2.0 ** -12)
    vs, _ = ppo_ref.gae(np.array([[-1.0]], np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32),
                        np.zeros((1, 1), np.float32), np.array([x], np.float32), x, 0.0, 1.0)
    assert vs[0, 0] == np.float32(2.0 ** -11)  # an fma would give 2^-11 + 2^-24


@pytest.mark.parametrize("sizes,act", [([72, 64, 64, 1], "elu"), ([540, 256, 1], "relu")])
def test_convert_value_params(sizes, act):
    rs = np.random.RandomState(3)
    params = _brax_like_params(rs, sizes)
    H = sizes[0] // 36
    v = export.convert_value_params(params, act, H)
    assert set(v) == {"observation_history", "in_shape", "layers"}
    assert v["observation_history"] == H and v["in_shape"] == [None, sizes[0]]
    assert v["layers"][-1]["activation"] == "linear" and v["layers"][-1]["shape"] == [None, 1]
    assert all(layer["activation"] == act for layer in v["layers"][:-1])
    # folding the normalizer == normalising the input
    x = rs.normal(size=(5, sizes[0]))
    norm, tree = params
    plain = {"layers": [{"activation": layer["activation"],
                         "weights": [np.asarray(p["kernel"]), np.asarray(p["bias"])]}
                        for layer, p in zip(v["layers"], tree["params"].values())]}
    want = export.policy_forward(plain, (x - norm.mean) / norm.std)
    got = export.policy_forward(v, x)
    assert got.shape == (5, 1)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_convert_value_params_rejects_a_wide_head():
    with pytest.raises(ValueError):
        export.convert_value_params(_brax_like_params(np.random.RandomState(0), [72, 32, 24]), "elu", 2)


def test_device_less_policy_accepts_the_value_dict():
    v = export.convert_value_params(_brax_like_params(np.random.RandomState(0), [72, 64, 1]), "elu", 2)
    dp = export.DevicePolicy(v, device=-1)
    try:
        assert dp.out_dim == 1 and dp.in_dim == 72 and dp.distribution is None
        assert _lib.load().pp3_policy_out_dim(dp._h) == 1
    finally:
        dp.close()


def test_gae_argument_errors_before_any_hip_call():
    """pp3_gae validates before it touches a device: the pointers here are never dereferenced."""
    L = _lib.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(7)]  # reward done trunc values bootstrap vs adv

    def call(nsteps=3, n=4, stride=4, ptrs=p, discount=0.97, lam=0.95, scaling=1.0):
        return L.pp3_gae(0, nsteps, n, stride, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], discount, lam, scaling,
                         ptrs[5], ptrs[6], None)

    for i in range(7):
        q = list(p)
        q[i] = None
        assert call(ptrs=q) == 1, i
        assert b"null" in L.pp3_ppo_last_error()
    assert call(nsteps=0) == 1 and call(n=0) == 1
    assert call(n=5, stride=4) == 1 and b"row_stride" in L.pp3_ppo_last_error()
    for kw in (dict(discount=float("nan")), dict(lam=float("inf")), dict(scaling=float("-inf"))):
        assert call(**kw) == 1 and b"finite" in L.pp3_ppo_last_error()
    for out in (5, 6):
        for inp in range(5):
            q = list(p)
            q[out] = q[inp]
            assert call(ptrs=q) == 1 and b"in-place" in L.pp3_ppo_last_error(), (out, inp)
    assert L.pp3_set_truncation_trajectory(None, None, 0) == 1
