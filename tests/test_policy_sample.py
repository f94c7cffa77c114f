"""Host side of the stochastic (tanh-Gaussian) policy: rng.normal, the training export, the numpy
meaning of a sample (export.sample_forward) and the C ABI's argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from pupperv3_mjx import _lib, export, rng
from test_export import _brax_like_params

LO = np.nextafter(np.float32(-1.0), np.float32(0.0))
CONVERT_ARGS = (0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True)


def _want_normal(key, shape, part):
    from scipy.special import erfinv
    u = rng.uniform(key, shape, LO, 1.0, part)
    assert u.dtype == np.float32
    return (np.sqrt(2.0) * erfinv(u.astype(np.float64))).astype(np.float32)


@pytest.mark.parametrize("part", [True, False])
def test_normal_is_erfinv_of_the_jax_uniform(part):
    key = rng.PRNGKey(7)
    z = rng.normal(key, (37, 12), part)
    assert z.dtype == np.float32 and z.shape == (37, 12)
    np.testing.assert_array_equal(z, _want_normal(key, (37, 12), part))
    assert np.all(np.isfinite(z))
    # a batch of keys: one stream per key
    keys = rng.split(rng.PRNGKey(8), 5, part)
    zb = rng.normal(keys, (3, 12), part)
    assert zb.shape == (5, 3, 12) and np.all(np.isfinite(zb))
    for i in range(5):
        np.testing.assert_array_equal(zb[i], rng.normal(keys[i], (3, 12), part))


def test_normal_is_finite_at_the_ends_of_the_uniform():
    """bits 0 and bits 0xffffffff: the uniform's smallest value is nextafter(-1, 0), never -1, and
    its largest stays below 1, so erfinv is finite everywhere."""
    from scipy.special import erfinv
    z = rng.normal(rng.PRNGKey(0), (4096, 12))
    assert np.all(np.isfinite(z)) and 3.0 < np.abs(z).max() < 6.0
    for bits in (np.uint32(0), np.uint32(0xFFFFFFFF)):
        f = rng.bits_to_unit_float(np.array([bits], dtype=np.uint32))
        u = np.maximum(LO, (f * (np.float32(1.0) - LO) + LO).astype(np.float32))
        assert -1.0 < u[0] < 1.0 and np.isfinite(erfinv(u.astype(np.float64)))[0]


@pytest.mark.parametrize("part", [True, False])
def test_normal_moments(part):
    """(512, 12) draws from PRNGKey(11): mean and variance within four standard errors."""
    z = rng.normal(rng.PRNGKey(11), (512, 12), part).astype(np.float64)
    n = z.size
    assert n == 6144
    assert abs(z.mean()) <= 4 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n), z.var()


@pytest.mark.parametrize("sizes,act", [([72, 64, 24], "elu"), ([72, 128, 128, 24], "tanh"), ([36, 32, 24], "relu")])
def test_training_export_keeps_the_head_and_matches_deployment(sizes, act):
    params = _brax_like_params(np.random.RandomState(0), sizes)
    H = sizes[0] // 36
    dep = export.convert_params(params, act, *CONVERT_ARGS, H, 30.0, 30.0)
    tr = export.convert_training_params(params, act, *CONVERT_ARGS, H, 30.0, 30.0)
    assert tr["layers"][-1]["activation"] == "linear" and tr["layers"][-1]["shape"] == [None, 24]
    assert tr["distribution"] == {"type": "normal_tanh", "min_std": 0.001, "var_scale": 1.0}
    assert {k: v for k, v in tr.items() if k not in ("layers", "distribution")} == \
        {k: v for k, v in dep.items() if k != "layers"}
    x = np.random.RandomState(1).normal(size=(9, sizes[0]))
    np.testing.assert_allclose(np.tanh(export.policy_forward(tr, x)[:, :12]), export.policy_forward(dep, x),
                               rtol=0, atol=1e-12)
    tr2 = export.convert_training_params(params, act, *CONVERT_ARGS, H, 30.0, 30.0, min_std=0.01, var_scale=0.5)
    assert tr2["distribution"] == {"type": "normal_tanh", "min_std": 0.01, "var_scale": 0.5}


def _training_policy(sizes=(72, 64, 24), seed=0, **kw):
    params = _brax_like_params(np.random.RandomState(seed), list(sizes))
    return export.convert_training_params(params, "elu", *CONVERT_ARGS, sizes[0] // 36, 30.0, 30.0, **kw)


@pytest.mark.parametrize("part", [True, False])
def test_sample_forward_against_the_independent_form(part):
    """log_prob = sum [norm.logpdf(raw; loc, scale) - log(1 - tanh(raw)^2)] (scipy's normal, the
    textbook Jacobian), the noise is rng.normal's row-major stream, action = tanh(raw)."""
    from scipy.stats import norm
    pol = _training_policy()
    x = np.random.RandomState(2).normal(size=(29, 72))
    key = rng.PRNGKey(5)
    action, raw, logp, logits = export.sample_forward(pol, x, key, part)
    assert action.shape == raw.shape == (29, 12) and logp.shape == (29,) and logits.shape == (29, 24)
    np.testing.assert_array_equal(logits, export.policy_forward(pol, x))
    loc, s = logits[:, :12], logits[:, 12:]
    scale = (np.log1p(np.exp(s)) + 0.001) * 1.0
    z = rng.normal(key, (29, 12), part).astype(np.float64)
    np.testing.assert_allclose(raw, loc + scale * z, rtol=0, atol=1e-13)
    np.testing.assert_array_equal(action, np.tanh(raw))
    ok = (np.abs(raw) < 4).all(axis=-1)  # (where the textbook Jacobian is itself accurate)
    assert ok.sum() >= 8
    want = (norm.logpdf(raw, loc, scale) - np.log(1 - np.tanh(raw) ** 2)).sum(axis=-1)
    np.testing.assert_allclose(logp[ok], want[ok], rtol=0, atol=1e-9)
    assert np.all(np.isfinite(logp))


def test_log_prob_is_finite_for_saturated_actions():
    """|raw| up to 30: 1 - tanh(raw)^2 is 0 in float64 from |raw| ~ 19 (its log: -inf); the stable
    Jacobian 2 (log 2 - raw - softplus(-2 raw)) stays finite and agrees where both are."""
    from scipy.stats import norm
    rs = np.random.RandomState(3)
    logits = rs.normal(size=(40, 24))
    raw = rs.uniform(-30, 30, size=(40, 12))
    raw[0, :4] = [30.0, -30.0, 19.5, -19.5]
    lp = export.normal_tanh_log_prob(logits, raw)
    assert np.all(np.isfinite(lp))
    loc, scale = export.normal_tanh_scale(logits)
    ok = np.abs(raw) < 4
    stable = -2.0 * (np.log(2.0) - raw - np.logaddexp(0.0, -2.0 * raw))
    np.testing.assert_allclose(stable[ok], -np.log(1 - np.tanh(raw[ok]) ** 2), rtol=0, atol=1e-10)
    np.testing.assert_allclose(lp, (norm.logpdf(raw, loc, scale) + stable).sum(axis=-1), rtol=1e-12)
    # min_std / var_scale enter the scale
    _, sc2 = export.normal_tanh_scale(logits, min_std=0.01, var_scale=0.5)
    np.testing.assert_allclose(sc2, (np.logaddexp(0.0, logits[:, 12:]) + 0.01) * 0.5, rtol=1e-14)


def _host_handle(sizes, acts):
    """A policy handle without device memory (device < 0): the layer records only."""
    L = _lib.load()
    o = np.array(sizes[1:], dtype=np.int32)
    a = np.array([export.ACTIVATIONS[n] for n in acts], dtype=np.int32)
    w = np.zeros(sum(k * m + m for k, m in zip(sizes[:-1], sizes[1:])), dtype=np.float32)
    h = C.c_void_p()
    rc = L.pp3_policy_create(-1, sizes[0], len(o), o.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                             w.ctypes.data_as(C.c_void_p), C.byref(h))
    assert rc == 0, L.pp3_policy_last_error()
    return L, h


def test_set_distribution_rejects_what_the_head_cannot_run_without_gpu_work():
    L, h = _host_handle([72, 32, 12], ["elu", "linear"])
    try:
        assert L.pp3_policy_out_dim(h) == 12
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.001, 1.0) == 1
        assert b"out_dim 24" in L.pp3_policy_last_error()
    finally:
        L.pp3_policy_destroy(h)
    L, h = _host_handle([72, 32, 24], ["elu", "tanh"])
    try:
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.001, 1.0) == 1
        assert b"linear" in L.pp3_policy_last_error()
    finally:
        L.pp3_policy_destroy(h)
    L, h = _host_handle([72, 32, 24], ["elu", "linear"])
    try:
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, -0.5, 1.0) == 1
        assert b"min_std" in L.pp3_policy_last_error()
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, float("nan"), 1.0) == 1
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.001, 0.0) == 1
        assert b"var_scale" in L.pp3_policy_last_error()
        assert L.pp3_policy_set_distribution(h, 7, 0.001, 1.0) == 1
        assert b"kind" in L.pp3_policy_last_error()
        key = np.array([0, 1], dtype=np.uint32)
        kp = key.ctypes.data_as(C.c_void_p)
        # no distribution yet: sampling is refused
        assert L.pp3_policy_sample(h, C.c_void_p(16), 72, 4, kp, 1, C.c_void_p(16), 12, None, None, None, None) == 1
        assert b"distribution" in L.pp3_policy_last_error()
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.0, 1.0) == 0
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.001, 1.0) == 0
        # a host-side handle launches nothing
        assert L.pp3_policy_sample(h, C.c_void_p(16), 72, 4, kp, 1, C.c_void_p(16), 12, None, None, None, None) == 1
        assert b"host-side" in L.pp3_policy_last_error()
        assert L.pp3_policy_act(h, C.c_void_p(16), 72, 4, C.c_void_p(16), 12, None) == 1
    finally:
        L.pp3_policy_destroy(h)


def test_sample_entry_points_reject_null_arguments_without_gpu_work():
    L = _lib.load()
    key = np.array([0, 1], dtype=np.uint32)
    kout = np.zeros(2, dtype=np.uint32)
    kp, ko, p = key.ctypes.data_as(C.c_void_p), kout.ctypes.data_as(C.c_void_p), C.c_void_p(16)
    assert L.pp3_policy_set_distribution(None, export.DIST_NORMAL_TANH, 0.001, 1.0) == 1
    assert b"pp3_policy_set_distribution" in L.pp3_policy_last_error()
    assert L.pp3_policy_sample(None, p, 72, 4, kp, 1, p, 12, p, p, None, None) == 1
    assert b"pp3_policy_sample" in L.pp3_policy_last_error()
    L2, h = _host_handle([72, 32, 24], ["elu", "linear"])
    try:
        assert L.pp3_policy_set_distribution(h, export.DIST_NORMAL_TANH, 0.001, 1.0) == 0
        assert L.pp3_policy_sample(h, None, 72, 4, kp, 1, p, 12, p, p, None, None) == 1
        assert L.pp3_policy_sample(h, p, 72, 4, None, 1, p, 12, p, p, None, None) == 1
        assert L.pp3_policy_sample(h, p, 72, 4, kp, 1, None, 12, p, p, None, None) == 1
        assert b"null" in L.pp3_policy_last_error()
        assert L.pp3_rollout_policy_sample(None, h, 4, kp, ko, p, None, None, None, None, None, None) == 1
        assert b"pp3_rollout_policy_sample" in L.pp3_last_error()
    finally:
        L.pp3_policy_destroy(h)
    assert L.pp3_rollout_policy_sample(None, None, 4, kp, ko, p, None, None, None, None, None, None) == 1
    ms = C.c_float()
    assert L.pp3_rollout_policy_sample_timed(None, None, 4, kp, ko, p, None, None, None, None, None, C.byref(ms)) == 1
